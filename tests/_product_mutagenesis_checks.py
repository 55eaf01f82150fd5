"""Run by tests/test_product_mutagenesis.py in a subprocess WITHOUT MURAL_HIP_FLAVOR: the substitution encoder and one small
saturation-mutagenesis map through the product library (libmural_hip.so) -- the checks of tests/test_gpu_mutagenesis.py."""
import ctypes
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    from mural_amd import _lib
    from tests import test_gpu_mutagenesis as G
    assert _lib.flavor() == "product"
    handle = ctypes.CDLL(_lib.LIB_PATH)
    assert all(hasattr(handle, name) for name in ("mural_encode_subst_windows", "mural_mutagenesis_rows", "mural_mutagenesis_reduce"))
    assert _lib.lib()._name == _lib.LIB_PATH
    G.check_encoder((6, 5, 3))
    G.check_encoder((100, 7, 1))
    G.check_map(5, 100, 2, chunks=(97,), oracle_sample=200)
    print("PRODUCT_MUTAGENESIS_OK")


if __name__ == "__main__":
    main()
