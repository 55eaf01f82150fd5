"""Run by tests/test_product_mutagenesis_indel.py in a subprocess WITHOUT MURAL_HIP_FLAVOR: ``mural_indel_forward_symbols`` and one
2-site INDEL saturation-mutagenesis map through the product library (libmural_hip.so) -- the checks of tests/test_gpu_mutagenesis_indel.py."""
import ctypes
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    from mural_amd import _lib
    from tests import test_gpu_mutagenesis_indel as G
    from tests.test_product_mutagenesis_indel import ENTRIES
    assert _lib.flavor() == "product"
    handle = ctypes.CDLL(_lib.LIB_PATH)
    assert all(hasattr(handle, name) for name in ENTRIES)
    assert _lib.lib()._name == _lib.LIB_PATH and _lib.lib().mural_abi_version() == 4
    res = G.check_map(chunks=(4096,))
    assert res.delta.shape[0] == 2
    print("PRODUCT_MUTAGENESIS_INDEL_OK")


if __name__ == "__main__":
    main()
