"""Run by tests/test_product_alleles.py in a subprocess WITHOUT MURAL_HIP_FLAVOR: the allele encoder on one configuration and one small
INDEL allele footprint through the product library (libmural_hip.so) -- the checks of tests/test_gpu_alleles.py."""
import ctypes
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    from mural_amd import _lib
    from tests import test_gpu_alleles as G
    from tests.test_product_alleles import ENTRIES
    assert _lib.flavor() == "product"
    handle = ctypes.CDLL(_lib.LIB_PATH)
    assert all(hasattr(handle, name) for name in ENTRIES)
    assert _lib.lib()._name == _lib.LIB_PATH and _lib.lib().mural_abi_version() == 4
    G.test_allele_encoder_equals_the_plain_encoders_on_the_patched_genome((6, 5, 3), "snv")
    G.test_indel_allele_footprint()
    print("PRODUCT_ALLELES_OK")


if __name__ == "__main__":
    main()
