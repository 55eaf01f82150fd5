"""Run by tests/test_product_mutagenesis_profile.py in a subprocess WITHOUT MURAL_HIP_FLAVOR: the profile entry against its twin and one
small profile through the product library (libmural_hip.so) -- checks of tests/test_gpu_mutagenesis_profile.py."""
import ctypes
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    from mural_amd import _lib
    from tests import test_gpu_mutagenesis_profile as G
    assert _lib.flavor() == "product"
    handle = ctypes.CDLL(_lib.LIB_PATH)
    assert hasattr(handle, "mural_mutagenesis_profile_window")
    assert _lib.lib()._name == _lib.LIB_PATH
    G.test_device_entry_equals_the_twin_on_the_edge_rows(97, True)
    G.test_profile_equals_the_twin_of_the_map_and_does_not_depend_on_how_it_was_reached(2)
    print("PRODUCT_MUTAGENESIS_PROFILE_OK")


if __name__ == "__main__":
    main()
