"""Run by tests/test_product_epoch_loader.py in a subprocess WITHOUT MURAL_HIP_FLAVOR: the epoch loader through the product library
(libmural_hip.so) -- the symbol resolves there, and its batches equal the old route's on the fixture of the debug-flavour tests."""
import ctypes
import os
import pathlib
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    from mural_amd import _lib
    from tests import _loader_data as D
    assert _lib.flavor() == "product"
    assert hasattr(ctypes.CDLL(_lib.LIB_PATH), "mural_train_batch_encode")
    assert _lib.lib()._name == _lib.LIB_PATH
    with tempfile.TemporaryDirectory() as tmp:
        fa, bed = D.write_fixture(pathlib.Path(tmp))
        for model_type in ("snv", "indel"):
            old = D.old_route(fa, bed, model_type, True, seed=3)
            D.assert_batches_equal(D.new_route(D.make_loader(fa, bed, model_type), True, seed=3), old, dense=model_type == "indel")
    print("PRODUCT_LOADER_OK")


if __name__ == "__main__":
    main()
