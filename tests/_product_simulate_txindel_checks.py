"""Run by tests/test_product_simulate_txindel.py in a subprocess WITHOUT MURAL_HIP_FLAVOR: mural_simulate_txindel_rows through the
product library (libmural_hip.so) -- the record of tests/_txindel_sim_data.py in two calls per kind, against the numpy twin."""
import ctypes
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    import numpy as np
    from mural_amd import _lib
    from tests import _txindel_sim_data as X
    from tests import test_gpu_simulate_txindel as G
    assert _lib.flavor() == "product"
    handle = ctypes.CDLL(_lib.LIB_PATH)
    assert hasattr(handle, "mural_simulate_txindel_rows") and hasattr(handle, "mural_simulate_txindel_workspace_bytes")
    assert _lib.lib()._name == _lib.LIB_PATH
    assert int(_lib.lib().mural_simulate_txindel_workspace_bytes(1000)) == 8192 + 8192 + 8192      # no guard bytes: the switch is not read
    names, segments, features = X.read(X.toy_text() + X.random_text(seed=1))
    prob, start, strand, _ = X.rows(1000, 8, dtype=np.float32)
    for kind in (0, 1, 2):
        table = None
        for rows in np.array_split(np.arange(len(start)), 2):
            table, status = G._kernel(prob[rows], start[rows], strand[rows], 8, segments, features, len(names), kind, 67, into=table)
            assert status == 0
        want, _ = G._twin(prob, start, strand, 8, segments, features, len(names), kind, 67)
        assert G._host(table, len(names), 67).tobytes() == want.tobytes() and want.any()
    print("PRODUCT_SIMULATE_TXINDEL_OK")


if __name__ == "__main__":
    main()
