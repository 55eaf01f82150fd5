"""Run by tests/test_product_simulate.py in a subprocess WITHOUT MURAL_HIP_FLAVOR: mural_simulate_annot_rows and mural_simulate_rows
through the product library (libmural_hip.so) -- one table and one mutation list against the numpy twins."""
import ctypes
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    import numpy as np
    from mural_amd import _lib
    from mural_amd.summaries import simulate_rows_host
    from tests import test_gpu_simulate as G
    assert _lib.flavor() == "product"
    handle = ctypes.CDLL(_lib.LIB_PATH)
    assert hasattr(handle, "mural_simulate_annot_rows") and hasattr(handle, "mural_simulate_rows")
    assert _lib.lib()._name == _lib.LIB_PATH
    prob, start, strand = G._rows(300, 4, np.float32, seed=1)
    pieces, n_groups = G._pieces_for(start)
    got, status = G._annot(prob, start, strand, 4, pieces, n_groups, 7)
    want, _ = G._twin(prob, start, strand, 4, pieces, n_groups, 7)
    assert status == 0 and want.sum() > 0 and np.array_equal(G._host(got, n_groups, 4, 7), want)
    (got_start, got_strand, got_label), status = G._list(prob, start, strand, 4, 6)
    label = simulate_rows_host(prob, start, strand, 4, G.KEY, G.SEED, [6])[:, 0]
    assert status == 0 and np.array_equal(got_start, start[label > 0]) and np.array_equal(got_label, label[label > 0])
    assert np.array_equal(got_strand, strand[label > 0])
    print("PRODUCT_SIMULATE_OK")


if __name__ == "__main__":
    main()
