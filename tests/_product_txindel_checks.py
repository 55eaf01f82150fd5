"""Run by tests/test_product_txindel.py in a subprocess WITHOUT MURAL_HIP_FLAVOR: mural_summary_txindel_rows through the product library
(libmural_hip.so) -- the record of tests/_txindel_data.py in two calls per kind, against the numpy twin and the brute-force oracle."""
import ctypes
import io
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    import numpy as np
    from mural_amd import _lib
    from mural_amd.predict import summary_txindel_host
    from mural_amd.tables import read_transcript_structure
    from tests import _txindel_data as I
    from tests import test_gpu_summary_txindel as G
    assert _lib.flavor() == "product"
    handle = ctypes.CDLL(_lib.LIB_PATH)
    assert hasattr(handle, "mural_summary_txindel_rows") and hasattr(handle, "mural_summary_txindel_workspace_bytes")
    assert _lib.lib()._name == _lib.LIB_PATH
    assert int(_lib.lib().mural_summary_txindel_workspace_bytes(1000)) == 8192 + 8192 + 8192      # no guard bytes: the switch is not read
    seq, text, names = I.build()
    _, meta, segments, features = read_transcript_structure(io.StringIO(text))
    prob, start, label = I.rows(seq, 8, dtype=np.float32)
    for kind in (0, 1, 2):
        acc = None
        for rows in np.array_split(np.arange(len(start)), 2):
            acc, status = G._kernel(prob[rows], start[rows], label[rows], 8, segments["chr1"], features["chr1"], len(names), kind, into=acc)
            assert status == 0
        want = summary_txindel_host(prob, start, label, 8, segments["chr1"], features["chr1"], len(names), kind)
        assert G._same(acc, want, len(names))
        assert I.as_integers(*G._host(acc, len(names))) == I.oracle(text, prob, start, label, 8, kind, 1, I.pairs(None, 8))
    print("PRODUCT_SUMMARY_TXINDEL_OK")


if __name__ == "__main__":
    main()
