"""Run by tests/test_product_conseq.py in a subprocess WITHOUT MURAL_HIP_FLAVOR: mural_summary_conseq_rows through the product library
(libmural_hip.so) -- the record of tests/_conseq_data.py in two calls, against the numpy twin and the brute-force oracle."""
import ctypes
import io
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    import numpy as np
    from mural_amd import _lib
    from mural_amd.predict import summary_conseq_host
    from mural_amd.tables import read_transcripts
    from tests import _conseq_data as D
    from tests import test_gpu_summary_conseq as G
    assert _lib.flavor() == "product"
    handle = ctypes.CDLL(_lib.LIB_PATH)
    assert hasattr(handle, "mural_summary_conseq_rows") and hasattr(handle, "mural_summary_conseq_workspace_bytes")
    assert _lib.lib()._name == _lib.LIB_PATH
    assert int(_lib.lib().mural_summary_conseq_workspace_bytes(1000)) == 8192 + 8192 + 8192      # no guard bytes: the switch is not read
    seq, text, names = D.build()
    _, meta, segments = read_transcripts(io.StringIO(text))
    prob, start, strand, label = D.rows(seq, dtype=np.float32)
    genome, acc = G._genome(seq), None
    for rows in np.array_split(np.arange(len(start)), 2):
        acc, status = G._kernel(genome, prob[rows], start[rows], strand[rows], label[rows], segments["chr1"], len(names), into=acc)
        assert status == 0
    want = summary_conseq_host(seq, prob, start, strand, label, segments["chr1"], len(names))
    assert G._same(acc, want, len(names))
    assert D.as_integers(*G._host(acc, len(names))) == D.oracle(seq, text, prob, start, strand, label)
    print("PRODUCT_SUMMARY_CONSEQ_OK")


if __name__ == "__main__":
    main()
