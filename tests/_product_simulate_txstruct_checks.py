"""Run by tests/test_product_simulate_txstruct.py in a subprocess WITHOUT MURAL_HIP_FLAVOR: mural_simulate_txstruct_rows through the
product library (libmural_hip.so) -- the record of tests/_txstruct_data.py in two calls, against the numpy twin."""
import ctypes
import io
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    import numpy as np
    from mural_amd import _lib
    from mural_amd.tables import read_transcript_structure
    from tests import _txstruct_data as S
    from tests import test_gpu_simulate_txstruct as G
    assert _lib.flavor() == "product"
    handle = ctypes.CDLL(_lib.LIB_PATH)
    assert hasattr(handle, "mural_simulate_txstruct_rows") and hasattr(handle, "mural_simulate_txstruct_workspace_bytes")
    assert _lib.lib()._name == _lib.LIB_PATH
    assert int(_lib.lib().mural_simulate_txstruct_workspace_bytes(1000)) == 8192 + 8192 + 8192      # no guard bytes: the switch is not read
    seq, text, names = S.build()
    _, meta, segments, features = read_transcript_structure(io.StringIO(text))
    prob, start, strand, _ = S.rows(seq, dtype=np.float32)
    genome, table = G._genome(seq), None
    for rows in np.array_split(np.arange(len(start)), 2):
        table, status = G._kernel(genome, prob[rows], start[rows], strand[rows], segments["chr1"], features["chr1"], len(names), 70, into=table)
        assert status == 0
    want, _ = G._twin(seq, prob, start, strand, segments["chr1"], features["chr1"], len(names), 70)
    assert G._host(table, len(names), 70).tobytes() == want.tobytes() and want.any()
    print("PRODUCT_SIMULATE_TXSTRUCT_OK")


if __name__ == "__main__":
    main()
