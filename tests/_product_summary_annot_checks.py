"""Run by tests/test_product_summary_annot.py in a subprocess WITHOUT MURAL_HIP_FLAVOR: mural_summary_annot_rows through the product
library (libmural_hip.so) -- the literal BED's two chromosomes into one table, against the numpy twin and the brute-force oracle."""
import ctypes
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    import numpy as np
    from mural_amd import _lib
    from mural_amd.predict import summary_annot_host
    from mural_amd.tables import read_annotations
    from tests import _annot_data as D
    from tests import test_gpu_summary_annot as G
    assert _lib.flavor() == "product"
    handle = ctypes.CDLL(_lib.LIB_PATH)
    assert hasattr(handle, "mural_summary_annot_rows") and hasattr(handle, "mural_summary_annot_workspace_bytes")
    assert _lib.lib()._name == _lib.LIB_PATH
    names, _, pieces = read_annotations(D.intervals_dict())
    per_chrom = {"chrA": D.rows(300, 4, 0), "chrB": D.rows(40, 4, 1, lo=0, hi=70, hole=(62, 64))}
    table, want = None, None
    for chrom, (prob, start, label) in per_chrom.items():
        table, status = G._kernel(prob, start, label, 4, pieces[chrom], len(names), into=table)
        assert status == 0
        want, _ = summary_annot_host(prob, start, label, 4, pieces[chrom], len(names), into=want)
    got = G._host(table, len(names), 4)
    assert np.array_equal(got, want) and D.as_integers(got) == D.oracle(per_chrom, 4, names)
    print("PRODUCT_SUMMARY_ANNOT_OK")


if __name__ == "__main__":
    main()
