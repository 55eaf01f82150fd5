"""Annotation summaries on the host (CPU): ``tables.read_annotations`` on a literal BED, the numpy twin ``summary_annot_host`` against a
brute-force oracle of Python integers, and ``SummarySink(annotations=...)`` on host shards -- bit-identical for any split into parts,
its two files, abort()."""
import gzip
import os

import numpy as np
import pytest

from tests import _annot_data as D


def _write(tmp_path, text=D.BED, name="annot.bed", gz=False):
    path = tmp_path / name
    if gz:
        with gzip.open(path, "wt") as fh:
            fh.write(text)
    else:
        path.write_text(text)
    return str(path)


# ---- read_annotations ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("gz", [False, True])
def test_read_annotations_names_meta_and_merged_pieces(tmp_path, gz):
    from mural_amd.tables import read_annotations
    names, meta, pieces = read_annotations(_write(tmp_path, gz=gz, name="a.bed.gz" if gz else "a.bed"))
    assert names == D.NAMES                                   # first appearance; the three-column row is named chrom:start-end
    assert meta["exons"] == (3, 90)                           # 100-150 + 140-180 + 180-190 -> one piece 100-190
    assert meta["gene"] == (4, 10 + 10 + 10 + 50)             # three exons on chrA and one on chrB
    assert meta["outer"] == (2, 400 + 30) and meta["inner"] == (1, 100) and meta["chrA:120-121"] == (1, 1)
    assert sorted(pieces) == ["chrA", "chrB", "chrC"]
    g = {nm: j for j, nm in enumerate(names)}
    b0, b1, grp = pieces["chrA"]
    assert b0.dtype == np.int64 and b1.dtype == np.int64 and grp.dtype == np.int32
    got = list(zip(b0.tolist(), b1.tolist(), grp.tolist()))
    assert got == sorted(got)                                 # sorted by (b0, b1, group)
    assert (100, 190, g["exons"]) in got and sum(1 for p in got if p[2] == g["exons"]) == 1
    assert [p[:2] for p in got if p[2] == g["gene"]] == [(210, 220), (250, 260), (700, 710)]
    assert (200, 600, g["outer"]) in got and (300, 400, g["inner"]) in got      # nested pieces of different names both stay
    assert list(zip(*(x.tolist() for x in pieces["chrB"]))) == [(0, 30, g["outer"]), (10, 60, g["gene"])]
    # a name's pieces are disjoint and do not touch
    for chrom, (b0, b1, grp) in pieces.items():
        for j in set(grp.tolist()):
            a, b = b0[grp == j], b1[grp == j]
            assert (a[1:] > b[:-1]).all()
    assert read_annotations((names, meta, pieces))[0] is names      # its own result passes through


def test_read_annotations_refuses_bad_rows_with_file_and_line(tmp_path):
    from mural_amd.tables import read_annotations
    path = _write(tmp_path, "chr1\t5\t9\ta\nchr1\t-1\t9\tb\n", "neg.bed")
    with pytest.raises(ValueError, match=r"neg\.bed:2"):
        read_annotations(path)
    path = _write(tmp_path, "# c\nchr1\t5\t9\ta\nchr1\t7\t7\tb\n", "empty.bed")
    with pytest.raises(ValueError, match=r"empty\.bed:3"):
        read_annotations(path)


# ---- the twin against the oracle ------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def data(tmp_path_factory):
    from mural_amd.tables import read_annotations
    annot = read_annotations(_write(tmp_path_factory.mktemp("annot")))
    per_chrom = {"chrA": D.rows(300, 4, 0), "chrB": D.rows(40, 4, 1, lo=0, hi=70, hole=(62, 64))}
    return annot, per_chrom, D.oracle(per_chrom, 4, annot[0])


def test_twin_equals_the_brute_force_oracle(data):
    from mural_amd.predict import summary_annot_host
    (names, meta, pieces), per_chrom, want = data
    assert len(names) == 12 and len(per_chrom["chrA"][1]) == 300
    table = None
    for chrom, (prob, start, label) in per_chrom.items():
        perm = np.random.default_rng(3).permutation(len(start))      # rows shuffled
        table, status = summary_annot_host(prob[perm], start[perm], label[perm], 4, pieces[chrom], len(names), into=table)
        assert status == 0
    assert table.dtype == np.uint64 and table.shape == (12, 3, 4)
    got = D.as_integers(table)
    assert got == want
    by = dict(zip(names, got))
    assert sum(by["everything"][0]) == 300 and sum(by["outer"][0]) > sum(by["inner"][0]) > 0
    for empty in ("past", "gap", "before", "never"):
        assert by[empty] == ([0] * 4, [0] * 4)
    assert sum(by["chrA:120-121"][0]) >= 2 and sum(by["last"][0]) >= 1       # duplicate starts count each
    start = per_chrom["chrA"][1]
    assert sum(by["dup_end"][0]) == int(((start >= 640) & (start < 650)).sum()) >= 3      # the run at 650 is outside, the one at 640 inside


def test_twin_skips_bad_rows_and_reports_them(data):
    from mural_amd.predict import summary_annot_host
    (names, meta, pieces), per_chrom, _ = data
    prob, start, label = (a.copy() for a in per_chrom["chrA"])
    whole, _ = summary_annot_host(prob, start, label, 4, pieces["chrA"], len(names))
    prob[10, 1], prob[20, 2], label[30], start[0] = np.nan, 1.5, 4, -3
    got, status = summary_annot_host(prob, start, label, 4, pieces["chrA"], len(names))
    assert status == 1 | 2 | 8
    keep = np.ones(300, bool)
    keep[[0, 10, 20, 30]] = False
    want, status = summary_annot_host(per_chrom["chrA"][0][keep], per_chrom["chrA"][1][keep], per_chrom["chrA"][2][keep], 4, pieces["chrA"],
                                      len(names))
    assert status == 0 and np.array_equal(got, want) and not np.array_equal(got, whole)
    none, status = summary_annot_host(prob, start, label, 4, None, len(names))
    assert not none.any()


# ---- the sink on host shards ----------------------------------------------------------------------------------------------------------------
def _shards(per_chrom, parts, k=4):
    for chrom, (prob, start, label) in per_chrom.items():
        perm = np.random.default_rng(parts).permutation(len(start))
        for rows in np.array_split(perm, parts):
            yield {"chrom": chrom, "start": start[rows], "end": start[rows] + 1, "strand": np.zeros(len(rows), np.uint8), "label": label[rows],
                   "prob": prob[rows], "n_class": k, "calibrated": False}


def _sink(data, parts, prefix=None, **kw):
    from mural_amd.predict import SummarySink
    annot, per_chrom, _ = data
    sink = SummarySink(prefix, annotations=annot, **kw)
    for shard in _shards(per_chrom, parts):
        sink(shard)
    sink.close()
    return sink


def test_sink_is_bit_identical_for_one_two_and_seven_parts_and_writes_both_files(data, tmp_path):
    from mural_amd import tables
    (names, meta, _), per_chrom, want = data
    sinks = [_sink(data, parts, str(tmp_path / f"p{parts}")) for parts in (1, 2, 7)]
    assert D.as_integers(sinks[0].annotation_sums()) == want
    for s in sinks[1:]:
        assert s.annotation_sums().tobytes() == sinks[0].annotation_sums().tobytes()
        assert s.result()["annotations"][2].tobytes() == sinks[0].result()["annotations"][2].tobytes()
    got_names, got_meta, table = sinks[0].result()["annotations"]
    assert got_names == names and got_meta.dtype == np.int64 and got_meta.tolist() == [list(meta[nm]) for nm in names]
    assert table.shape == (12, 9) and table.dtype == np.float64
    for j, (counts, sums) in enumerate(want):
        assert table[j, 0] == sum(counts) and table[j, 1:5].tolist() == counts
        assert table[j, 5:].tolist() == [v / (1 << 71) for v in sums]
    rates, corr = (str(tmp_path / f"p1.annotation.{ext}") for ext in ("mut_rates.tsv", "corr.txt"))
    assert (rates, corr) == tables.annotation_output_names(str(tmp_path / "p1"))
    lines = open(rates).read().splitlines()
    assert lines[0].split("\t") == (["name", "n_intervals", "length", "number_of_all"] + [f"number_of_mut{c}" for c in (1, 2, 3)]
                                    + [f"expected_mut{c}" for c in (1, 2, 3)])
    assert [ln.split("\t")[0] for ln in lines[1:]] == names
    j = names.index("gene")
    counts, sums = want[j]
    assert lines[1 + j].split("\t") == (["gene", "4", "80", str(sum(counts))] + [str(c) for c in counts[1:]]
                                        + [repr(v / (1 << 71)) for v in sums[1:]])
    assert lines[1 + names.index("never")].split("\t") == ["never", "1", "45", "0", "0", "0", "0", "0.0", "0.0", "0.0"]
    used = table[:, 0] > 0
    want_corr = "".join("annotation\t%d\t%.5f\t%.10e\n" % ((c,) + tables.pearson(table[used, 1 + c], table[used, 5 + c])) for c in (1, 2, 3))
    assert open(corr).read() == want_corr
    for p in (2, 7):
        assert open(str(tmp_path / f"p{p}.annotation.mut_rates.tsv")).read() == open(rates).read()


def test_sink_without_labels_writes_nan_correlations_and_abort_removes_both_files(data, tmp_path):
    from mural_amd.predict import SummarySink
    annot, per_chrom, _ = data
    prefix = str(tmp_path / "q")
    sink = SummarySink(prefix, annotations=annot)
    for shard in _shards(per_chrom, 2):
        sink(dict(shard, label=np.zeros_like(shard["label"])))
    sink.close()
    paths = [prefix + ".annotation.mut_rates.tsv", prefix + ".annotation.corr.txt"]
    assert all(os.path.exists(p) for p in paths)
    assert [ln.split("\t")[2] for ln in open(paths[1]).read().splitlines()] == ["nan"] * 3
    sink.abort()
    assert not any(os.path.exists(p) for p in paths)
    with pytest.raises(RuntimeError):
        sink.result()


def test_sink_runs_annotations_beside_the_window_tables(data, tmp_path):
    sink = _sink(data, 2, str(tmp_path / "w"), windows=(1000,))
    assert sorted(os.listdir(tmp_path)) == sorted(f"w.{kind}.{ext}" for kind in ("1Kb", "annotation") for ext in ("corr.txt", "mut_rates.tsv"))
    assert D.as_integers(sink.annotation_sums()) == data[2]
