"""The host side of the observed-mutation labels of a regions run: ``label_sites_host`` -- the numpy
specification the device lookup is tested against -- against a plain dict lookup, and ``read_mutations`` (order, gzip, its four
refusals, which chromosomes of a list a regions run takes).  No GPU."""
import gzip

import numpy as np
import pytest

from mural_amd.data.genome import STATS_INIT, label_sites_host, new_label_stats
from mural_amd.data.ingest import read_mutations
from mural_amd.predict import mutations_for_regions


def _dict_labels(pos, strand, muts, check_strand):
    """One site at a time: (labels, matched rows, smallest list index of a matched entry on the other strand or STATS_INIT[1])."""
    by_start = {int(s): j for j, s in enumerate(muts[0])}
    label, matched, wrong = [], 0, STATS_INIT[1]
    for p, st in zip(pos.tolist(), strand.tolist()):
        j = by_start.get(p)
        label.append(0.0 if j is None else float(muts[2][j]))
        if j is not None:
            matched += 1
            if check_strand and int(muts[1][j]) != st:
                wrong = min(wrong, j)
    return np.array(label, np.float32), matched, wrong


@pytest.mark.parametrize("seed", range(6))
def test_host_labels_equal_a_dict_lookup(seed):
    rng = np.random.default_rng(seed)
    n, m = int(rng.integers(1, 400)), int(rng.integers(0, 200))
    pos = np.sort(rng.choice(1000, size=n, replace=False)).astype(np.int64)
    strand = rng.integers(0, 2, n).astype(np.uint8)
    m_start = np.sort(rng.choice(np.arange(-20, 1020), size=m, replace=False)).astype(np.int64)      # entries below pos[0] and above pos[-1]
    muts = (m_start, rng.integers(0, 2, m).astype(np.uint8), rng.integers(0, 4, m).astype(np.float32))
    for check in (True, False):
        want, matched, wrong = _dict_labels(pos, strand, muts, check)
        stats = new_label_stats()
        assert stats.tolist() == list(STATS_INIT) and stats.dtype == np.int64
        got = label_sites_host(pos, strand, muts, check, stats)
        assert got.dtype == np.float32 and np.array_equal(got, want)
        assert stats.tolist() == [matched, wrong]
        # two calls accumulate to the one-call result
        two, cut = new_label_stats(), n // 3
        parts = [label_sites_host(pos[a:b], strand[a:b], muts, check, two) for a, b in ((0, cut), (cut, n))]
        assert np.array_equal(np.concatenate(parts), want) and two.tolist() == [matched, wrong]


def test_host_labels_without_a_list_or_without_sites():
    pos, strand = np.array([3, 9], np.int64), np.array([0, 1], np.uint8)
    empty = (np.zeros(0, np.int64), np.zeros(0, np.uint8), np.zeros(0, np.float32))
    for muts in (None, empty):
        stats = new_label_stats()
        assert label_sites_host(pos, strand, muts, True, stats).tolist() == [0.0, 0.0] and stats.tolist() == list(STATS_INIT)
    stats = new_label_stats()
    one = (np.array([9], np.int64), np.array([0], np.uint8), np.array([0.0], np.float32))
    assert label_sites_host(pos[:0], strand[:0], one, True, stats).shape == (0,) and stats.tolist() == list(STATS_INIT)
    # a matched entry with score 0 counts as matched; its strand is checked like any other
    assert label_sites_host(pos, strand, one, True, stats).tolist() == [0.0, 0.0] and stats.tolist() == [1, 0]


ROWS = [("chrB", 70, 2, "+"), ("chrA", 500, 1, "-"), ("chrA", 12, 3, "+"), ("chrB", 5, 1, "-"), ("chrA", 13, 0, "-"), ("chrA", 499, 2, "+")]


def _bed(path, rows, opener=open):
    with opener(path, "wt") as fh:
        fh.write("".join(f"{c}\t{s}\t{s + 1 if e is None else e}\t.\t{sc}\t{st}\n" for c, s, sc, st, e in
                         ((*r, None) if len(r) == 4 else r for r in rows)))
    return str(path)


def _check_rows(got):
    assert sorted(got) == ["chrA", "chrB"]
    a, b = got["chrA"], got["chrB"]
    assert [x.dtype for x in a] == [np.int64, np.uint8, np.float32]
    assert a[0].tolist() == [12, 13, 499, 500] and a[1].tolist() == [0, 1, 0, 1] and a[2].tolist() == [3.0, 0.0, 2.0, 1.0]
    assert b[0].tolist() == [5, 70] and b[1].tolist() == [1, 0] and b[2].tolist() == [1.0, 2.0]


def test_read_mutations_sorts_unsorted_input(tmp_path):
    _check_rows(read_mutations(_bed(tmp_path / "m.bed", ROWS)))
    _check_rows(read_mutations(_bed(tmp_path / "m.bed", ROWS), n_class=4))


def test_read_mutations_reads_gzip(tmp_path):
    _check_rows(read_mutations(_bed(tmp_path / "m.bed.gz", ROWS, gzip.open)))


@pytest.mark.parametrize("bad,n_class,where", [
    (("chrA", 499, 1, "-"), None, "chrA:499"),                     # the same (chrom, start) twice, whatever the strand and the score
    (("chrB", 80, 1, "+", 82), None, "chrB:80"),                   # end != start + 1
    (("chrB", 81, 1, "+", 81), None, "chrB:81"),
    (("chrA", 40, "1.5", "+"), None, "chrA:40"),                   # a score that is no integer >= 0
    (("chrA", 41, -1, "+"), None, "chrA:41"),
    (("chrB", 90, 4, "+"), 4, "chrB:90"),                          # a score >= n_class
])
def test_read_mutations_refuses(tmp_path, bad, n_class, where):
    path = _bed(tmp_path / "bad.bed", ROWS[:3] + [bad] + ROWS[3:])
    with pytest.raises(ValueError) as err:
        read_mutations(path, n_class=n_class)
    assert where in str(err.value)
    if n_class is not None:                                        # ... and only with n_class
        assert read_mutations(path)["chrB"][2].max() == 4.0


def test_a_regions_run_takes_its_own_chromosomes_from_the_list(tmp_path):
    muts = read_mutations(_bed(tmp_path / "m.bed", ROWS))
    regions = {"chrA": [(0, 13), (499, 500)], "chrC": [(0, 100)]}
    taken = mutations_for_regions(muts, regions)
    # chrB is listed and no region names it: ignored.  chrC has regions and no list: every label 0
    assert sorted(taken) == ["chrA", "chrC"] and taken["chrC"] == (None, 0)
    listed, inside = taken["chrA"]
    assert listed is muts["chrA"] and inside == 2                  # 12 and 499; 13 and 500 lie just outside their regions
    pos, strand = np.arange(0, 100, dtype=np.int64), np.zeros(100, np.uint8)
    stats = new_label_stats()
    assert not label_sites_host(pos, strand, taken["chrC"][0], True, stats).any() and stats.tolist() == list(STATS_INIT)
    assert mutations_for_regions(muts, {"chrA": [(0, 1 << 62)], "chrB": [(6, 70)]}) == {"chrA": (muts["chrA"], 4), "chrB": (muts["chrB"], 0)}
