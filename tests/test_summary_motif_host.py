"""The numpy twin of the motif reduction (mural_amd.predict.summary_motif_host -- the specification csrc/summary_kmer.hip's
mural_summary_motif_rows is tested against) on the CPU: against a row-by-row brute force in Python strings, dicts and Fractions, and
against what the reference's calc_motif_corr.run_motif_corr_calc wrote for the same tables (tests/golden/motif.npz)."""
import numpy as np
import pytest

from tests import _motif_data as D

PARAMS = [(name, m) for name in D.CASES for m in D.MOTIFS]


@pytest.fixture(scope="module")
def twin():
    return {name: D.twin_tables(name) for name in D.CASES}


@pytest.mark.parametrize("name,m", PARAMS)
def test_twin_equals_brute_force(twin, name, m):
    """Counts, quantised sums, first windows, order and names: all exact."""
    want, _ = D.brute_force(name, m)
    got = D.sums_as_dict(*twin[name][m], m)
    assert list(got) == list(want)
    assert got == want


def test_float32_probabilities_are_widened_exactly():
    """... and probabilities below the 2^-71 quantum round half to even, 0 and 1 are the ends of the range."""
    p32 = {ch: cols[0].astype(np.float32) for ch, cols in D.case("snv")["rows"].items()}
    for j, v in enumerate(D.TINY):
        p32["chrM2"][1000 + j, 1 + j % 3] = v
    want, _ = D.brute_force("snv", 5, prob_of=p32)
    assert D.sums_as_dict(*D.twin_tables("snv", (5,), prob_of=p32)[5], 5) == want


@pytest.mark.parametrize("name", D.CASES)
def test_the_data_holds_the_cases_it_promises(name):
    c = D.case(name)
    indel = c["model_type"] == "indel"
    long_name, short_name = D.CHROMS[0][0], D.CHROMS[1][0]
    assert sorted(c["rows"]) != list(c["rows"]) and 2500 < sum(len(v[1]) for v in c["rows"].values()) < 3500
    for m in D.MOTIFS:
        want, empty = D.brute_force(name, m)
        names = list(want)
        # both orientations of the name rule: entries named by the larger of the pair (its reverse complement would sort first) and by the smaller
        assert any(n > D.revcomp(n) for n in names) and any(n < D.revcomp(n) for n in names)
        # the short chromosome's first windows come after the long one's although its name sorts first
        assert {w[2][0] for w in want.values()} == {0, 1} or m < 7
        # a row in the homopolymer run adds m (INDEL m - 1) times to one cell
        prob, start, end, label = c["rows"][long_name]
        r = int(np.nonzero((start == D.HOMOPOLYMER[0] + 11) & (end == start + 1))[0][0])
        assert [w for _, w in D.windows(D.SEQS[long_name], start[r], end[r], m, indel)] == ["A" * m] * (m - indel)
        # Ns cut some windows of a row, all windows of another
        kept = [len(D.windows(D.SEQS[long_name], s, e, m, indel)) for s, e in zip(start, end)]
        one_base = end == start + 1
        assert 0 in kept and any(0 < k < m - indel for k, o in zip(kept, one_base) if o)
        # slice starts that go negative and wrap: none of them is m bases long (see the data module), on either chromosome
        for ch, (_, st, en, _) in c["rows"].items():
            seq, wrapped = D.SEQS[ch], 0
            for s, e in zip(st, en):
                for i in range(1 if indel else 0, m):
                    a, b = (s - i + 1, e + m - i) if indel else (s - i, e + m - 1 - i)
                    if a < 0:
                        wrapped += 1
                        assert len(seq[int(a):int(b)]) != m
            assert wrapped > 0
        if indel:                      # a row longer than a base keeps exactly the windows the chromosome's end clips to m bases
            long_rows = [(s, e) for s, e in zip(start, end) if e - s > 1]
            assert any(D.windows(D.SEQS[long_name], s, e, m, True) for s, e in long_rows)
            assert all(e + m - i > len(D.SEQS[long_name]) for s, e in long_rows for i, _ in D.windows(D.SEQS[long_name], s, e, m, True))
        if m == 3:
            assert empty <= D.NO_WINDOW_CAP * sum(len(v[1]) for v in c["rows"].values())


@pytest.mark.parametrize("name,m", PARAMS)
def test_twin_reproduces_the_reference_s_recorded_output(twin, name, m, tmp_path):
    """Names and their order and every count exact; rates within 1e-12 relative and the correlation lines as tests/test_gpu_tables.py
    holds ``tables.kmer_table`` to tables.npz (label, class and r to five decimals as text, p within 1e-9 relative)."""
    from mural_amd import tables
    from mural_amd.predict import motif_table_from_sums
    nc = D.CASES[name]["n_class"]
    names, obs, pred, counts, corr_lines = D.golden(name, m)
    got_names, table = motif_table_from_sums(*twin[name][m], m, nc)
    assert got_names == names
    assert np.array_equal(table[:, 2:1 + nc], counts[:, :-1]) and np.array_equal(table[:, 0], counts[:, -1])
    assert np.array_equal(table[:, 1:1 + nc].sum(axis=1), counts[:, -1])
    g_obs, g_pred, _, tot = tables._rates(table, nc)
    assert np.array_equal(g_obs, obs)
    assert (np.abs(g_pred - pred) <= 1e-12 * np.abs(pred)).all()
    # the share of rows without a window, against the reference's counts: every kept window of an SNV row at m = 3 is counted once
    if m == 3:
        _, empty = D.brute_force(name, 3)
        rows = sum(len(v[1]) for v in D.case(name)["rows"].values())
        assert empty <= D.NO_WINDOW_CAP * rows and counts[:, -1].sum() >= (3 - (nc == 8)) * (1 - D.NO_WINDOW_CAP) * rows * 0.9
    # the two files, through the writer the sink and the table route share
    tables.write_motif_outputs(got_names, table, nc, m, str(tmp_path / "o"))
    rates_path, corr_path = tables.motif_output_names(str(tmp_path / "o"), m)
    got_lines = open(corr_path).read().split("\n")[:-1]
    assert len(got_lines) == len(corr_lines) == nc - 1
    for g, w in zip(got_lines, corr_lines):
        g, w = g.split("\t"), w.split("\t")
        assert g[:3] == w[:3] and g[0] == f"{m}-moitf"
        assert float(g[3]) == float(w[3]) or abs(float(g[3]) - float(w[3])) <= 1e-9 * abs(float(w[3]))
    head = open(rates_path).readline().rstrip("\n").split("\t")
    assert head == np.load(D.GOLDEN)[f"{name}/motif{m}/rates"].item().split("\n")[0].split("\t")


def test_refused_input():
    from mural_amd import tables
    from mural_amd.predict import SummarySink, summary_motif_host
    prob, start, end, label = (a[:50].copy() for a in D.case("snv")["rows"]["chrM2"])
    seq = D.SEQS["chrM2"]
    for m in (4, 1, 0, -3, 2):
        with pytest.raises(ValueError, match="positive odd integer >1"):
            summary_motif_host(seq, prob, start, end, label, 4, (m,))
        with pytest.raises(ValueError, match="positive odd integer >1"):
            tables.check_motif_length(m)
        with pytest.raises(ValueError, match="positive odd integer >1"):
            SummarySink(motifs=(m,), genome=lambda name: seq)
    for m in (3, 5, 7, 9, tables.MAX_MOTIF):
        assert tables.check_motif_length(m) == m
    with pytest.raises(ValueError, match="larger than"):
        tables.check_motif_length(tables.MAX_MOTIF + 2)
    with pytest.raises(ValueError, match="genome="):
        SummarySink(motifs=(3,))
    clean, status = summary_motif_host(seq, np.delete(prob, 7, 0), np.delete(start, 7), np.delete(end, 7), np.delete(label, 7), 4, (3,))
    assert status == 0
    for what, bit, message in (("nan", 8, "NaN, negative or above 1"), ("label", 2, "mut_type outside"), ("start", 1, "negative start")):
        p, s, lab = prob.copy(), start.copy(), label.copy()
        if what == "nan":
            p[7, 2] = np.nan
        elif what == "label":
            lab[7] = 4
        else:
            s[7] = -2
        got, status = summary_motif_host(seq, p, s, end, lab, 4, (3,))
        assert status == bit                       # the row is left out of the table ...
        assert np.array_equal(got[3][0], clean[3][0]) and np.array_equal(got[3][1], clean[3][1])
        sink = SummarySink(motifs=(3,), genome=lambda name: seq)      # ... and a sink that met it raises at close()
        sink({"chrom": "chrM2", "start": s, "end": end, "strand": np.zeros(50, np.uint8), "label": lab, "prob": p, "n_class": 4,
              "calibrated": False, "aligned": True})
        with pytest.raises(ValueError, match=message):
            sink.close()


def test_host_sink_equals_the_twin_and_writes_the_reference_s_files(twin, tmp_path):
    """Host shards go through the twin; chromosomes are ordered by name at close(), as in the table a run writes."""
    from mural_amd.predict import SummarySink
    c = D.case("snv")
    sink = SummarySink(tmp_path / "h", motifs=(3, 5), genome=lambda name: D.SEQS[name])
    for chrom, (prob, start, end, label) in c["rows"].items():
        for part in (slice(0, 100), slice(100, None)):
            sink({"chrom": chrom, "start": start[part], "end": end[part], "strand": np.zeros(len(start[part]), np.uint8),
                  "label": label[part], "prob": prob[part], "n_class": 4, "calibrated": False, "aligned": True})
    sink.close()
    for m in (3, 5):
        names, table = sink.result()["motifs"][m]
        assert np.array_equal(sink.motif_sums()[m][0], twin["snv"][m][0])          # the tables do not depend on the order ...
        want = D.golden("snv", m)
        assert sorted(min(n, D.revcomp(n)) for n in names) == sorted(min(n, D.revcomp(n)) for n in want[0])
        assert names != want[0]                    # ... the names and their order do: chr10s leads here, chrM2 in the recorded table
        assert table[:, 0].sum() == want[3][:, -1].sum()
        assert [ln.split("\t")[0] for ln in open(tmp_path / f"h.{m}-motif.mut_rates.tsv")][1:] == names
