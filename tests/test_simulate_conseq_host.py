"""The simulated null of the consequence table on the host: the numpy twin ``simulate_conseq_host`` against its defining identity
(``summary_conseq_host`` run with the labels ``simulate_rows_host`` draws), known answers that do not depend on Philox (the 64 codons
with p_c = 1), the simulation's row checks, invariance under any split of the rows, the sink's host route with its file, the
command-line refusals and the draw kernel's resource report."""
import io
import os
import re
import subprocess
import sys

import numpy as np
import pytest

from tests import _conseq_data as D

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KEY, SEED = 0x1234ABCD, (7 << 40) + 11


def _tables():
    from mural_amd import tables
    return tables


def _twin(seq, segments, n_tx, prob, start, strand, n_rep, **kw):
    from mural_amd.summaries import simulate_conseq_host
    return simulate_conseq_host(seq, prob, start, strand, segments, n_tx, kw.pop("key", KEY), kw.pop("seed", SEED), n_rep, **kw)


@pytest.fixture(scope="module")
def record(tmp_path_factory):
    seq, text, names = D.build()
    path = tmp_path_factory.mktemp("tx") / "tx.bed"
    path.write_text(text)
    _, meta, segments = _tables().read_transcripts(str(path))
    return dict(seq=seq, text=text, names=names, meta=meta, segments=segments, path=path)


# ---- 1. the defining identity ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_the_defining_identity_on_the_record(record, dtype):
    from mural_amd.summaries import simulate_rows_host, summary_conseq_host
    prob, start, strand, _ = D.rows(record["seq"], seed=3, dtype=dtype)
    n_tx, R = len(record["names"]), 5
    table, status = _twin(record["seq"], record["segments"]["chr1"], n_tx, prob, start, strand, R)
    assert status == 0 and table.shape == (n_tx, 5, R) and table.dtype == np.uint32 and table.any()
    labels = simulate_rows_host(prob, start, strand, 4, KEY, SEED, np.arange(R))
    for r in range(R):
        want, counters, st = summary_conseq_host(record["seq"], prob, start, strand, labels[:, r].astype(np.int64), record["segments"]["chr1"], n_tx)
        assert st == 0
        assert (table[:, :, r] == want[:, :, 0]).all(), r
        # per transcript: the five bins hold the CDS rows whose draw is not 0
        assert (table[:, :, r].sum(axis=1) == counters[:, 0] - counters[:, 1]).all(), r


# ---- 2. known answers that do not depend on Philox ---------------------------------------------------------------------------------------
def _codons(strand, sizes, p_row, n_rep=3):
    rng = np.random.default_rng(1)
    body = D.ALL_CODONS if strand == "+" else D.revcomp(D.ALL_CODONS)
    piece, blocks = D._cut(body, list(sizes), rng, 5)
    seq = "ACGTA" + piece + "TTGCA"
    _, meta, segments = _tables().read_transcripts(io.StringIO(D.bed12("chr1", "t", strand, blocks) + "\n"))
    start = np.array([q for a, b in blocks for q in range(a, b)], np.int64)
    prob = np.tile(np.asarray(p_row, np.float64), (len(start), 1))
    table, status = _twin(seq, segments["chr1"], 1, prob, start, None, n_rep, aa=meta["aa"])
    assert status == 0
    return table[0]


@pytest.mark.parametrize("strand", ["+", "-"])
@pytest.mark.parametrize("sizes", [(), (1, 1, 2, 3, 1, 1, 1, 4, 2, 1, 5, 1, 1, 2, 7, 1, 1, 1, 1, 3, 2, 2, 1, 1, 9, 1, 40)])
def test_the_64_codons_with_a_certain_class(strand, sizes):
    total = np.zeros(5, np.int64)
    for c in (1, 2, 3):
        p = [0.0] * 4
        p[c] = 1.0
        cell = _codons(strand, sizes, p)
        assert (cell == cell[:, :1]).all()            # every replicate is identical
        assert cell[:, 0].sum() == 192                # every row mutates, to class c
        total += cell[:, 0]
    assert total.tolist() == [138, 392, 23, 23, 0]    # the figures of the consequence table's known-answer test
    assert not _codons(strand, sizes, [1.0, 0.0, 0.0, 0.0]).any()


# ---- 3. bad rows and the status ----------------------------------------------------------------------------------------------------------
def _five_rows(record):
    seg = record["segments"]["chr1"]
    start = np.arange(10, 15, dtype=np.int64)           # inside codons_plus
    prob = np.tile(np.array([0.0, 1.0, 0.0, 0.0]), (5, 1))
    return seg, start, prob


@pytest.mark.parametrize("bad", [np.nan, -0.25, np.inf])
def test_a_bad_probability_draws_class_0_and_sets_8(record, bad):
    seg, start, prob = _five_rows(record)
    clean, status = _twin(record["seq"], seg, len(record["names"]), prob, start, None, 4)
    assert status == 0 and clean[0].sum() == 5 * 4
    prob[2, 3] = bad                                    # another class of the row: the whole row draws 0
    table, status = _twin(record["seq"], seg, len(record["names"]), prob, start, None, 4)
    assert status == 8 and table[0].sum() == 4 * 4
    keep = np.array([0, 1, 3, 4])
    assert (table == _twin(record["seq"], seg, len(record["names"]), prob[keep], start[keep], None, 4)[0]).all()


def test_a_negative_start_sets_1_and_a_descending_pair_sets_4(record):
    seg, start, prob = _five_rows(record)
    n_tx = len(record["names"])
    table, status = _twin(record["seq"], seg, n_tx, np.concatenate([prob[:1], prob]), np.concatenate([[-3], start]), None, 2)
    assert status == 1 and (table == _twin(record["seq"], seg, n_tx, prob, start, None, 2)[0]).all()
    _, status = _twin(record["seq"], seg, n_tx, prob, start[::-1].copy(), None, 2)
    assert status == 4


def test_a_probability_above_one_is_clamped_not_refused(record):
    seg, start, prob = _five_rows(record)
    n_tx = len(record["names"])
    want, _ = _twin(record["seq"], seg, n_tx, prob, start, None, 6)
    prob[:, 1] = 1.5
    table, status = _twin(record["seq"], seg, n_tx, prob, start, None, 6)
    assert status == 0 and (table == want).all() and table[0].sum() == 5 * 6


# ---- 4. invariance and accumulation ------------------------------------------------------------------------------------------------------
def test_any_split_and_any_order_of_the_parts_gives_the_one_call_table(record):
    prob, start, strand, _ = D.rows(record["seq"], seed=4, dtype=np.float32)
    n_tx = len(record["names"])
    want, _ = _twin(record["seq"], record["segments"]["chr1"], n_tx, prob, start, strand, 6)
    rng = np.random.default_rng(0)
    for n_parts in (2, 5):
        cuts = np.sort(rng.integers(0, len(start), size=n_parts - 1))
        parts = np.split(np.arange(len(start)), cuts)
        into = np.zeros_like(want)
        for j in rng.permutation(len(parts)):
            p = parts[j]
            _, status = _twin(record["seq"], record["segments"]["chr1"], n_tx, prob[p], start[p], strand[p], 6, into=into)
            assert status == 0
        assert into.tobytes() == want.tobytes()


def test_two_rows_with_equal_start_and_strand_tie(record):
    seg = record["segments"]["chr1"]
    n_tx = len(record["names"])
    prob = np.tile(np.array([0.4, 0.2, 0.2, 0.2]), (2, 1))
    start = np.array([30, 30], np.int64)
    for strand in ([0, 0], [1, 1]):
        two, _ = _twin(record["seq"], seg, n_tx, prob, start, np.array(strand, np.uint8), 64)
        one, _ = _twin(record["seq"], seg, n_tx, prob[:1], start[:1], np.array(strand[:1], np.uint8), 64)
        assert (two == 2 * one).all() and one.any()


# ---- 5. the sink's host route ------------------------------------------------------------------------------------------------------------
def _feed(sink, prob, start, strand, label, n_parts):
    for part in np.array_split(np.arange(len(start)), n_parts):
        sink({"chrom": "chr1", "start": start[part], "end": start[part] + 1, "strand": strand[part], "label": label[part].astype(np.float32),
              "prob": prob[part], "n_class": 4, "calibrated": False, "aligned": True})
    sink.close()


def test_sink_on_host_shards_and_the_file(record, tmp_path):
    from mural_amd.predict import SummarySink
    from mural_amd.summaries import simulate_chrom_key, simulate_pvalues
    prob, start, strand, label = D.rows(record["seq"], seed=6, dtype=np.float32)
    n_tx, R = len(record["names"]), 9
    want, _ = _twin(record["seq"], record["segments"]["chr1"], n_tx, prob, start, strand, R, key=simulate_chrom_key("chr1"), seed=5)
    kw = dict(transcripts=str(record["path"]), genome=lambda name: record["seq"], simulate=R, simulate_seed=5, simulate_transcripts=True)
    for n_parts in (1, 2, 7):
        sink = SummarySink(str(tmp_path / f"p{n_parts}"), **kw)
        _feed(sink, prob, start, strand, label, n_parts)
        assert sink.consequence_simulation_counts().tobytes() == want.tobytes()
    names, counts, observed, expected = sink.result()["consequence_simulation"]
    conseq = sink.result()["consequences"][2]
    assert names == record["names"] and (observed == conseq[:, 4:11:2]).all() and (expected == conseq[:, 3:11:2]).all()
    lines = (tmp_path / "p7.consequence.sim.tsv").read_text().splitlines()
    assert lines[0].split("\t") == ["name", "consequence", "observed", "expected", "sim_mean", "sim_min", "sim_max", "n_ge", "n_le", "p_upper",
                                    "p_lower"]
    assert len(lines) == 1 + 4 * n_tx                                       # bin 4 gets no line
    assert [ln.split("\t")[:2] for ln in lines[1:5]] == [[record["names"][0], what] for what in _tables().CONSEQUENCES]
    t = record["names"].index("codons_cut_minus")
    for b in range(4):
        row = lines[1 + 4 * t + b].split("\t")
        sim = want[t, b].astype(np.int64)
        obs = int(conseq[t, 4 + 2 * b])
        n_ge, n_le = int((sim >= obs).sum()), int((sim <= obs).sum())
        assert (int(row[2]), int(row[5]), int(row[6]), int(row[7]), int(row[8])) == (obs, sim.min(), sim.max(), n_ge, n_le)
        assert float(row[3]) == pytest.approx(conseq[t, 3 + 2 * b], rel=1e-5) and float(row[4]) == pytest.approx(sim.mean(), rel=1e-5)
        assert float(row[9]) == pytest.approx((n_ge + 1) / (R + 1), rel=1e-5) and float(row[10]) == pytest.approx((n_le + 1) / (R + 1), rel=1e-5)
        assert simulate_pvalues(want[t, b:b + 1], [obs])[0][3:5] == (n_ge, n_le)
    sink = SummarySink(str(tmp_path / "na"), transcript_labels=False, **kw)
    _feed(sink, prob, start, strand, label, 2)
    assert sink.result()["consequence_simulation"][2] is None
    row = (tmp_path / "na.consequence.sim.tsv").read_text().splitlines()[1 + 4 * t].split("\t")
    assert row[2] == "NA" and row[7:] == ["NA"] * 4 and row[4] != "NA"


def test_sink_refusals_and_the_opt_in(record, tmp_path):
    from mural_amd.predict import SummarySink
    prob, start, strand, label = D.rows(record["seq"], seed=6, dtype=np.float32)
    n_tx = len(record["names"])
    kw = dict(transcripts=str(record["path"]), genome=lambda name: record["seq"], simulate=8, simulate_seed=1)
    with pytest.raises(ValueError, match="simulate_table_bytes_max"):
        SummarySink(None, simulate_transcripts=True, simulate_table_bytes_max=n_tx * 5 * 8 * 4 - 1, **kw)
    SummarySink(None, simulate_transcripts=True, simulate_table_bytes_max=n_tx * 5 * 8 * 4, **kw)
    with pytest.raises(ValueError, match="transcripts"):
        SummarySink(None, simulate=8, simulate_seed=1, simulate_transcripts=True)
    with pytest.raises(ValueError, match="simulate"):
        SummarySink(None, transcripts=str(record["path"]), genome=lambda name: record["seq"], simulate_transcripts=True)
    with pytest.raises(ValueError, match="annotations"):      # without the flag simulate= still needs its own consumer
        SummarySink(None, **kw)
    # the three-way call that is legal today starts no new table and no new file
    sink = SummarySink(str(tmp_path / "three"), annotations={"chr1": [(0, 500, "first")]}, **kw)
    _feed(sink, prob, start, strand, label, 2)
    assert "consequence_simulation" not in sink.result() and not (tmp_path / "three.consequence.sim.tsv").exists()
    assert sorted(p.name for p in tmp_path.iterdir()) == ["three.annotation.corr.txt", "three.annotation.mut_rates.tsv", "three.annotation.sim.tsv",
                                                          "three.consequence.mut_rates.tsv"]


# ---- 6. the command line -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("argv, what", [
    (["--summary", "P", "--simulate", "5", "--seed", "3"], "--annotations BED"),
    (["--summary", "P", "--simulate", "5", "--seed", "3", "--simulate_consequences"], "--simulate_consequences needs --transcripts"),
    (["--summary", "P", "--transcripts", "T", "--simulate_consequences"], "--simulate_consequences needs --simulate"),
    (["--summary", "P", "--transcripts", "T", "--simulate", "5", "--simulate_consequences"], "--simulate needs --seed"),
    (["--summary", "P", "--transcripts", "T", "--simulate", "5", "--seed", "3", "--simulate_consequences", "--model_set", "a", "0=m"],
     "--simulate does not go with --model_set"),
])
def test_command_line_refusals_are_one_line(argv, what, tmp_path):
    (tmp_path / "tx.bed").write_text(D.bed12("chr1", "t", "+", [(0, 30)]) + "\n")      # the options are checked with the file read
    argv = [str(tmp_path / "tx.bed") if a == "T" else a for a in argv]
    done = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "predict_files.py"), "m", "f", "b", "o"] + argv, capture_output=True,
                          text=True, cwd=ROOT)
    assert done.returncode != 0
    message = done.stderr.strip().splitlines()
    assert len(message) == 1 and what in message[0], done.stderr


# ---- 7. the draw kernel's resources ------------------------------------------------------------------------------------------------------
def test_the_draw_kernel_does_not_spill():
    path = os.path.join(ROOT, "mural_amd", "csrc", "simulate_conseq.resources.txt")
    if not os.path.exists(path):
        pytest.skip("no resource report: the library was not built from this tree")
    text = open(path).read()
    blocks = re.split(r"remark: Function Name: ", text)[1:]
    draw = [b for b in blocks if "simulate_conseq_draw_kernel" in b.splitlines()[0]]
    assert len(draw) == 2                                   # float and double
    for b in draw:
        assert int(re.search(r"ScratchSize \[bytes/lane\]: (\d+)", b).group(1)) == 0, b
