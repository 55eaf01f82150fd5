"""The simulated null of the structure table on the host: the numpy twin ``simulate_txstruct_host`` against its three defining
identities -- (a) ``summary_txstruct_host`` run with the labels ``simulate_rows_host`` draws, (b) bins 7 + 8 against
``simulate_conseq_host``, (c) the LoF sum against the structure file's observed_lof --, known answers that do not depend on Philox (the
toy transcript of the structure table with p_1 = 1), the simulation's row checks, invariance under any split of the rows, the sink's host
route with its file, every refusal of the flag combinations, the command-line refusals and the draw kernel's resource report."""
import io
import os
import re
import subprocess
import sys

import numpy as np
import pytest

from tests import _conseq_data as D
from tests import _txstruct_data as S

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KEY, SEED = 0x1234ABCD, (7 << 40) + 11
OTHER = dict(aa=D.CODE.replace("W", "*").replace("M", "I"), alt_order="TGC,TGA,TCA,GCA")


def _tables():
    from mural_amd import tables
    return tables


def _twin(rec, prob, start, strand, n_rep, **kw):
    from mural_amd.summaries import simulate_txstruct_host
    return simulate_txstruct_host(rec["seq"], prob, start, strand, rec["segments"], rec["features"], rec["n_tx"], kw.pop("key", KEY),
                                  kw.pop("seed", SEED), n_rep, **kw)


def _conseq_twin(rec, prob, start, strand, n_rep, **kw):
    from mural_amd.summaries import simulate_conseq_host
    return simulate_conseq_host(rec["seq"], prob, start, strand, rec["segments"], rec["n_tx"], kw.pop("key", KEY), kw.pop("seed", SEED), n_rep,
                                **kw)


@pytest.fixture(scope="module")
def record(tmp_path_factory):
    seq, text, names = S.build()
    path = tmp_path_factory.mktemp("tx") / "tx.bed"
    path.write_text(text)
    tx = _tables().read_transcript_structure(str(path))
    return dict(seq=seq, text=text, names=names, meta=tx[1], tx=tx, segments=tx[2]["chr1"], features=tx[3]["chr1"], n_tx=len(names), path=path)


# ---- 1. the defining identities ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype,stranded,kw", [(np.float32, True, {}), (np.float64, False, {}), (np.float64, True, OTHER), (np.float32, False, OTHER)])
def test_the_three_identities_on_the_record(record, dtype, stranded, kw):
    from mural_amd.summaries import simulate_lof_counts, simulate_rows_host, summary_conseq_host, summary_txstruct_host
    prob, start, strand, _ = S.rows(record["seq"], seed=3, dtype=dtype)
    strand = strand if stranded else None
    n_tx, R = record["n_tx"], 5
    table, status = _twin(record, prob, start, strand, R, **kw)
    assert status == 0 and table.shape == (n_tx, 9, R) and table.dtype == np.uint32 and table.any()
    conseq, status = _conseq_twin(record, prob, start, strand, R, **kw)
    assert status == 0
    # (b) bins 7 + 8 are the five consequence bins, per transcript and replicate
    assert (table[:, 7].astype(np.int64) + table[:, 8] == conseq.astype(np.int64).sum(axis=1)).all()
    lof = simulate_lof_counts(conseq, table)
    assert lof.shape == (n_tx, R)
    labels = simulate_rows_host(prob, start, strand, 4, KEY, SEED, np.arange(R))
    for r in range(R):
        lab = labels[:, r].astype(np.int64)
        want, counters, st = summary_txstruct_host(record["seq"], prob, start, strand, lab, record["segments"], record["features"], n_tx, **kw)
        assert st == 0
        assert (table[:, :, r] == want[:, :, 0]).all(), r                                 # (a)
        assert (table[:, :, r].sum(axis=1) == counters[:, 0] - counters[:, 1]).all(), r   # the nine bins hold the span's rows whose draw is not 0
        stop_gained = summary_conseq_host(record["seq"], prob, start, strand, lab, record["segments"], n_tx, **kw)[0][:, 2]
        observed = _tables().structure_cells_from_sums(want, stop_gained)[1]
        assert (lof[:, r] == observed[:, 9]).all(), r                                     # (c) the structure file's observed_lof
        assert (table[:, :, r] == observed[:, :9]).all(), r


def test_simulate_lof_counts():
    from mural_amd.summaries import simulate_lof_counts
    rng = np.random.default_rng(0)
    conseq, struct = rng.integers(0, 1 << 32, size=(4, 5, 6), dtype=np.uint32), rng.integers(0, 1 << 32, size=(4, 9, 6), dtype=np.uint32)
    lof = simulate_lof_counts(conseq, struct)
    assert lof.dtype == np.int64 and lof.shape == (4, 6)
    for t in range(4):
        for r in range(6):
            assert int(lof[t, r]) == int(conseq[t, 2, r]) + int(struct[t, 3, r]) + int(struct[t, 4, r]) + int(struct[t, 7, r])
    for bad in ((conseq[:, :4], struct), (conseq, struct[:, :, :5]), (conseq[:3], struct), (conseq[0], struct[0])):
        with pytest.raises(ValueError, match="simulate_lof_counts"):
            simulate_lof_counts(*bad)


# ---- 2. known answers that do not depend on Philox ---------------------------------------------------------------------------------------
def _toy(strand):
    """The toy transcript of the structure table: blocks [10,20) [30,40) [50,60), thick [15,55); codon 0 is ATG on the transcript's
    strand, every other base a G: the counts below need only codon 0."""
    seq = ["G"] * 70
    if strand == "+":
        seq[15:18] = "ATG"
    else:
        seq[52:55] = "CAT"
    seq = "".join(seq)
    tx = _tables().read_transcript_structure(io.StringIO(D.bed12("chr1", "toy", strand, [(10, 20), (30, 40), (50, 60)], (15, 55)) + "\n"))
    return dict(seq=seq, segments=tx[2]["chr1"], features=tx[3]["chr1"], n_tx=1)


@pytest.mark.parametrize("strand", ["+", "-"])
def test_the_toy_transcript_with_a_certain_class(strand):
    rec = _toy(strand)
    start = np.arange(0, 70, dtype=np.int64)
    for c in (1, 2, 3):
        prob = np.zeros((70, 4))
        prob[:, c] = 1.0
        table, status = _twin(rec, prob, start, None, 7)
        assert status == 0 and (table == table[:, :, :1]).all()            # every replicate is identical
        cell = table[0, :, 0].tolist()
        # 5 + 5 UTR bases, no non-coding exon, two coding introns of 10 bases: 2 + 2 donor, 2 + 2 acceptor, 6 + 6 between; of the 20 CDS
        # bases the three of ATG change the amino acid whatever the class (M has one codon): 3 start lost, 17 cds
        assert cell == [5, 5, 0, 4, 4, 0, 12, 3, 17], (strand, c)
    # which end is the donor: a row at the first base of the first gap alone
    prob = np.zeros((1, 4))
    prob[:, 1] = 1.0
    first, _ = _twin(rec, prob, np.array([20], np.int64), None, 2)
    last, _ = _twin(rec, prob, np.array([29], np.int64), None, 2)
    donor, acceptor = (3, 4) if strand == "+" else (4, 3)
    assert first[0, donor].tolist() == [1, 1] and last[0, acceptor].tolist() == [1, 1] and first.sum() == last.sum() == 2
    # the 5' UTR is the low end on '+', the high end on '-'
    low, _ = _twin(rec, prob, np.array([12], np.int64), None, 1)
    assert low[0, 0 if strand == "+" else 1, 0] == 1
    # class 0 counts nowhere, and rows outside the span count nowhere
    prob = np.zeros((70, 4))
    prob[:, 0] = 1.0
    assert not _twin(rec, prob, start, None, 3)[0].any()
    prob[:, 1] = 1.0
    outside = np.concatenate([np.arange(0, 10), np.arange(60, 70)]).astype(np.int64)
    assert not _twin(rec, prob[:20], outside, None, 3)[0].any()


def test_gaps_of_three_and_four_bases():
    tx = _tables().read_transcript_structure(io.StringIO(D.bed12("chr1", "t", "+", [(10, 16), (19, 25), (29, 35)]) + "\n"))
    rec = dict(seq="ACGT" * 10, segments=tx[2]["chr1"], features=tx[3]["chr1"], n_tx=1)
    prob = np.zeros((7, 4))
    prob[:, 2] = 1.0
    table, _ = _twin(rec, prob[:3], np.arange(16, 19).astype(np.int64), None, 1)
    assert table[0, :, 0].tolist() == [0, 0, 0, 0, 0, 0, 3, 0, 0]           # a gap of 3: no splice sites
    table, _ = _twin(rec, prob[:4], np.arange(25, 29).astype(np.int64), None, 1)
    assert table[0, :, 0].tolist() == [0, 0, 0, 2, 2, 0, 0, 0, 0]           # a gap of 4: donor and acceptor and nothing between


# ---- 3. every bin is reached at 129 replicates -------------------------------------------------------------------------------------------
def test_every_bin_and_lof_is_reached_at_129_replicates(record):
    from mural_amd.summaries import simulate_lof_counts
    prob, start, strand, _ = S.rows(record["seq"], seed=1, dtype=np.float32)
    table, status = _twin(record, prob, start, strand, 129)
    conseq, _ = _conseq_twin(record, prob, start, strand, 129)
    assert status == 0 and (table.sum(axis=(0, 2)) > 0).all() and simulate_lof_counts(conseq, table).any()
    # replicate r does not depend on the replicate count
    few, _ = _twin(record, prob, start, strand, 5)
    assert few.tobytes() == np.ascontiguousarray(table[:, :, :5]).tobytes()
    assert record["n_tx"] > 60 and len(record["features"]["feat_b0"]) > 600 and len(start) > 3000


# ---- 4. bad rows and the status ----------------------------------------------------------------------------------------------------------
def _five_rows():
    rec = _toy("+")
    start = np.arange(18, 23, dtype=np.int64)           # two CDS bases, three of the first intron
    prob = np.tile(np.array([0.0, 1.0, 0.0, 0.0]), (5, 1))
    return rec, start, prob


@pytest.mark.parametrize("bad", [np.nan, -0.25, np.inf])
def test_a_bad_probability_draws_class_0_and_sets_8(bad):
    rec, start, prob = _five_rows()
    clean, status = _twin(rec, prob, start, None, 4)
    assert status == 0 and clean[0].sum() == 5 * 4
    prob[2, 3] = bad                                    # another class of the row: the whole row draws 0
    table, status = _twin(rec, prob, start, None, 4)
    assert status == 8 and table[0].sum() == 4 * 4
    keep = np.array([0, 1, 3, 4])
    assert (table == _twin(rec, prob[keep], start[keep], None, 4)[0]).all()


def test_a_negative_start_sets_1_a_descending_pair_4_and_above_one_is_clamped():
    rec, start, prob = _five_rows()
    table, status = _twin(rec, np.concatenate([prob[:1], prob]), np.concatenate([[-3], start]), None, 2)
    assert status == 1 and (table == _twin(rec, prob, start, None, 2)[0]).all()
    assert _twin(rec, prob, start[::-1].copy(), None, 2)[1] == 4
    want, _ = _twin(rec, prob, start, None, 6)
    prob[:, 1] = 1.5
    table, status = _twin(rec, prob, start, None, 6)
    assert status == 0 and (table == want).all() and table[0].sum() == 5 * 6


# ---- 5. invariance and accumulation ------------------------------------------------------------------------------------------------------
def test_any_split_and_any_order_of_the_parts_gives_the_one_call_table(record):
    prob, start, strand, _ = S.rows(record["seq"], seed=4, dtype=np.float32)
    want, _ = _twin(record, prob, start, strand, 6)
    rng = np.random.default_rng(0)
    for n_parts in (2, 5):
        cuts = np.sort(rng.integers(0, len(start), size=n_parts - 1))
        parts = np.split(np.arange(len(start)), cuts)
        into = np.zeros_like(want)
        for j in rng.permutation(len(parts)):
            p = parts[j]
            _, status = _twin(record, prob[p], start[p], strand[p], 6, into=into)
            assert status == 0
        assert into.tobytes() == want.tobytes()


# ---- 6. the sink's host route ------------------------------------------------------------------------------------------------------------
def _feed(sink, prob, start, strand, label, n_parts):
    for part in np.array_split(np.arange(len(start)), n_parts):
        sink({"chrom": "chr1", "start": start[part], "end": start[part] + 1, "strand": strand[part], "label": label[part].astype(np.float32),
              "prob": prob[part], "n_class": 4, "calibrated": False, "aligned": True})
    sink.close()


def _sink_kw(record, R=9, seed=5):
    return dict(transcripts=str(record["path"]), genome=lambda name: record["seq"], simulate=R, simulate_seed=seed, simulate_transcripts=True,
                transcript_structure=True, simulate_structure=True)


def test_sink_on_host_shards_and_the_file(record, tmp_path):
    from mural_amd.predict import SummarySink
    from mural_amd.summaries import simulate_chrom_key, simulate_lof_counts
    prob, start, strand, label = S.rows(record["seq"], seed=6, dtype=np.float32)
    n_tx, R = record["n_tx"], 9
    key = simulate_chrom_key("chr1")
    want, _ = _twin(record, prob, start, strand, R, key=key, seed=5)
    want_lof = simulate_lof_counts(_conseq_twin(record, prob, start, strand, R, key=key, seed=5)[0], want)
    kw = _sink_kw(record)
    for n_parts in (1, 2, 7):
        sink = SummarySink(str(tmp_path / f"p{n_parts}"), **kw)
        _feed(sink, prob, start, strand, label, n_parts)
        assert sink.structure_simulation_counts().tobytes() == want.tobytes()
    names, counts, lof, observed, expected = sink.result()["structure_simulation"]
    assert names == record["names"] and counts.tobytes() == want.tobytes() and np.array_equal(lof, want_lof)
    assert observed.shape == expected.shape == (n_tx, 10)
    structure = [ln.split("\t") for ln in (tmp_path / "p7.consequence.structure.tsv").read_text().splitlines()]
    lines = [ln.split("\t") for ln in (tmp_path / "p7.consequence.structure.sim.tsv").read_text().splitlines()]
    assert lines[0] == ["name", "bin", "observed", "expected", "sim_mean", "sim_min", "sim_max", "n_ge", "n_le", "p_upper", "p_lower"]
    whats = list(_tables().STRUCTURE_BINS) + ["lof"]
    assert len(lines) == 1 + 10 * n_tx and [ln[:2] for ln in lines[1:11]] == [[record["names"][0], what] for what in whats]
    t = record["names"].index("known_m")
    for b, what in enumerate(whats):
        row = lines[1 + 10 * t + b]
        sim = (want[t, b] if b < 9 else want_lof[t]).astype(np.int64)
        # observed and expected are the structure file's own text
        assert row[3] == structure[1 + t][structure[0].index(f"expected_{what}")] and row[2] == structure[1 + t][structure[0].index(f"observed_{what}")]
        obs = int(row[2])
        n_ge, n_le = int((sim >= obs).sum()), int((sim <= obs).sum())
        assert (int(row[5]), int(row[6]), int(row[7]), int(row[8])) == (sim.min(), sim.max(), n_ge, n_le)
        assert float(row[4]) == pytest.approx(sim.mean(), rel=1e-5)
        assert float(row[9]) == pytest.approx((n_ge + 1) / (R + 1), rel=1e-5) and float(row[10]) == pytest.approx((n_le + 1) / (R + 1), rel=1e-5)
    # the files the run wrote before the flag existed are the same bytes with it
    plain = SummarySink(str(tmp_path / "plain"), **dict(kw, simulate_structure=False))
    _feed(plain, prob, start, strand, label, 2)
    for tail in ("consequence.mut_rates.tsv", "consequence.sim.tsv", "consequence.structure.tsv"):
        assert (tmp_path / f"plain.{tail}").read_bytes() == (tmp_path / f"p2.{tail}").read_bytes()
    assert not (tmp_path / "plain.consequence.structure.sim.tsv").exists() and "structure_simulation" not in plain.result()
    sink = SummarySink(str(tmp_path / "na"), transcript_labels=False, **kw)
    _feed(sink, prob, start, strand, label, 2)
    assert sink.result()["structure_simulation"][3] is None
    row = (tmp_path / "na.consequence.structure.sim.tsv").read_text().splitlines()[1 + 10 * t + 9].split("\t")
    assert row[2] == "NA" and row[7:] == ["NA"] * 4 and row[3] != "NA" and row[4] != "NA"


def test_the_writer_alone(tmp_path):
    tables = _tables()
    counts = np.zeros((1, 9, 4), np.uint32)
    counts[0, 3] = [0, 1, 2, 3]
    lof = np.array([[5, 5, 6, 7]])
    expected, observed = np.arange(10, dtype=np.float64)[None] / 4, np.arange(10)[None]
    path = tables.write_structure_simulation_outputs(["g"], counts, lof, observed, expected, str(tmp_path / "w"))
    assert path == tables.structure_simulation_output_name(str(tmp_path / "w")) == str(tmp_path / "w.consequence.structure.sim.tsv")
    rows = [ln.split("\t") for ln in open(path).read().splitlines()]
    assert rows[4] == ["g", "splice_donor", "3", "0.75", "1.5", "0", "3", "1", "4", "0.4", "1.0"]
    assert rows[10] == ["g", "lof", "9", "2.25", "5.75", "5", "7", "0", "4", "0.2", "1.0"]
    tables.write_structure_simulation_outputs(["g"], counts, lof, None, expected, str(tmp_path / "w"))
    rows = [ln.split("\t") for ln in open(path).read().splitlines()]
    assert rows[10] == ["g", "lof", "NA", "2.25", "5.75", "5", "7", "NA", "NA", "NA", "NA"]


def test_sink_refusals_and_the_opt_in(record):
    from mural_amd.predict import SummarySink
    n_tx = record["n_tx"]
    kw = _sink_kw(record, R=8, seed=1)
    with pytest.raises(ValueError, match="9 structure bins.*simulate_table_bytes_max"):
        SummarySink(None, simulate_table_bytes_max=n_tx * 9 * 8 * 4 - 1, **kw)
    SummarySink(None, simulate_table_bytes_max=n_tx * 9 * 8 * 4, **kw)
    without = lambda *keys: {k: v for k, v in kw.items() if k not in keys}      # noqa: E731
    with pytest.raises(ValueError, match="simulate_structure needs simulate=R with simulate_seed"):
        SummarySink(None, **without("simulate", "simulate_seed", "simulate_transcripts"))
    with pytest.raises(ValueError, match="simulate_structure needs transcript_structure=True"):
        SummarySink(None, **without("transcript_structure"))
    with pytest.raises(ValueError, match="simulate_structure needs simulate_transcripts=True"):
        SummarySink(None, **without("simulate_transcripts"))
    with pytest.raises(ValueError, match="simulate_structure needs transcript_structure=True.*simulate_transcripts=True"):
        SummarySink(None, **without("transcripts", "genome", "transcript_structure", "simulate_transcripts"), annotations={"chr1": [(0, 5, "a")]})
    with pytest.raises(ValueError, match="simulate_structure needs simulate=R.*transcript_structure=True.*simulate_transcripts=True"):
        SummarySink(None, simulate_structure=True)
    with pytest.raises(ValueError, match="simulate_seed"):      # simulate=R alone is refused as before
        SummarySink(None, **without("simulate_seed"))


# ---- 7. the command line -----------------------------------------------------------------------------------------------------------------
_ALL = ["--summary", "P", "--transcripts", "T", "--transcript_structure", "--simulate", "5", "--seed", "3", "--simulate_consequences",
        "--simulate_structure"]


def _drop(*names):
    out, skip = [], 0
    for a in _ALL:
        if skip:
            skip -= 1
        elif a in names:
            skip = 1 if a in ("--transcripts", "--simulate", "--seed") else 0
        else:
            out.append(a)
    return out


@pytest.mark.parametrize("argv, what", [
    (_drop("--transcripts", "--transcript_structure"), "--simulate_structure needs --transcripts"),
    (_drop("--transcript_structure"), "--simulate_structure needs --transcript_structure"),
    (_drop("--simulate", "--seed"), "--simulate_structure needs --simulate R --seed S"),
    (_drop("--simulate_consequences"), "--simulate_structure needs --simulate_consequences"),
    (_drop("--seed"), "--simulate needs --seed"),
    (_ALL + ["--indel"], "--simulate_structure takes SNV rows: it does not go with --indel"),
])
def test_command_line_refusals_are_one_line(argv, what, tmp_path):
    (tmp_path / "tx.bed").write_text(D.bed12("chr1", "t", "+", [(0, 30)]) + "\n")      # the options are checked with the file read
    argv = [str(tmp_path / "tx.bed") if a == "T" else a for a in argv]
    done = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "predict_files.py"), "m", "f", "b", "o"] + argv, capture_output=True,
                          text=True, cwd=ROOT)
    assert done.returncode != 0
    message = done.stderr.strip().splitlines()
    assert len(message) == 1 and what in message[0], done.stderr


# ---- 8. the draw kernel's resources ------------------------------------------------------------------------------------------------------
def test_the_draw_kernel_does_not_spill():
    path = os.path.join(ROOT, "mural_amd", "csrc", "simulate_txstruct.resources.txt")
    if not os.path.exists(path):
        pytest.skip("no resource report: the library was not built from this tree")
    text = open(path).read()
    blocks = re.split(r"remark: Function Name: ", text)[1:]
    draw = [b for b in blocks if "simulate_txstruct_draw_kernel" in b.splitlines()[0]]
    assert len(draw) == 2                                   # float and double
    for b in draw:
        assert int(re.search(r"ScratchSize \[bytes/lane\]: (\d+)", b).group(1)) == 0, b
