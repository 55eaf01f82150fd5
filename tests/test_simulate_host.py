"""The specification of the simulated mutation sets (mural_amd.summaries: ``philox4x32_10``, ``simulate_rows_host``,
``simulate_annot_host``, ``simulate_pvalues``) on the host: the generator against an independent scalar implementation and the
Random123 known answers, the class rule on crafted rows, split invariance, the annotation semantics against a brute-force oracle, the
calibration of the draw, the p-value columns and the sink's host route."""
import numpy as np
import pytest

from tests import _annot_data as D

MASK = 0xFFFFFFFF


def _S():
    from mural_amd import summaries
    return summaries


# ---- an independent scalar Philox4x32-10 in plain Python integers ------------------------------------------------------------------------
def philox_scalar(counter, key):
    c, k = [int(x) for x in counter], [int(x) for x in key]
    for rnd in range(10):
        prod0, prod1 = 0xD2511F53 * c[0], 0xCD9E8D57 * c[2]
        c = [(prod1 >> 32) ^ c[1] ^ k[0], prod1 & MASK, (prod0 >> 32) ^ c[3] ^ k[1], prod0 & MASK]
        k = [(k[0] + 0x9E3779B9) & MASK, (k[1] + 0xBB67AE85) & MASK]      # (the bump after the last round is never read)
    return c


def label_scalar(prob_row, start, minus, n_class, chrom_key, seed, rep):
    """The class rule in Python integers and ``fractions``-free exact arithmetic: float.as_integer_ratio gives p exactly."""
    if any(not np.isfinite(p) or (p < 0) for p in prob_row[1:n_class]) or start < 0:
        return 0
    s = start & 0xFFFFFFFFFFFFFFFF
    u = philox_scalar((s & MASK, s >> 32, chrom_key, (rep >> 2) | (int(minus) << 31)), (seed & MASK, seed >> 32))[rep & 3]
    run = 0
    for c in range(1, n_class):
        num, den = float(prob_row[c]).as_integer_ratio()
        run += (num << 32) // den
        if u < min(run, 1 << 32):
            return c
    return 0


KNOWN = [((0, 0, 0, 0), (0, 0), (0x6627E8D5, 0xE169C58D, 0xBC57AC4C, 0x9B00DBD8)),
         ((MASK,) * 4, (MASK,) * 2, (0x408F276D, 0x41C83B0E, 0xA20BC7C6, 0x6D5451FD))]


def test_generator_equals_the_scalar_implementation_and_the_known_answers():
    S = _S()
    for ctr, key, want in KNOWN:
        assert tuple(philox_scalar(ctr, key)) == want
        assert tuple(int(x) for x in S.philox4x32_10(np.array(ctr), np.array(key))) == want
    rng = np.random.default_rng(11)
    ctr = rng.integers(0, 1 << 32, size=(300, 4), dtype=np.uint64)
    key = rng.integers(0, 1 << 32, size=(300, 2), dtype=np.uint64)
    ctr[:4] = [[0, 0, 0, 0], [MASK] * 4, [MASK, 0, MASK, 0], [0, MASK, 0, MASK]]
    got = S.philox4x32_10(ctr, key)
    assert got.dtype == np.uint32 and got.shape == (300, 4)
    assert got.tolist() == [philox_scalar(c, k) for c, k in zip(ctr.tolist(), key.tolist())]
    one_key = S.philox4x32_10(ctr, key[0])                       # a key broadcast over the counters
    assert one_key.tolist() == [philox_scalar(c, key[0].tolist()) for c in ctr.tolist()]


def _u_of(start, minus, chrom_key, seed, rep):
    s = start & 0xFFFFFFFFFFFFFFFF
    return philox_scalar((s & MASK, s >> 32, chrom_key, (rep >> 2) | (minus << 31)), (seed & MASK, seed >> 32))[rep & 3]


# ---- the class rule -----------------------------------------------------------------------------------------------------------------------
def test_cum_landing_exactly_on_u_and_on_u_plus_one():
    """u < cum is strict: with q_1 = u the row draws past class 1, with q_1 = u + 1 it draws class 1 (float64 holds u * 2^-32 exactly)."""
    S = _S()
    seed, ck = 0x123456789ABCDEF, 77
    start = np.arange(1000, 1040, dtype=np.int64)
    for rep in (0, 1, 2, 3, 4, 9):
        u = np.array([_u_of(int(s), 0, ck, seed, rep) for s in start], np.float64)
        on = np.zeros((len(start), 3))
        on[:, 1] = u / 2.0 ** 32
        above = on.copy()
        above[:, 1] = (u + 1) / 2.0 ** 32
        assert (S.simulate_rows_host(on, start, None, 3, ck, seed, [rep])[:, 0] == 0).all()
        assert (S.simulate_rows_host(above, start, None, 3, ck, seed, [rep])[:, 0] == 1).all()
        on[:, 2] = 2.0 ** -32                                   # the next class takes exactly the value u
        assert (S.simulate_rows_host(on, start, None, 3, ck, seed, [rep])[:, 0] == 2).all()


@pytest.mark.parametrize("n_class", [2, 8])
def test_labels_equal_the_scalar_rule_and_float32_equals_float64(n_class):
    S = _S()
    rng = np.random.default_rng(n_class)
    n = 120
    prob32 = (rng.dirichlet(np.ones(n_class), size=n) * rng.choice([0.05, 0.5, 1.0, 1.7], size=(n, 1))).astype(np.float32)
    prob32[:4, 1] = [0.0, 1.0, 2.0 ** -32, 2.0 ** -33]
    prob64 = prob32.astype(np.float64)                          # the same values
    start = np.sort(rng.choice(1 << 34, size=n, replace=False)).astype(np.int64)      # past 2^32: both counter words
    strand = rng.integers(0, 2, size=n).astype(np.uint8)
    seed, ck, reps = (1 << 63) + 12345, S.simulate_chrom_key("chr7"), [0, 1, 2, 3, 4, 66, (1 << 20) - 1]
    got32 = S.simulate_rows_host(prob32, start, strand, n_class, ck, seed, reps)
    got64 = S.simulate_rows_host(prob64, start, strand, n_class, ck, seed, reps)
    assert got32.dtype == np.uint8 and np.array_equal(got32, got64)
    want = [[label_scalar(prob64[i], int(start[i]), strand[i], n_class, ck, seed, r) for r in reps] for i in range(n)]
    assert got64.tolist() == want
    assert len(set(np.unique(got64))) > 1
    plus = S.simulate_rows_host(prob64, start, None, n_class, ck, seed, reps)
    assert np.array_equal(plus[strand == 0], got64[strand == 0]) and not np.array_equal(plus, got64)


def test_probabilities_summing_above_one_are_clamped():
    S = _S()
    n = 200
    start = np.arange(n, dtype=np.int64) * 3
    prob = np.tile(np.array([0.0, 0.75, 0.75, 0.75]), (n, 1))
    lab = S.simulate_rows_host(prob, start, None, 4, 5, 9, np.arange(8))
    assert set(np.unique(lab)) == {1, 2}                        # cum = 0.75, 1, 1: class 3 and class 0 are never drawn
    huge = prob.copy()
    huge[:, 1] = 1e300                                          # finite: class 1 with certainty
    assert (S.simulate_rows_host(huge, start, None, 4, 5, 9, [0, 5]) == 1).all()


def test_a_bad_row_draws_zero_and_sets_status():
    S = _S()
    n = 50
    start = np.arange(n, dtype=np.int64)
    prob = np.tile(np.array([0.0, 0.5, 0.5], np.float32), (n, 1))
    for value, where, bit in ((np.nan, 1, 8), (-0.25, 2, 8), (np.inf, 1, 8)):
        p = prob.copy()
        p[7, where] = value
        lab, status = S.simulate_rows_host(p, start, None, 3, 1, 2, np.arange(6), with_status=True)
        assert status == bit and (lab[7] == 0).all() and (np.delete(lab, 7, axis=0) > 0).all()
    p = prob.copy()
    p[7, 0] = np.nan                                            # class 0 is never read
    p[8, 1] = -0.0                                              # -0.0 is 0
    lab, status = S.simulate_rows_host(p, start, None, 3, 1, 2, np.arange(6), with_status=True)
    assert status == 0 and (lab[7] > 0).all() and set(lab[8].tolist()) == {0, 2}      # cum = 0, 0.5
    st = start.copy()
    st[0] = -1
    lab, status = S.simulate_rows_host(prob, st, None, 3, 1, 2, np.arange(6), with_status=True)
    assert status == 1 and (lab[0] == 0).all()


def test_rows_with_the_same_chromosome_start_and_strand_draw_the_same_value():
    """The documented consequence of the counter: the draw is a function of (seed, chromosome, start, strand, replicate) alone."""
    S = _S()
    prob = np.tile(np.array([0.5, 0.25, 0.25]), (4, 1))
    start = np.array([10, 10, 10, 11], np.int64)
    strand = np.array([0, 0, 1, 0], np.uint8)
    lab = S.simulate_rows_host(prob, start, strand, 3, 3, 4, np.arange(64))
    assert np.array_equal(lab[0], lab[1]) and not np.array_equal(lab[0], lab[2]) and not np.array_equal(lab[0], lab[3])
    assert not np.array_equal(lab, S.simulate_rows_host(prob, start, strand, 3, 4, 4, np.arange(64)))      # another chromosome
    assert not np.array_equal(lab, S.simulate_rows_host(prob, start, strand, 3, 3, 5, np.arange(64)))      # another seed


# ---- split invariance and the annotation semantics ---------------------------------------------------------------------------------------
def _unique_rows(n, n_class, seed, lo=100, hi=900):
    """Rows of one chromosome with distinct starts (``_annot_data.rows`` holds runs of equal starts on purpose), none in 500 .. 509."""
    rng = np.random.default_rng(seed)
    where = np.arange(lo, hi)
    start = np.sort(rng.choice(where[(where < 500) | (where >= 510)], size=n, replace=False)).astype(np.int64)
    prob = rng.dirichlet(np.ones(n_class), size=n)
    prob[:, 1:] *= 0.6
    return prob, start, rng.integers(0, 2, size=n).astype(np.uint8)


def _pieces():
    from mural_amd.tables import read_annotations
    return read_annotations(D.intervals_dict())


def test_one_call_equals_any_split_into_parts():
    S = _S()
    names, _, pieces = _pieces()
    prob, start, strand = _unique_rows(300, 4, 0)
    ck = S.simulate_chrom_key("chrA")
    whole, status = S.simulate_annot_host(prob, start, strand, 4, ck, 7, pieces["chrA"], len(names), 9)
    assert status == 0 and whole.dtype == np.uint32 and whole.shape == (len(names), 3, 9) and whole.sum() > 0
    labels = S.simulate_rows_host(prob, start, strand, 4, ck, 7, np.arange(9))
    N = len(start)
    rng = np.random.default_rng(5)
    for cuts in ([0], [1], [N - 1], [N], sorted(rng.integers(0, N + 1, size=4).tolist()), sorted(rng.integers(0, N + 1, size=9).tolist())):
        table, got_labels = None, []
        for rows in np.split(np.arange(N), cuts):
            table, _ = S.simulate_annot_host(prob[rows], start[rows], strand[rows], 4, ck, 7, pieces["chrA"], len(names), 9, into=table)
            got_labels.append(S.simulate_rows_host(prob[rows], start[rows], strand[rows], 4, ck, 7, np.arange(9)))
        assert np.array_equal(table, whole), cuts
        assert np.array_equal(np.concatenate(got_labels), labels), cuts


def brute_force(per_chrom, n_class, names, seed, n_rep):
    """[[count per replicate] per class >= 1] per name in Python integers: any(b0 <= start < b1) over the name's unmerged intervals."""
    S = _S()
    iv = D.intervals()
    out = [[[0] * n_rep for _ in range(n_class - 1)] for _ in names]
    for chrom, (prob, start, strand) in per_chrom.items():
        labels = S.simulate_rows_host(prob, start, strand, n_class, S.simulate_chrom_key(chrom), seed, np.arange(n_rep)).tolist()
        for g, name in enumerate(names):
            for i, s in enumerate(start.tolist()):
                if any(c == chrom and b0 <= s < b1 for c, b0, b1 in iv[name]):
                    for r, lab in enumerate(labels[i]):
                        if lab:
                            out[g][lab - 1][r] += 1
    return out


def per_chrom_rows():
    return {"chrA": _unique_rows(300, 4, 0), "chrB": _unique_rows(40, 4, 1, lo=0, hi=70)}


def test_table_twin_equals_the_brute_force_oracle():
    """The literal BED: nested (`inner` in `outer`), overlapping and touching (`exons`) intervals, a name on two chromosomes (`gene`,
    `outer`), names without rows (`past`, `gap`, `before`, `never`)."""
    S = _S()
    names, _, pieces = _pieces()
    assert names == D.NAMES
    table = None
    for chrom, (prob, start, strand) in per_chrom_rows().items():
        table, status = S.simulate_annot_host(prob, start, strand, 4, S.simulate_chrom_key(chrom), 7, pieces.get(chrom), len(names), 5,
                                              into=table)
        assert status == 0
    assert table.tolist() == brute_force(per_chrom_rows(), 4, names, 7, 5)
    for name in ("past", "gap", "before", "never"):
        assert not table[names.index(name)].any()
    assert 0 < table[names.index("inner")].sum() < table[names.index("outer")].sum() < table[names.index("everything")].sum()
    on_a = S.simulate_annot_host(*per_chrom_rows()["chrA"], 4, S.simulate_chrom_key("chrA"), 7, pieces["chrA"], len(names), 5)[0]
    assert table[names.index("gene")].sum() > on_a[names.index("gene")].sum() > 0      # the name's rows on chrB count too


# ---- calibration of the draw --------------------------------------------------------------------------------------------------------------
CALIBRATION_SEED = 20261020      # chosen once on the host so that the twin meets the bounds below; no retries


def test_the_draw_is_calibrated():
    """20 000 rows, p_c in [0.01, 0.1] for three classes, R = 64: every per-class total over rows x replicates within 5 standard
    deviations of sum p_c R (variance sum p (1 - p) R: the draws are independent Bernoulli), and every per-replicate total of class 1
    within 5 standard deviations of sum p_1.  The expectation uses q_c 2^-32, the probability the rule realises exactly."""
    S = _S()
    n, R = 20_000, 64
    rng = np.random.default_rng(3)
    prob = np.zeros((n, 4))
    prob[:, 1:] = rng.uniform(0.01, 0.1, size=(n, 3))
    prob[:, 0] = 1 - prob[:, 1:].sum(axis=1)
    start = np.arange(n, dtype=np.int64) * 7 + 3
    lab = S.simulate_rows_host(prob, start, None, 4, S.simulate_chrom_key("chr1"), CALIBRATION_SEED, np.arange(R))
    for c in (1, 2, 3):
        p = np.floor(prob[:, c] * 2.0 ** 32) / 2.0 ** 32
        total = int((lab == c).sum())
        sd = np.sqrt((p * (1 - p)).sum() * R)
        assert abs(total - p.sum() * R) <= 5 * sd, (c, total, p.sum() * R, sd)
    p = np.floor(prob[:, 1] * 2.0 ** 32) / 2.0 ** 32
    per_rep = (lab == 1).sum(axis=0)
    sd = np.sqrt((p * (1 - p)).sum())
    assert (np.abs(per_rep - p.sum()) <= 5 * sd).all(), (per_rep.tolist(), p.sum(), sd)
    assert len(set(per_rep.tolist())) > R // 2                  # the replicates differ


# ---- the p-value columns ------------------------------------------------------------------------------------------------------------------
def test_pvalue_columns_of_a_hand_made_table():
    S = _S()
    counts = [[0, 1, 2, 3, 4, 5, 6, 7, 8, 9], [5] * 10, [0] * 10]
    got = S.simulate_pvalues(counts, [3, 5, 1])
    assert got[0] == (4.5, 0, 9, 7, 4, 8 / 11, 5 / 11)
    assert got[1] == (5.0, 5, 5, 10, 10, 1.0, 1.0)
    assert got[2] == (0.0, 0, 0, 0, 10, 1 / 11, 1.0)
    assert S.simulate_pvalues(counts)[0] == (4.5, 0, 9, None, None, None, None)


# ---- the sink's host route ----------------------------------------------------------------------------------------------------------------
def _shards(per_chrom, parts, labels=True):
    for chrom, (prob, start, strand) in per_chrom.items():
        label = (np.arange(len(start)) % 4 * (np.arange(len(start)) % 3 == 0)).astype(np.float32)
        for rows in np.array_split(np.arange(len(start)), parts):
            yield {"chrom": chrom, "start": start[rows], "end": start[rows] + 1, "strand": strand[rows],
                   "label": label[rows] if labels else np.zeros(len(rows), np.float32), "prob": prob[rows], "n_class": 4,
                   "calibrated": False, "aligned": True}


def test_sink_arguments_are_checked():
    from mural_amd.predict import SummarySink
    with pytest.raises(ValueError, match="simulate_seed"):
        SummarySink(None, annotations=D.intervals_dict(), simulate=5)
    with pytest.raises(ValueError, match="annotations"):
        SummarySink(None, simulate=5, simulate_seed=1)
    with pytest.raises(ValueError, match="simulate_write"):
        SummarySink("p", annotations=D.intervals_dict(), simulate=5, simulate_seed=1, simulate_write=(5,))
    with pytest.raises(ValueError, match="2\\^20"):
        SummarySink(None, annotations=D.intervals_dict(), simulate=(1 << 20) + 1, simulate_seed=1)
    sink = SummarySink(None, annotations=D.intervals_dict(), simulate=1000, simulate_seed=1, simulate_table_bytes_max=12 * 3 * 1000 * 4 - 1)
    with pytest.raises(ValueError, match="simulate_table_bytes_max"):
        for shard in _shards(per_chrom_rows(), 1):
            sink(shard)


def test_host_sink_writes_the_table_and_the_mutation_list(tmp_path):
    """Host shards in 1 and in 3 parts: byte-identical files; the table's columns against the twin and ``simulate_pvalues``; the
    mutation list read back by ``read_mutations`` is replicate 1's non-zero labels."""
    from mural_amd.data import read_mutations
    from mural_amd.predict import SummarySink
    S = _S()
    texts = []
    for parts in (1, 3):
        sink = SummarySink(str(tmp_path / f"p{parts}"), annotations=D.intervals_dict(), simulate=5, simulate_seed=7, simulate_write=(1,))
        for shard in _shards(per_chrom_rows(), parts):
            sink(shard)
        sink.close()
        texts.append(((tmp_path / f"p{parts}.annotation.sim.tsv").read_text(), (tmp_path / f"p{parts}.sim1.mutations.bed").read_text()))
        assert np.array_equal(sink.simulation_counts(), np.array(brute_force(per_chrom_rows(), 4, D.NAMES, 7, 5), np.uint32))
    assert texts[0] == texts[1]
    lines = [ln.split("\t") for ln in texts[0][0].splitlines()]
    assert lines[0] == ["name", "class", "observed", "expected", "sim_mean", "sim_min", "sim_max", "n_ge", "n_le", "p_upper", "p_lower"]
    assert [(ln[0], ln[1]) for ln in lines[1:]] == [(nm, str(c)) for nm in D.NAMES for c in (1, 2, 3)]
    counts = np.array(brute_force(per_chrom_rows(), 4, D.NAMES, 7, 5))
    row = lines[1 + 3 * D.NAMES.index("outer") + 1]             # outer, class 2
    g = counts[D.NAMES.index("outer"), 1]
    observed = int(row[2])
    assert observed > 0 and float(row[4]) == g.mean() and (int(row[5]), int(row[6])) == (g.min(), g.max())
    assert (int(row[7]), int(row[8])) == ((g >= observed).sum(), (g <= observed).sum())
    assert float(row[9]) == ((g >= observed).sum() + 1) / 6 and float(row[10]) == ((g <= observed).sum() + 1) / 6
    muts = read_mutations(str(tmp_path / "p1.sim1.mutations.bed"), 4)
    for chrom, (prob, start, strand) in per_chrom_rows().items():
        lab = S.simulate_rows_host(prob, start, strand, 4, S.simulate_chrom_key(chrom), 7, [1])[:, 0]
        assert np.array_equal(muts[chrom][0], start[lab > 0]) and np.array_equal(muts[chrom][1], strand[lab > 0])
        assert np.array_equal(muts[chrom][2], lab[lab > 0].astype(np.float32))


def test_without_labels_the_observed_columns_are_NA(tmp_path):
    from mural_amd.predict import SummarySink
    sink = SummarySink(str(tmp_path / "p"), annotations=D.intervals_dict(), simulate=4, simulate_seed=7, simulate_labels=False)
    for shard in _shards(per_chrom_rows(), 2, labels=False):
        sink(shard)
    sink.close()
    lines = [ln.split("\t") for ln in (tmp_path / "p.annotation.sim.tsv").read_text().splitlines()[1:]]
    assert all(ln[2] == "NA" and ln[7:] == ["NA"] * 4 for ln in lines) and any(float(ln[4]) > 0 for ln in lines)


def test_simulate_write_alone_needs_no_annotations(tmp_path):
    from mural_amd.predict import SummarySink
    sink = SummarySink(str(tmp_path / "p"), simulate=3, simulate_seed=9, simulate_write=(0, 2))
    for shard in _shards(per_chrom_rows(), 2):
        sink(shard)
    sink.close()
    assert (tmp_path / "p.sim0.mutations.bed").exists() and (tmp_path / "p.sim2.mutations.bed").exists()
    assert not (tmp_path / "p.annotation.sim.tsv").exists()


# ---- the command line -----------------------------------------------------------------------------------------------------------------------
def test_command_line_refusals():
    import importlib.util
    import os
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    spec = importlib.util.spec_from_file_location("predict_files", os.path.join(root, "tools", "predict_files.py"))
    tool = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(tool)
    base = ["m", "g.fa", "--regions", "chr1", "--no-table", "--summary", "p"]
    for extra, message in ((["--simulate", "5"], "--simulate needs --seed S"), (["--seed", "3"], "go with --simulate"),
                           (["--simulate", "5", "--seed", "3"], "--annotations BED"),
                           (["--simulate", "5", "--seed", "3", "--write_simulated", "5"], "below --simulate"),
                           (["--simulate", "0", "--seed", "3", "--write_simulated", "0"], "2^20")):
        with pytest.raises(SystemExit) as e:
            tool.main(base + extra)
        assert message in str(e.value) and "\n" not in str(e.value), extra      # one line
    flags, args, values = tool._split(base + ["--simulate", "5", "--seed", "0x10", "--write_simulated", "0", "3"])
    opts = tool._summary_options(flags, values)
    assert (opts["simulate"], opts["seed"], opts["write_simulated"]) == (5, 16, (0, 3)) and args == ["m", "g.fa"]
