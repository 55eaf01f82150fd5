"""The simulated null of the INDEL structure table on the host (mural_amd.summaries.simulate_txindel_host, the specification of
csrc/simulate_txindel.hip): the three defining identities -- (a) a replicate's column is the observed word of
``summary_txindel_host`` labelled with that replicate's draws, (b) ``simulate_indel_lof_counts`` gives the observed_lof /
observed_lof_upper integers of such a run, (c) parts through `into=` and permuted equal starts give the same bytes --, a known answer,
the status bits, the refusals, ``summary_txindel_host`` after the ``_txindel_pairs`` refactor against a brute-force oracle built anew
(tests/_txindel_sim_data.py), and the draw kernel's resource report."""
import os
import re

import numpy as np
import pytest

from tests import _txindel_sim_data as X

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
R = 5


def _sim(prob, start, strand, k, segments, features, n_tx, kind, n_rep=R, off=1, spec=None, **kw):
    from mural_amd.summaries import simulate_txindel_host
    return simulate_txindel_host(prob, start, strand, k, segments, features, n_tx, kind, X.KEY, X.SEED, n_rep, off, spec, **kw)


def _labels(prob, start, strand, k, n_rep=R):
    from mural_amd.summaries import simulate_rows_host
    return simulate_rows_host(prob, start, strand, k, X.KEY, X.SEED, np.arange(n_rep))


@pytest.fixture(scope="module", params=["toy", "random"])
def structure(request):
    text = X.toy_text() if request.param == "toy" else X.random_text()
    names, segments, features = X.read(text)
    if request.param == "random":
        assert len(names) == 20
    length = int(np.asarray(features["feat_b1"]).max()) + 25
    return dict(text=text, names=names, segments=segments, features=features, n_tx=len(names), length=length)


# ---- 1. identity (a) ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("k", [2, 5, 8])
@pytest.mark.parametrize("kind,off", [(0, 1), (0, 0), (1, 1), (1, 0), (2, 1), (2, 0)])
def test_a_replicate_is_the_observed_word_of_a_run_labelled_with_its_draws(structure, kind, off, k):
    from mural_amd.summaries import summary_txindel_host
    prob, start, strand, _ = X.rows(structure["length"], k, seed=kind + 3 * off + k)
    args = (k, structure["segments"], structure["features"], structure["n_tx"], kind)
    counts, status = _sim(prob, start, strand, *args, off=off, spec=X.LENGTHS[k], chrom_length=structure["length"] - 20)
    labels = _labels(prob, start, strand, k)
    assert status == 0 and counts.shape == (structure["n_tx"], 10, R) and counts.dtype == np.uint32 and counts.any()
    for r in range(R):
        table, _, st = summary_txindel_host(prob, start, labels[:, r], *args, off, X.LENGTHS[k], structure["length"] - 20)
        assert st == 0 and np.array_equal(counts[:, :, r], table[:, :, 0]), r


# ---- 2. identities (b) and (c) ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", [0, 1, 2])
def test_lof_counts_parts_and_permuted_equal_starts(structure, kind, tmp_path):
    from mural_amd import tables
    from mural_amd.summaries import simulate_indel_lof_counts, summary_txindel_host
    k = 8
    prob, start, strand, _ = X.rows(structure["length"], k, seed=20 + kind, extra=400)
    args = (k, structure["segments"], structure["features"], structure["n_tx"], kind)
    counts, status = _sim(prob, start, strand, *args)
    lof, upper = simulate_indel_lof_counts(counts)
    assert status == 0 and lof.shape == upper.shape == (structure["n_tx"], R) and (upper >= lof).all()
    labels = _labels(prob, start, strand, k)
    meta = dict(chrom=["chr1"] * structure["n_tx"], strand=[0] * structure["n_tx"])
    for r in (0, R - 1):      # (b): the integers the INDEL structure file prints for a run labelled with replicate r
        table, rows, _ = summary_txindel_host(prob, start, labels[:, r], *args)
        text = open(tables.write_indel_structure_outputs(structure["names"], meta, table, rows, kind, str(tmp_path / f"r{r}"))).read().splitlines()
        head = text[0].split("\t")
        for t, line in enumerate(text[1:]):
            f = line.split("\t")
            assert int(f[head.index("observed_lof")]) == lof[t, r] and int(f[head.index("observed_lof_upper")]) == upper[t, r]
    # (c): three parts through into=, the rows of equal starts in another order
    rng = np.random.default_rng(kind)
    perm = np.lexsort((rng.random(len(start)), start))
    assert not np.array_equal(perm, np.arange(len(start)))
    into = None
    for part in np.array_split(perm, 3):
        into, st = _sim(prob[part], start[part], strand[part], *args, into=into)
        assert st == 0
    assert into.tobytes() == counts.tobytes()
    shuffled = rng.permutation(len(start))      # any order of one call: the twin sorts; status 4 says that the rows did not ascend
    other, st = _sim(prob[shuffled], start[shuffled], strand[shuffled], *args)
    assert st == 4 and other.tobytes() == counts.tobytes()


# ---- 3. a known answer -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", [0, 1, 2])
@pytest.mark.parametrize("c", [1, 3, 7])
def test_a_certain_class_gives_the_row_counts_of_its_bins_in_every_replicate(structure, kind, c):
    from mural_amd.summaries import summary_txindel_host
    k = 8
    start = np.arange(structure["length"], dtype=np.int64)
    prob = np.zeros((len(start), k))
    prob[:, c] = 1
    args = (k, structure["segments"], structure["features"], structure["n_tx"], kind)
    counts, status = _sim(prob, start, None, *args)
    table, rows, _ = summary_txindel_host(prob, start, np.full(len(start), c), *args)
    assert status == 0 and (counts == table[:, :, :1].astype(np.uint32)).all() and counts.any()
    assert (counts.sum(axis=1) == rows[:, :1].astype(np.uint32)).all()      # every counted row lands in exactly one bin


# ---- 4. status bits, the clamp, the refusals ---------------------------------------------------------------------------------------------
def test_status_bits_and_bad_rows_draw_nothing(structure):
    k = 5
    prob, start, strand, _ = X.rows(structure["length"], k, seed=2)
    args = (k, structure["segments"], structure["features"], structure["n_tx"], 1)
    spec = X.LENGTHS[k]
    clean, status = _sim(prob, start, strand, *args, spec=spec)
    assert status == 0
    inside = int(np.nonzero(start >= int(np.asarray(structure["features"]["feat_b0"]).min()) + 3)[0][0])
    for value, bit in ((np.nan, 8), (-0.25, 8), (np.inf, 8)):
        bad = prob.copy()
        bad[inside] = 0
        bad[inside, 2] = value
        bad[inside + 1, 0] = np.nan                                            # class 0's probability is never read
        zero = prob.copy()
        zero[inside] = 0                                                       # a row that draws class 0 in every replicate
        got, st = _sim(bad, start, strand, *args, spec=spec)
        assert st == bit and got.tobytes() == _sim(zero, start, strand, *args, spec=spec)[0].tobytes()
    neg = start.copy()
    neg[0] = -3
    got, st = _sim(prob, neg, strand, *args, spec=spec)
    assert st == 1
    swapped = start.copy()
    swapped[40], swapped[41] = start[41] + 1, start[40]
    assert swapped[40] > swapped[41] and _sim(prob, swapped, strand, *args, spec=spec)[1] == 4
    above = prob.copy()                                                         # p_c above 1: clamped, not refused
    above[inside] = 0
    above[inside, 3] = 1.5
    one = above.copy()
    one[inside, 3] = 1.0
    got, st = _sim(above, start, strand, *args, spec=spec)
    assert st == 0 and got.tobytes() == _sim(one, start, strand, *args, spec=spec)[0].tobytes() != clean.tobytes()


def test_refusals(structure):
    prob, start, strand, _ = X.rows(structure["length"], 9, seed=2)
    args = (structure["segments"], structure["features"], structure["n_tx"], 0)
    with pytest.raises(ValueError, match=r"2 \.\. 8 classes.*SIM_MAX_CLASS"):
        _sim(prob, start, strand, 9, *args, spec="1,2,3,4,5,6,7,8")
    with pytest.raises(ValueError, match="2 .. 8"):
        _sim(prob, start, strand, 16, *args, spec=",".join(str(v) for v in range(1, 16)))
    for n_rep in (0, (1 << 20) + 1):
        with pytest.raises(ValueError, match="replicates"):
            _sim(prob[:, :8], start, strand, 8, *args, n_rep=n_rep)
    with pytest.raises(ValueError):
        _sim(prob[:, :8], start, strand, 8, structure["segments"], structure["features"], structure["n_tx"], 3)
    from mural_amd.summaries import simulate_indel_lof_counts
    with pytest.raises(ValueError, match="counts"):
        simulate_indel_lof_counts(np.zeros((2, 9, 3), np.uint32))


# ---- 5. the refactored summary twin against an oracle built anew ---------------------------------------------------------------------------
@pytest.mark.parametrize("kind,off,k", [(0, 1, 8), (0, 0, 5), (1, 1, 8), (1, 0, 2), (2, 1, 5), (2, 0, 8)])
def test_summary_txindel_host_equals_a_brute_force_oracle_word_for_word(kind, off, k):
    from mural_amd import tables
    from mural_amd.summaries import summary_txindel_host
    text = X.toy_text() + X.random_text(seed=3)
    names, segments, features = X.read(text)
    length = int(np.asarray(features["feat_b1"]).max()) - 15      # the chromosome ends inside the last transcripts; no row lies beyond it
    prob, start, _, label = X.rows(length - 1, k, seed=50 + kind)
    pairs = [tuple(r) for r in tables.check_indel_lengths(X.LENGTHS[k], k)[1:].tolist()]
    for chrom_len in (None, length):
        table, rows, status = summary_txindel_host(prob, start, label, k, segments, features, len(names), kind, off, X.LENGTHS[k], chrom_len)
        want = X.oracle(text, prob, start, label, k, kind, off, pairs, chrom_len)
        assert status == 0 and table.tolist() == want[0] and rows.tolist() == want[1]
    assert sum(1 for b in range(10) if any(cells[b][0] for cells in want[0])) >= (8 if k == 8 else 5)


# ---- 6. the draw kernel's resources ----------------------------------------------------------------------------------------------------------
def test_the_draw_kernel_does_not_spill():
    path = os.path.join(ROOT, "mural_amd", "csrc", "simulate_txindel.resources.txt")
    if not os.path.exists(path):
        pytest.skip("no resource report: the library was not built from this tree")
    text = open(path).read()
    blocks = re.split(r"remark: Function Name: ", text)[1:]
    draw = [b for b in blocks if "simulate_txindel_draw_kernel" in b.splitlines()[0]]
    assert len(draw) == 2                                   # float and double
    for b in draw:
        assert int(re.search(r"ScratchSize \[bytes/lane\]: (\d+)", b).group(1)) == 0, b
