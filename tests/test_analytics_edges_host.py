"""What tests/_analytics_edges_data.py promises about its inputs and references, checked on the CPU before a GPU sees them: the paths
the group cases are meant to take, the exactness of the 2^-20 probabilities, the float32 facts about the bin bounds, the cap on the rows
left out near a bound, the clipped / unclipped mix of the large-weight fit case, and the restated references against oracle/eval_ref.py."""
import numpy as np
import pytest
import torch

from oracle import eval_ref
from tests import _analytics_edges_data as D


# ------------------------------------------------------------------------------------------------------------------ keys
def test_kmer_reference_and_the_31_bit_case():
    assert 8 * 5 ** 12 < 2 ** 31 <= 9 * 5 ** 12
    for d in range(1, 7):
        for name, ncols, left0, right0 in D.kmer_layouts(d):
            cols = D.flank_cols(left0, right0, d)
            assert len(set(cols)) == 2 * d and min(cols) >= 0 and max(cols) < ncols, (d, name)
            codes = D.kmer_codes(257, ncols, left0, right0, d, d)
            keys, status = D.kmer_keys_ref(codes, left0, right0, d)
            assert status == 0 and keys[0] == 0 and keys[-1] == 5 ** (2 * d) - 1 and keys.min() >= 0
            # the same keys from oracle/eval_ref.py's column list where the layout is the product's (snv: a mid column; indel: none)
            if name == "2d":
                assert cols == eval_ref.flank_columns(ncols, 2 * d, "indel")
            # every column outside the flanks holds a value that would be refused in a flank
            outside = [c for c in range(ncols) if c not in cols]
            assert all(((codes[:, c] < 0) | (codes[:, c] > 4)).all() for c in outside)
            # regions: rows past the last whole region get -1 and no status
            keys, status = D.kmer_keys_ref(codes, left0, right0, d, 100, 2)
            assert status == 0 and (keys[200:] == -1).all() and (keys[:200] >= 0).all() and keys[199] // 5 ** (2 * d) == 1
            for bad in D.BAD_CODES:
                c2 = codes.copy()
                c2[100, cols[-1]] = bad
                k2, status = D.kmer_keys_ref(c2, left0, right0, d)
                assert status == 1 and k2[100] == -1 and (np.delete(k2, 100) == np.delete(D.kmer_keys_ref(codes, left0, right0, d)[0], 100)).all()
            for n in D.KMER_ROWS:
                regions = D.kmer_regions(n, d)
                assert regions * 5 ** (2 * d) < 2 ** 31 and regions * 100 < n
                keys, status = D.kmer_keys_ref(D.kmer_codes(n, ncols, left0, right0, d, n), left0, right0, d, 100, regions)
                assert status == 0 and (keys[regions * 100:] == -1).all() and (keys[:regions * 100] >= 0).all()
    assert D.kmer_regions(65537, 6) == 8 and D.kmer_regions(65537, 4) == 655
    codes = D.kmer_codes(65537, 12, 0, 6, 6, 99)
    keys, _ = D.kmer_keys_ref(codes, 0, 6, 6, 8192, 8)
    assert keys[-1] == -1 and keys[:-1].min() >= 0 and keys.max() < 2 ** 31


def test_window_reference():
    for window in (1, 1000, 10 ** 12):
        for n_chrom in (1, 25):
            chrom, start, base = D.window_case(4099, window, n_chrom, 3)
            keys, status = D.window_keys_ref(chrom, start, window, base, n_chrom)
            assert status == 0 and keys.min() >= 0
            assert n_chrom == 1 or (np.diff(base) < 0).any()
            assert start[0] == 0 and keys[0] == base[chrom[0]]
            if window == 1000:
                assert start[1] == 999 and keys[1] == base[chrom[1]] and start[2] == 1000 and keys[2] == base[chrom[2]] + 1
            if window > 50000:
                assert (keys == base[chrom]).all()


# ------------------------------------------------------------------------------------------------------------------ group_obs_pred
@pytest.mark.parametrize("nc", D.GROUP_CLASSES)
def test_group_cases_take_the_paths_they_are_meant_to(nc):
    for n in D.EQUAL_ROWS:
        keys, label = np.full(n, 5), np.arange(n) % nc
        assert D.wave_paths(keys, label, nc, 8) == (n // 64, n % 64), n
    # runs of 64, 96, 100: wave 0 uniform, wave 1 uniform (run 2 covers rows 64..159), wave 2 straddles, ...
    keys = D.run_keys(40)
    uniform, lanes = D.wave_paths(keys, keys * 0, nc, 40)
    assert uniform >= 10 and lanes >= 640 and uniform * 64 + lanes == len(keys)
    perm = np.random.default_rng(1).permutation(len(keys))
    assert D.wave_paths(keys[perm], keys * 0, nc, 40) == (0, len(keys))
    # one hole in a wave of equal keys: that wave goes lane by lane and counts 63
    keys, label = np.full(256, 5), np.arange(256) % nc
    for hole_key, hole_label in ((-1, 0), (5, -1), (5, nc), (8, 0)):
        k2, l2 = keys.copy(), label.copy()
        k2[70], l2[70] = hole_key, hole_label
        assert D.wave_paths(k2, l2, nc, 8) == (3, 63)
    lo, hi = D.lds_boundary_groups(nc)
    assert D.uses_lds(nc, lo) and not D.uses_lds(nc, hi)
    assert lo * (1 + 2 * nc) <= 4096 < hi * (1 + 2 * nc) and (lo + 1) * (1 + 2 * nc) > 4096
    if nc == 1:
        assert (lo, hi) == (1365, 1366) and lo * 3 == 4095


@pytest.mark.parametrize("nc", D.GROUP_CLASSES)
def test_exact_probabilities_sum_exactly_in_any_order(nc):
    p64, p32 = D.group_probs(5000, nc, "exact", nc)
    assert np.array_equal(p32.astype(np.float64), p64) and np.array_equal(p64 * 2 ** 20, np.round(p64 * 2 ** 20))
    assert p64.min() >= 0 and p64.max() <= 1
    assert D.BIG_GROUP_ROWS * 2 ** 20 < 2 ** 53                       # every partial sum of the largest case is an integer below 2^53
    keys = np.random.default_rng(nc).integers(0, 7, size=5000)
    table, S, status = D.group_ref(keys, keys % nc, p64, nc, 7)
    perm = np.random.default_rng(2).permutation(5000)
    t2, _, _ = D.group_ref(keys[perm], (keys % nc)[perm], p64[perm], nc, 7)
    assert status == 0 and np.array_equal(table, t2) and np.array_equal(table[:, 1 + nc:], S[:, 1 + nc:])
    # and the Dirichlet rows differ between the formats (so both are worth running)
    q64, q32 = D.group_probs(100, nc, "dirichlet", nc)
    assert not np.array_equal(q32.astype(np.float64), q64)


def test_group_reference_statuses_and_the_big_formula():
    keys = np.array([0, 1, -1, -7, 2, 3, 1, 0])
    label = np.array([0, 1, 0, 1, 0, 1, 0, 1])
    p = np.full((8, 2), 0.25)
    table, _, status = D.group_ref(keys, label, p, 2, 4)
    assert status == 0 and table[:, 0].tolist() == [2, 2, 1, 1]
    for at, (k, lab) in zip((0, 1, 4), ((4, 0), (1, -1), (1, 2))):
        k2, l2 = keys.copy(), label.copy()
        k2[at], l2[at] = k, lab
        t2, _, status = D.group_ref(k2, l2, p, 2, 4)
        assert status == 2 and t2[:, 0].sum() == 5
    i = np.arange(D.BIG_GROUP_ROWS, dtype=np.int64)
    k, lab, num = D.big_group_formula(i)
    assert k.min() == 0 and k.max() == D.BIG_GROUPS - 1 and not lab.any() and num.min() >= 0 and num.max() <= 2 ** 20
    assert np.bincount(k).min() > 3000                                   # every group is hit, none dominates
    kt, _, numt = D.big_group_formula(torch.arange(5000, dtype=torch.int64))
    assert np.array_equal(kt.numpy(), k[:5000]) and np.array_equal(numt.numpy(), num[:5000])
    assert D.uses_lds(1, D.BIG_GROUPS) and D.BIG_GROUP_ROWS > 2048 * 2048


# ------------------------------------------------------------------------------------------------------------------ calib_metrics
def test_float32_bin_bounds():
    for k in (2, 4, 8, 16):
        b = D.calib_bounds(80)
        assert b.dtype == torch.float32 and float(b[80 // k]) == 1.0 / k, k
    assert float(D.calib_bounds(50)[25]) == 0.5
    for nb in D.CALIB_BINS:
        b = D.calib_bounds(nb)
        assert float(b[0]) == 0.0 and float(b[-1]) == 1.0 and bool((b[1:] > b[:-1]).all())
    assert D.calib_cells(16, 80) == 4082 <= 4096 < D.calib_cells(16, 81) == 4133


@pytest.mark.parametrize("dtype", ["float32", "float64"])
@pytest.mark.parametrize("nc", D.CALIB_CLASSES)
def test_rows_left_out_near_a_bound_stay_under_the_cap(dtype, nc):
    for nb in D.CALIB_BINS:
        for n in D.CALIB_ROWS:
            for scale in (1.0,) if n != 257 else (1.0, 0.5, 3.0):
                prob, label, excluded = D.calib_case(dtype, nc, nb, n, scale)
                assert prob.shape == (n, nc) and prob.dtype == np.dtype(dtype) and (prob > 0).all()
                assert excluded <= D.EXCLUDE_CAP * n, (dtype, nc, nb, n, scale, excluded)
                assert nc == 1 or not D.near_a_bound(prob, nb).any()      # (one class: the score is exactly 1, nothing is left out)
                if scale != 1.0 and nc > 1:
                    assert abs(float(prob[0].astype(np.float64).sum()) - scale) < 1e-5


def test_float32_and_float64_scores_fall_in_the_same_bins():
    """20 000 Dirichlet(0.7) rows, 50 bins: the two precisions disagree on no bin (the room under the cap)"""
    for nc in (2, 3, 4, 8, 16):
        rng = np.random.default_rng(nc)
        p = D._dirichlet(rng, 20000, nc, np.float32)
        y = np.zeros(20000, np.int64)
        q64 = D._scores_np(p, y, np.float64)[0]
        q32 = D._scores_torch32(p, y)[0]
        b = D.calib_bounds(50).double().numpy()
        keep = ~D.near_a_bound(p, 50)
        assert (~keep).mean() <= D.EXCLUDE_CAP
        assert np.array_equal(np.searchsorted(b, q64[keep], "left"), np.searchsorted(b, q32[keep], "left"))


@pytest.mark.parametrize("dtype", ["float32", "float64"])
def test_calib_reference_against_eval_ref_and_by_hand(dtype):
    # the four summary numbers eval_ref derives, from the per-cell vector
    for nc, nb, n in ((3, 50, 4099), (4, 15, 257), (16, 80, 256)):
        prob, label, _ = D.calib_case(dtype, nc, nb, n)
        label = label.copy()
        label[0] = nc - 1                                   # (eval_ref takes the class count from the largest label)
        ref = D.calib_reference(prob, label, nb)
        want = eval_ref.calibration_metrics(prob, label, nb)
        out = ref["want"]
        bins = out[2:].reshape(1 + nc, nb, 3)

        def ece(c):
            live = c[:, 0] > 0
            return float(np.sum(np.abs(c[live, 1] - c[live, 2]) / n))

        # (hand-set, host-only: they hold the per-cell restatement against eval_ref's four float32-evaluated numbers; no kernel is judged by them)
        tol = 1e-5 if dtype == "float32" else 1e-12
        assert abs(out[0] / n - want["nll"]) < tol and abs(out[1] / n - want["brier"]) < tol
        tol = max(tol, 1e-7)                                # (eval_ref's hit rates and bin weights are float32 means whatever the input)
        assert abs(ece(bins[0]) - want["ece"]) < tol and abs(np.mean([ece(bins[1 + c]) for c in range(nc)]) - want["c_ece"]) < tol
        assert bins[:, :, 0].sum() == n * (1 + nc) and ref["status"] == 0 and (ref["bound"][ref["exact"]] == 0).all()
        assert (ref["ref_err"] <= ref["bound"]).all()
    # by hand: uniform rows sit ON the bound 1 / k and belong to the bin below it
    for nc, nb in ((2, 80), (4, 80), (8, 80), (16, 80), (2, 50)):
        prob, label = D.calib_exact_case("uniform", nc, dtype)
        ref = D.calib_reference(prob, label, nb)
        bins = ref["want"][2:].reshape(1 + nc, nb, 3)
        b = nb // nc - 1
        assert (bins[:, b, 0] == 70).all() and bins[:, :, 0].sum() == 70 * (1 + nc) and (bins[:, b, 1] == 70.0 / nc).all()
        assert bins[0, b, 2] == (label == 0).sum() and all(bins[1 + c, b, 2] == (label == c).sum() for c in range(nc))
        assert not D.near_a_bound(prob[:0], nb).any() and D.near_a_bound(prob, nb).all()     # (the rule would drop them: it is not applied)
    # one-hot rows: 1 in the last bin, 0 in no bin; a label on a zero class makes the NLL infinite
    for nc in (2, 4, 16):
        prob, label = D.calib_exact_case("onehot", nc, dtype)
        ref = D.calib_reference(prob, label, 15)
        bins = ref["want"][2:].reshape(1 + nc, 15, 3)
        assert ref["want"][0] == np.inf and bins[:, :14].sum() == 0 and bins[0, 14, 0] == 70 and bins[1:, 14, 0].sum() == 70
        hot = (np.arange(70) // 2) % nc
        assert ref["want"][1] == 2.0 * (hot != label).sum() and bins[0, 14, 2] == (hot == label).sum()
    prob, label = D.calib_exact_case("single", 1, dtype)
    ref = D.calib_reference(prob, label, 15)
    assert ref["want"][0] == 0 and ref["want"][1] == 0 and ref["want"][2 + 3 * 14] == 70 and ref["want"][2 + 3 * 15 + 3 * 14 + 1] == 70
    # a bad label: status 2, the row is nowhere
    prob, label, _ = D.calib_case(dtype, 3, 15, 257)
    bad = label.copy()
    bad[[5, 200]] = (-1, 3)
    ref = D.calib_reference(prob, bad, 15)
    keep = np.ones(257, bool)
    keep[[5, 200]] = False
    assert ref["status"] == 2 and np.array_equal(ref["want"], D.calib_reference(prob[keep], label[keep], 15)["want"])


def test_big_calib_formula():
    i = np.arange(D.BIG_CALIB_ROWS, dtype=np.int64)
    m, lab = D.big_calib_formula(i)
    assert m.min() == 1 and m.max() == 1023 and not (m == 512).any() and set(np.unique(lab)) == {0, 1}
    mt, labt = D.big_calib_formula(torch.arange(5000, dtype=torch.int64))
    assert np.array_equal(mt.numpy(), m[:5000]) and np.array_equal(labt.numpy(), lab[:5000])
    prob = np.stack([m, 1024 - m], axis=1).astype(np.float32) / np.float32(1024)
    assert np.array_equal(prob.astype(np.float64).sum(axis=1), np.ones(len(m)))
    assert not D.near_a_bound(prob[:20000], 2).any() and D.BIG_CALIB_ROWS > 1024 * 2048


# ------------------------------------------------------------------------------------------------------------------ dirichlet_fit_terms
@pytest.mark.parametrize("dtype", ["float32", "float64"])
def test_fit_features_take_the_log_in_the_inputs_precision(dtype):
    prob, _ = D.fit_probs(1000, 4, dtype, 11)
    assert prob.dtype == np.dtype(dtype) and (prob[1] == 0).any() and (prob[2] == 1).any()
    assert 0 < prob[3, 0] < np.finfo(prob.dtype).tiny
    X = D.fit_features(prob)
    assert np.array_equal(X, eval_ref.fit_features(prob)) and X.dtype == np.float64
    tiny = np.finfo(prob.dtype).tiny
    assert X[1].min() == float(np.log(tiny)) and X[3, 0] == float(np.log(tiny)) and X[2, 1] == 0.0
    if dtype == "float32":
        assert np.array_equal(X[:, :4].astype(np.float32).astype(np.float64), X[:, :4])
        assert not np.array_equal(X[:, :4], np.log(np.clip(prob.astype(np.float64), tiny, 1)))


@pytest.mark.parametrize("dtype", ["float32", "float64"])
@pytest.mark.parametrize("k", D.FIT_CLASSES)
@pytest.mark.parametrize("kind", D.FIT_WEIGHTS)
def test_fit_reference_and_the_clipped_mix(dtype, k, kind):
    for n in D.FIT_ROWS:
        prob, label, w, reps, tail, ref = D.fit_case(dtype, k, kind, n)
        assert reps * len(label) + tail == n == ref["rows"] and ref["status"] == 0
        # the restated row terms add up to eval_ref's.  1e-9 is hand-set and host-only: it guards the restatement and judges no kernel
        # (eval_ref's matrix products round z differently, and exp(z) carries it on)
        assert (np.abs(ref["own_sum"] - ref["want"]) <= 1e-9 * ref["mag"]).all()
        # Host-only guards (hand-set, about twice what these cases show) that keep the two additions to the issue's fit bound from
        # making it vacuous should eval_ref or numpy change: eval_ref's own distance from longdouble stays a fraction of the rest of
        # the bound over a case's entries (entry by entry it may reach a few times the rest where the rest is the any-order floor),
        # and taking the longdouble log too widens the float64 bound by less than 2 over a case's entries (a single entry whose
        # float64 term happens to be exact with the float64 log has no ratio worth a guard)
        rest = ref["bound"] - ref["own"]
        assert ref["own"].sum() <= 0.25 * rest.sum() and (ref["own"] <= 4.0 * rest + 1e-300).all(), (k, kind, n)
        assert ref["main"].sum() <= 2.0 * ref["main_same_log"].sum(), (k, kind, n)
        assert (ref["ref_err"] <= ref["bound"]).all() and np.isfinite(ref["bound"]).all()
        live, sy = ref["live"], ref["sy"]
        # no row sits where a last-bit difference of a feature could switch the clip of s_y on or off: one float32 ulp on each of k
        # log features (at most 2^-17, at |log tiny| = 87) under weights of 40 moves a logit by at most 8 * 40 * 2^-17 < 0.0025,
        # s_y by a factor below exp(0.005) < 1.01
        # (at the upper end the terms that the clip removes are 2^-52 times the features: nothing to switch)
        assert not ((sy > D.EPS64 / 1.01) & (sy < D.EPS64 * 1.01)).any()
        if kind == "mag40":
            assert np.abs(w).min() == 40 == np.abs(w).max()
            if n > 1:
                assert (~live).any() and live.any(), (k, n, int(live.sum()))
                assert (sy[~live] < D.EPS64).any() and (sy[~live] > 1 - D.EPS64).any() and live[4] and not live[2]
        elif kind == "identity" and n > 1:
            assert not live[2]                             # the one-hot row: s_y = 1 to the last bit
