"""Inputs and float64 references of the edge tests of the five evaluation reductions (csrc/analytics.hip: mural_eval_kmer_keys,
_window_keys, _group_obs_pred, _calib_metrics, _dirichlet_fit_terms).  CPU only (numpy / torch-CPU): tests/test_analytics_edges_host.py
checks here what the inputs are meant to be, tests/test_gpu_analytics_edges.py runs them through the C entries.

Tolerances are derived, never tuned:
  * key kernels, row counts, label counts and hits: bit equality;
  * float64 atomic sums of m terms in any order: 2 (m + 2) 2^-53 sum|term| (``any_order_bound``: tests/_parity.py's ``_sum_check`` with
    the float64 unit roundoff); probabilities that are multiples of 2^-20 make every partial sum exact, so those tables are bit-equal;
  * anything with a log / exp in it: 8 x the distance of the same formula one precision down from the formula one precision up (torch
    float32 against float64 for float32 input, numpy float64 against longdouble for float64 input), at least 4 ulp, row by row and
    added up over the rows of a sum (the rule of ``_loose`` applied as test_gpu_step_ops.py's ``_ce_loss_bound`` applies it)."""
import functools

import numpy as np
import torch
import torch.nn.functional as F

from oracle import eval_ref

U53 = 2.0 ** -53
KEY_SENTINEL = -123456789            # what the key outputs hold before every call
AN_THREADS, AN_LDS_DOUBLES = 256, 4096


def any_order_bound(m, S):
    """|float64 sum of m terms in any order - exact sum| <= 2 (m + 2) 2^-53 sum|term|, element by element"""
    return 2.0 * (np.asarray(m, np.float64) + 2.0) * U53 * np.asarray(S, np.float64)


# ================================================================================================================== key kernels
KMER_ROWS = [1, 255, 256, 257, 65537]
JUNK = np.array([5, -1, 1 << 40, 7, -(1 << 35), (1 << 32) + 2], np.int64)      # what the columns outside the flanks hold
BAD_CODES = [5, -1, 1 << 40]


def kmer_layouts(d):
    """(name, ncols, left0, right0): the flanks fill the row; 2d + 3 columns with the left flank on column 0 (a mid column between the
    flanks, two unused columns behind); 2d + 3 columns with the right flank on the last column (two unused columns in front)"""
    return [("2d", 2 * d, 0, d), ("2d+3 first", 2 * d + 3, 0, d + 1), ("2d+3 last", 2 * d + 3, 2, d + 3)]


def flank_cols(left0, right0, d):
    return list(range(left0, left0 + d)) + list(range(right0, right0 + d))


def kmer_codes(n, ncols, left0, right0, d, seed):
    """codes 0..4 in the flank columns (row 0 all 0, the last row all 4: the smallest and the largest key), JUNK everywhere else"""
    rng = np.random.default_rng(seed)
    codes = rng.integers(0, 5, size=(n, ncols)).astype(np.int64)
    cols = flank_cols(left0, right0, d)
    for c in range(ncols):
        if c not in cols:
            codes[:, c] = JUNK[rng.integers(0, len(JUNK), size=n)]
    codes[0, cols] = 0
    codes[n - 1, cols] = 4
    return codes


def kmer_keys_ref(codes, left0, right0, d, region_size=0, n_regions=0):
    """(int32 keys, status): the base-5 number of the 2d flank codes, + region * 5^(2d) for rows of a whole region, -1 for rows past the
    last one; a flank code outside 0..4 gives -1 for its row and status 1"""
    n = codes.shape[0]
    flank = codes[:, flank_cols(left0, right0, d)]
    bad = ((flank < 0) | (flank > 4)).any(axis=1)
    key = np.zeros(n, np.int64)
    for j in range(2 * d):
        key = key * 5 + np.where(bad, 0, flank[:, j])
    if region_size > 0:
        reg = np.arange(n, dtype=np.int64) // region_size
        key = np.where(reg < n_regions, reg * 5 ** (2 * d) + key, -1)
    key[bad] = -1
    assert key.max(initial=0) < 2 ** 31
    return key.astype(np.int32), int(bad.any())


def kmer_regions(n, d):
    """regions of 100 rows: the whole ones among n rows, or as many as 31 bits hold keys for"""
    return min(n // 100, (2 ** 31 - 1) // 5 ** (2 * d))


WINDOW_ROWS = [1, 257, 4099]


def window_case(n, window, n_chrom, seed):
    """(chrom_id int32, start int64, chrom_base int64): starts below 50000 with 0, window - 1 and window among them (where they are
    below 50000); chrom_base a shuffled multiple of the slots per chromosome, so it is not monotone"""
    rng = np.random.default_rng(seed)
    chrom = rng.integers(0, n_chrom, size=n).astype(np.int32)
    start = rng.integers(0, 50000, size=n).astype(np.int64)
    for row, s in enumerate((0, window - 1, window)):
        if row < n and s < 50000:
            start[row] = s
    per = 50000 // window + 1
    base = (rng.permutation(n_chrom) * per).astype(np.int64)
    return chrom, start, base


def window_keys_ref(chrom, start, window, base, n_chrom):
    bad = (chrom < 0) | (chrom >= n_chrom) | (start < 0)
    key = base[np.clip(chrom, 0, n_chrom - 1)] + np.where(bad, 0, start) // window
    key[bad] = -1
    return key.astype(np.int32), int(bad.any())


# ================================================================================================================== group_obs_pred
GROUP_CLASSES = [1, 2, 3, 4, 5, 8, 16]
EQUAL_ROWS = [1, 63, 64, 65, 256, 257, 2048 * 256 + 65]
BIG_GROUP_ROWS = 2048 * 2048 + 300      # beyond one round of the capped grid (2048 workgroups x 2048 rows)
BIG_GROUPS = 1000


def wave_paths(keys, label, nc, n_groups):
    """(waves on the one-atomic-per-wave path, rows on the per-lane path) as the kernel's conditions give them: rows are padded with key
    -1 to a multiple of 256, a row with key >= n_groups or a label outside the classes turns to key -1, a wave of 64 equal keys >= 0
    is uniform, every other row with key >= 0 goes lane by lane.  (The grid's stride is a multiple of 256, so wave w is rows 64 w ..)"""
    k = np.asarray(keys, np.int64).copy()
    lab = np.asarray(label, np.int64)
    k[(k >= n_groups) | (lab < 0) | (lab >= nc)] = -1
    pad = (-len(k)) % AN_THREADS
    k = np.concatenate([k, np.full(pad, -1, np.int64)]).reshape(-1, 64)
    uniform = (k == k[:, :1]).all(axis=1)
    return int((uniform & (k[:, 0] >= 0)).sum()), int((k[~uniform] >= 0).sum())


def uses_lds(nc, n_groups):
    return n_groups * (1 + 2 * nc) <= AN_LDS_DOUBLES


def lds_boundary_groups(nc):
    """(the largest n_groups whose table is privatised in LDS, the smallest that takes global atomics)"""
    g = AN_LDS_DOUBLES // (1 + 2 * nc)
    return g, g + 1


def group_probs(n, nc, kind, seed):
    """(float64 rows, float32 rows).  'exact': multiples of 2^-20 in [0, 1], the same numbers in both formats; 'dirichlet': Dirichlet(0.7)
    rows (uniform numbers for one class) and their float32 cast"""
    rng = np.random.default_rng(seed)
    if kind == "exact":
        p64 = rng.integers(0, 2 ** 20 + 1, size=(n, nc)).astype(np.float64) / 2.0 ** 20
    elif nc == 1:
        p64 = rng.random((n, 1))
    else:
        g = rng.standard_gamma(0.7, size=(n, nc)) + 1e-300
        p64 = g / g.sum(axis=1, keepdims=True)
    return p64, p64.astype(np.float32)


def group_ref(keys, label, prob, nc, n_groups):
    """(table, abs-sum table, status): float64 (n_groups, 1 + 2 nc) by np.bincount over the rows the kernel keeps (0 <= key < n_groups
    and 0 <= label < nc); status 2 when a key >= n_groups or a label outside the classes is among the rows"""
    keys, label = np.asarray(keys, np.int64), np.asarray(label, np.int64)
    bad = (keys >= n_groups) | (label < 0) | (label >= nc)
    live = (keys >= 0) & ~bad
    k, lab, p = keys[live], label[live], np.asarray(prob, np.float64)[live]
    table = np.zeros((n_groups, 1 + 2 * nc))
    S = np.zeros_like(table)
    table[:, 0] = np.bincount(k, minlength=n_groups)
    for c in range(nc):
        table[:, 1 + c] = np.bincount(k, weights=(lab == c), minlength=n_groups)
        table[:, 1 + nc + c] = np.bincount(k, weights=p[:, c], minlength=n_groups)
        S[:, 1 + nc + c] = np.bincount(k, weights=np.abs(p[:, c]), minlength=n_groups)
    return table, S, 2 if bad.any() else 0


def group_bound(table, S):
    """the any-order bound of every cell: m = the group's row count"""
    return any_order_bound(table[:, :1], S)


def run_keys(n_groups, rows=4000):
    """sorted keys in runs of 64, 96 and 100 rows: wave 0 (rows 0..63, the first run) and wave 1 (rows 64..127, inside the second run) are
    uniform, wave 2 (rows 128..191) straddles the second and the third run and goes lane by lane, and so on with every alignment"""
    runs, g = [], 0
    while sum(runs) < rows:
        runs.append((64, 96, 100)[g % 3])
        g += 1
    return np.repeat(np.arange(len(runs)) % n_groups, runs).astype(np.int32)


def big_group_formula(i):
    """(keys, label, numerator of prob over 2^20) of row i; `i` an int64 numpy array or torch tensor (only + * % >> are used, and no
    product passes 2^53)"""
    h = (i * 1103515245 + 12345) % 2147483648
    return (h >> 11) % BIG_GROUPS, i * 0, (i * 48271 + 11) % 1048577


# ================================================================================================================== calib_metrics
CALIB_CLASSES = [1, 2, 3, 4, 8, 16]
CALIB_BINS = [1, 2, 15, 50, 80]
CALIB_ROWS = [1, 255, 256, 257, 4099]
BIG_CALIB_ROWS = 1024 * 2048 + 129      # beyond one round of the capped grid (1024 workgroups x 2048 rows)
EXCLUDE_ULP = 4
EXCLUDE_CAP = 0.001
SPARE_ROWS = 16


def calib_cells(nc, nb):
    return 2 + 3 * nb * (1 + nc)


def calib_bounds(nb):
    return torch.linspace(0, 1, nb + 1)


def _scores_np(p, y, T):
    """softmax(log p), the cross entropy -log softmax(log p)[y] and the Brier term of every row, evaluated in numpy type T"""
    n, nc = p.shape
    with np.errstate(divide="ignore"):
        l = np.log(p.astype(T))
    m = l.max(axis=1, keepdims=True)
    e = np.exp(l - m)
    s = e.sum(axis=1, keepdims=True)
    q = e / s
    ar = np.arange(n)
    nll = -(l[ar, y] - m[:, 0] - np.log(s[:, 0]))
    hot = (y[:, None] == np.arange(nc)[None, :]).astype(T)
    return q, nll, ((hot - q) ** 2).sum(axis=1)


def _scores_torch32(p, y):
    """the same three in torch-CPU float32, with eval_ref.calibration_metrics' own calls"""
    lg = torch.log(torch.from_numpy(np.ascontiguousarray(p)))
    yt = torch.from_numpy(y).long()
    q = F.softmax(lg, dim=1)
    nll = F.cross_entropy(lg, yt, reduction="none")
    brier = torch.sum((F.one_hot(yt, p.shape[1]).to(q.dtype) - q) ** 2, dim=1)
    return q.numpy().astype(np.float64), nll.numpy().astype(np.float64), brier.numpy().astype(np.float64)


def _two_precisions(p, y):
    """((q, nll, brier) one precision up, the same in the input's precision, ulp function of the input's precision)"""
    if p.dtype == np.float32:
        return _scores_np(p, y, np.float64), _scores_torch32(p, y), lambda v: np.spacing(np.asarray(v, np.float64).astype(np.float32)).astype(np.float64)
    return _scores_np(p, y, np.longdouble), _scores_np(p, y, np.float64), lambda v: np.spacing(np.asarray(v).astype(np.float64))


def near_a_bound(prob, nb):
    """rows of which some reference score lies within EXCLUDE_ULP ulp (of prob's precision, taken at the bound) of a bin bound"""
    prob = np.ascontiguousarray(prob)
    (q, _, _), _, _ = _two_precisions(prob, np.zeros(len(prob), np.int64))
    b = calib_bounds(nb).numpy()
    width = EXCLUDE_ULP * np.spacing(b.astype(prob.dtype)).astype(np.float64)
    q = q.astype(np.float64)
    return (np.abs(q[:, :, None] - b.astype(np.float64)[None, None, :]) <= width[None, None, :]).any(axis=(1, 2))


def calib_reference(prob, label, nb):
    """dict(want, bound, ref_err, exact, status): the whole `out` vector of mural_eval_calib_metrics over the rows with a label inside the
    classes.  want: float64 (sums of the one-precision-up scores); exact: the cells that are row or hit counts; bound / ref_err: per
    cell, the rows' max(8 |lower precision - higher|, 4 ulp) added up, score by score, + the any-order bound of the float64 atomics / the distance of
    the lower-precision sum.  An infinite NLL (a label on a class of probability 0) has want = inf and bound 0."""
    prob = np.ascontiguousarray(prob)
    label = np.asarray(label, np.int64)
    nc = prob.shape[1]
    ok = (label >= 0) & (label < nc)
    p, y = prob[ok], label[ok]
    n = len(y)
    (qh, nllh, brh), (ql, nlll, brl), ulp = _two_precisions(p, y)
    b = calib_bounds(nb).numpy()
    cells = calib_cells(nc, nb)
    want, bound, ref_err = np.zeros(cells), np.zeros(cells), np.zeros(cells)
    exact = np.zeros(cells, bool)

    def row_bound(hi, lo):
        hi64 = np.asarray(hi, np.float64)
        with np.errstate(invalid="ignore"):
            return np.maximum(8.0 * np.abs(np.asarray(lo, np.float64) - hi64), 4.0 * ulp(hi64))

    for at, hi, lo in ((0, nllh, nlll), (1, brh, brl)):
        fin = np.isfinite(np.asarray(hi, np.float64))
        want[at] = float(hi.sum()) if fin.all() else float(np.asarray(hi, np.float64).sum())
        if fin.all():
            bound[at] = row_bound(hi, lo).sum() + any_order_bound(n, np.abs(np.asarray(hi, np.float64)).sum())
            ref_err[at] = abs(float(lo.sum()) - want[at])
    # scores: column 0 the confidence (first maximum), columns 1.. the classes
    arg = np.argmax(qh, axis=1) if n else np.zeros(0, np.int64)
    ar = np.arange(n)
    vh = np.concatenate([qh[ar, arg][:, None], qh], axis=1)
    vl = np.concatenate([ql[ar, np.argmax(ql, axis=1) if n else arg][:, None], ql], axis=1)
    hit = np.concatenate([(arg == y)[:, None], y[:, None] == np.arange(nc)[None, :]], axis=1)
    bins = np.searchsorted(b.astype(vh.dtype), vh, side="left") - 1          # (lower, upper]: v on a bound belongs below it
    inside = (bins >= 0) & (bins < nb)
    cell = 2 + 3 * (np.arange(1 + nc)[None, :] * nb + bins)
    cell, v_hi, v_lo, h = cell[inside], vh[inside], vl[inside], hit[inside]
    rb = row_bound(v_hi, v_lo)                               # (score by score: each its own distance and its own ulp)
    want[0 + np.arange(2, cells, 3)] = np.bincount(cell, minlength=cells)[2::3]
    want[1 + np.arange(2, cells, 3)] = np.bincount(cell, weights=v_hi.astype(np.float64), minlength=cells)[2::3]
    want[2 + np.arange(2, cells, 3)] = np.bincount(cell, weights=h, minlength=cells)[2::3]
    rows = np.bincount(cell, minlength=cells)[2::3]
    S = np.bincount(cell, weights=np.abs(v_hi.astype(np.float64)), minlength=cells)[2::3]
    bound[3::3] = np.bincount(cell, weights=rb, minlength=cells)[2::3] + any_order_bound(rows, S)
    ref_err[3::3] = np.abs(np.bincount(cell, weights=v_lo, minlength=cells)[2::3] - want[3::3])
    exact[2::3] = exact[4::3] = True
    return dict(want=want, bound=bound, ref_err=ref_err, exact=exact, status=0 if ok.all() else 2, rows=n)


def _dirichlet(rng, n, nc, dtype):
    if nc == 1:
        return (0.05 + 0.95 * rng.random((n, 1))).astype(dtype)
    g = rng.standard_gamma(0.7, size=(n, nc)) + 1e-30
    return (g / g.sum(axis=1, keepdims=True)).astype(dtype)


@functools.lru_cache(maxsize=None)
def calib_case(dtype, nc, nb, n, scale=1.0):
    """(prob, label, excluded): n Dirichlet(0.7) rows x scale (0.5 and 3: unnormalised rows; the softmax renormalises them) with labels drawn
    uniformly, the first n of n + SPARE_ROWS generated rows that are not ``near_a_bound``; excluded: how many were passed over"""
    dtype = np.dtype(dtype)
    rng = np.random.default_rng([nc, nb, n, dtype.itemsize, int(scale * 2)])
    pool = (_dirichlet(rng, n + SPARE_ROWS, nc, np.float64) * scale).astype(dtype)
    label = rng.integers(0, nc, size=n + SPARE_ROWS)
    near = near_a_bound(pool, nb) if nc > 1 else np.zeros(len(pool), bool)      # (one class: the score is exactly 1)
    keep = np.flatnonzero(~near)[:n]
    assert len(keep) == n
    excluded = int(near[:keep[-1] + 1].sum())
    return np.ascontiguousarray(pool[keep]), label[keep], excluded


def calib_exact_case(kind, nc, dtype):
    """rows whose scores are exact whatever the math library, so no row is excluded: 'uniform' (every probability 1 / nc: log p is one
    number, every exponential exp(0) = 1, their sum nc: every score 1 / nc), 'onehot' (scores exactly 1 and 0; the label runs over the
    classes, so for nc > 1 some NLL terms are +inf), 'single' (nc = 1: the score is 1 whatever the probability)"""
    n = 70
    label = (np.arange(n) % nc).astype(np.int64)
    if kind == "uniform":
        prob = np.full((n, nc), 1.0 / nc, dtype)
    elif kind == "onehot":
        prob = np.zeros((n, nc), dtype)
        prob[np.arange(n), (np.arange(n) // 2) % nc] = 1.0
    else:
        assert nc == 1
        prob = np.linspace(0.01, 2.0, n).reshape(n, 1).astype(dtype)
    return prob, label


def big_calib_formula(i):
    """(numerator m of p0 = m / 1024 with p1 = 1 - p0, label) of row i: m in 1..1023 without 512, so the true scores (p0, p1) stay
    1 / 1024 away from the bounds 0, 0.5 and 1 of n_bins = 2 and no row is near a bound"""
    h = (i * 1103515245 + 12345) % 2147483648
    m = (h >> 7) % 1023 + 1
    m = m + (m == 512)
    return m, (h >> 3) % 2


# ================================================================================================================== dirichlet_fit_terms
FIT_CLASSES = [2, 3, 4, 5, 6, 7, 8]
FIT_LONG_BASE = 257
FIT_LONG_ROWS = 512 * 512 + 129        # beyond one round of the capped grid (512 workgroups x 512 rows)
FIT_ROWS = [1, 127, 128, 129, 1000, FIT_LONG_ROWS]
FIT_WEIGHTS = ["identity", "perturbed", "mag40"]
EPS64 = float(np.finfo(np.float64).eps)


def fit_weights(kind, k):
    rng = np.random.default_rng([k, FIT_WEIGHTS.index(kind)])
    ident = np.hstack([np.eye(k), np.zeros((k, 1))])
    if kind == "identity":
        return ident
    if kind == "perturbed":
        return ident + 0.3 * rng.standard_normal((k, k + 1))
    # +40 on the diagonal and in the intercepts, -40 elsewhere: logit differences are 80 log(p_j / p_j'), so s_y leaves [eps, 1 - eps] as
    # soon as the label's probability and the largest other one differ by a factor beyond exp(36 / 80) = 1.57
    return 40.0 * np.hstack([2.0 * np.eye(k) - 1.0, np.ones((k, 1))])


def fit_features(prob):
    """log(clip(p, tiny, 1 - tiny)) in prob's own precision, widened to float64, and a column of ones: what the kernel feeds on.
    eval_ref.fit_features states the same (the host test holds the two together)."""
    tiny = np.finfo(prob.dtype).tiny
    x = np.log(np.clip(prob, tiny, prob.dtype.type(1) - tiny))
    assert x.dtype == prob.dtype
    return np.hstack((x.astype(np.float64), np.ones((len(x), 1))))


def fit_probs(n, k, dtype, seed):
    """Dirichlet(0.7) rows; row 1 holds an exact 0 (clipped to the precision's tiny), row 2 is one-hot (an exact 1 and zeros), row 3 holds a
    subnormal, row 4 is uniform (equal logits under every weight matrix here whose rows differ only on the diagonal: never clipped), rows 5
    and 6 carry their label on the largest and on the smallest probability.  A single row is the row with the exact 0."""
    dtype = np.dtype(dtype)
    rng = np.random.default_rng([seed, k, n])
    prob = _dirichlet(rng, n, k, np.float64)
    label = rng.integers(0, k, size=n)
    prob = prob.astype(dtype)
    sub = np.finfo(dtype).smallest_subnormal * 3
    for row, kind in ((0, "zero"),) if n == 1 else ((1, "zero"), (2, "onehot"), (3, "subnormal")):
        if kind == "zero":
            prob[row, row % k] = 0.0
        elif kind == "onehot":
            prob[row] = 0.0
            prob[row, 1] = 1.0
            label[row] = 1
        else:
            prob[row, 0] = sub
    if n > 6:
        prob[4] = 1.0 / k
        label[5], label[6] = np.argmax(prob[5]), np.argmin(prob[6])
    return prob, label


def fit_rows(X, y, w, T=np.float64):
    """(row terms (n, 1 + km + km km), unclipped rows): per row the loss -log clip(s_y, eps, 1 - eps), its gradient (s - onehot) x^T and
    Hessian (diag(s) - s s^T) (x) x x^T w.r.t. the (k, k + 1) weights, the last two zero where the clip is active (eval_ref.fit_row_terms
    before its sums), evaluated in numpy type T from float64 features"""
    X, w = X.astype(T), np.asarray(w).astype(T)
    n, m = X.shape
    k = w.shape[0]
    km = k * m
    z = (X[:, None, :] * w[None, :, :]).sum(axis=2)
    z = z - z.max(axis=1, keepdims=True)
    s = np.exp(z)
    s = s / s.sum(axis=1, keepdims=True)
    eps = T(EPS64)
    ar = np.arange(n)
    sy = s[ar, y]
    live = (sy >= eps) & (sy <= T(1) - eps)
    loss = -np.log(np.clip(sy, eps, T(1) - eps))
    r = s.copy()
    r[ar, y] -= T(1)
    r[~live] = 0
    g = (r[:, :, None] * X[:, None, :]).reshape(n, km)
    sl = s * live[:, None]
    a = -sl[:, :, None] * sl[:, None, :]
    a[:, np.arange(k), np.arange(k)] += sl
    h = (a[:, :, None, :, None] * X[:, None, :, None, None]) * X[:, None, None, None, :]
    return np.concatenate([loss[:, None], g, h.reshape(n, km * km)], axis=1), live, sy


def fit_reference(prob, label, w, reps=1, tail=0):
    """dict(want, bound, ref_err, status, clipped, rows) of the sums of mural_eval_dirichlet_fit_terms over `reps` copies of the rows and
    the first `tail` of them once more.  want: eval_ref.fit_row_terms (a mean) times its row count.  bound, per entry of `out`:
    max(8 sum_rows |float64 term - longdouble term|, 2 (n + 2) 2^-53 sum_rows |term|), the longdouble term being the whole reference in
    longdouble (for float64 input its logarithm too: the device's log and numpy's may differ in the last bit, and that is part of the
    float64 reference's own error); for float32 input + sum_rows sum_features of the larger change of the term with that one log feature a
    float32 ulp up or a float32 ulp down (the device logf and numpy's may differ in the last bit of any feature, in either direction:
    moving all features the same way would cancel in every difference of logits).
    To that, the distance of eval_ref's own float64 number from the longdouble sum is added.
    ref_err: the restated float64 sum's distance from the longdouble sum."""
    prob = np.ascontiguousarray(prob)
    label = np.asarray(label, np.int64)
    k = prob.shape[1]
    ok = (label >= 0) & (label < k)
    p, y = prob[ok], label[ok]
    assert tail == 0 or ok.all()
    X = fit_features(p)
    t64, live, sy = fit_rows(X, y, w)
    moved = np.zeros_like(t64)
    if prob.dtype == np.float32:
        # the float32 logs are the float64 part's exact input; what a last-bit difference of each does is added feature by feature
        Xld = X
        x32 = X[:, :k].astype(np.float32)
        assert np.array_equal(x32.astype(np.float64), X[:, :k])
        for c in range(k):
            worse = np.zeros_like(t64)
            for to in (np.float32(np.inf), np.float32(-np.inf)):
                Xm = X.copy()
                Xm[:, c] = np.nextafter(x32[:, c], to).astype(np.float64)
                worse = np.maximum(worse, np.abs(fit_rows(Xm, y, w)[0] - t64))
            moved += worse
    else:
        # the reference in longdouble takes its logarithm in longdouble too (the clip stays the input's)
        tiny = np.finfo(np.float64).tiny
        Xld = np.hstack((np.log(np.clip(p, tiny, 1.0 - tiny).astype(np.longdouble)), np.ones((len(p), 1), np.longdouble)))
    tld, _, _ = fit_rows(Xld, y, w, np.longdouble)
    dist = np.abs(t64 - tld).astype(np.float64)
    dist_same_log = dist if Xld is X else np.abs(t64 - fit_rows(X, y, w, np.longdouble)[0]).astype(np.float64)
    mag = np.abs(t64)

    def total(rows):
        return reps * rows.sum(axis=0) + rows[:tail].sum(axis=0)

    def ref_sum(X_, y_):
        if not len(y_):
            return np.zeros(t64.shape[1])
        loss, g, h = eval_ref.fit_row_terms(X_, y_, np.asarray(w, np.float64), True)
        return np.concatenate([[loss], g, h.ravel()]) * len(y_)

    n = reps * len(y) + tail
    want = reps * ref_sum(X, y) + (ref_sum(X[:tail], y[:tail]) if tail else 0.0)
    truth = reps * tld.sum(axis=0) + tld[:tail].sum(axis=0)
    # eval_ref forms its logits and sums by matrix products (fused multiply-adds, blocked sums): a float64 evaluation of its own, whose
    # distance from the longdouble sums is no error of the kernel's.  The rule above bounds |kernel - longdouble|; `want` is eval_ref's
    # number, so its own distance is added (the triangle inequality)
    own = np.abs(want - truth).astype(np.float64)
    bound = np.maximum(8.0 * total(dist), any_order_bound(n, total(mag))) + total(moved) + own
    ref_err = np.abs(total(t64) - truth).astype(np.float64)
    return dict(want=want, bound=bound, ref_err=ref_err, status=0 if ok.all() else 2, live=live, sy=sy, rows=n, own_sum=total(t64), mag=total(mag),
                own=own, main=np.maximum(8.0 * total(dist), any_order_bound(n, total(mag))),
                main_same_log=np.maximum(8.0 * total(dist_same_log), any_order_bound(n, total(mag))))


def fit_layout(n):
    """(base rows, reps, tail): the long case repeats a base of FIT_LONG_BASE rows, so its reference is computed on the base alone"""
    if n == FIT_LONG_ROWS:
        reps, tail = divmod(n, FIT_LONG_BASE)
        return FIT_LONG_BASE, reps, tail
    return n, 1, 0


@functools.lru_cache(maxsize=None)
def fit_case(dtype, k, kind, n):
    """(prob, label, weights, reps, tail, reference) of one case; the reference is computed once and shared"""
    base, reps, tail = fit_layout(n)
    prob, label = fit_probs(base, k, dtype, 11)
    w = fit_weights(kind, k)
    # a row whose s_y lies within 1 % of eps could have its clip switched by a last-bit difference of a float32 log feature (the host
    # test derives the 1 %): such rows are drawn again
    rng = np.random.default_rng([k, FIT_WEIGHTS.index(kind), base, 5])
    for _ in range(8):
        sy = fit_rows(fit_features(prob), label, w)[2]
        edge = np.flatnonzero((sy > EPS64 / 1.01) & (sy < EPS64 * 1.01))
        if not len(edge):
            break
        prob[edge] = _dirichlet(rng, len(edge), k, np.float64).astype(prob.dtype)
    return prob, label, w, reps, tail, fit_reference(prob, label, w, reps, tail)
