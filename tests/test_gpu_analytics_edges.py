"""The five evaluation reductions (csrc/analytics.hip) one by one through their C entries, at the sizes and inputs where their code
changes course, against numpy restatements and float64 / longdouble references built on the CPU by tests/_analytics_edges_data.py
(tests/test_analytics_edges_host.py checks those inputs first).  Key outputs hold a sentinel and status words 0 before every call, and
every status is read back.

Tolerances (derived in the data module, never tuned): bit equality for keys, row counts, label counts, hits and for every sum of
probabilities that are multiples of 2^-20; the any-order bound 2 (m + 2) 2^-53 sum|p| for float64 atomic sums of Dirichlet rows; 8 x the
distance between the reference one precision down and one precision up, row by row, for everything behind a log or an exp."""
import math

import numpy as np
import pytest
import torch

from mural_amd import _lib
from tests import _analytics_edges_data as D
from tests._parity import NAN, _Stats

pytestmark = pytest.mark.gpu
GUARD = 64
TAG = "analytics"


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _status():
    return torch.zeros(1, dtype=torch.int32, device="cuda")


def _vec_check(got, want, bound, ref_err, what, case, stats):
    """|got - want| <= bound element by element; the element nearest its bound goes into the table"""
    got, want, bound = np.asarray(got, np.float64).ravel(), np.asarray(want, np.float64).ravel(), np.asarray(bound, np.float64).ravel()
    if not got.size:
        return
    err = np.abs(got - want)
    with np.errstate(divide="ignore", invalid="ignore"):
        ratio = np.where(bound > 0, err / bound, np.where(err == 0, 0.0, math.inf))
    worst = int(np.argmax(np.nan_to_num(ratio, nan=math.inf)))
    stats.add(what, None if ref_err is None else float(np.asarray(ref_err).ravel()[worst]), float(err[worst]), float(bound[worst]), case)
    ok = err <= bound
    assert bool(ok.all()), f"{what} at {case}: {int((~ok).sum())} of {err.size} beyond their bound, worst {err[worst]:.3e} > {bound[worst]:.3e}"


def _exact_check(got, want, what, case, stats):
    got, want = np.asarray(got), np.asarray(want)
    diff = int((got != want).sum())
    stats.add(what, None, float(diff), 0.0, case)
    assert diff == 0, f"{what} at {case}: {diff} of {got.size} differ, first at {np.argwhere(got != want)[0].tolist()}"


# ================================================================================================================== key kernels
def _kmer(codes, left0, right0, d, region_size=0, n_regions=0, status0=0):
    n, ncols = codes.shape
    dc = _dev(codes)
    keys = torch.full((n + GUARD,), D.KEY_SENTINEL, dtype=torch.int32, device="cuda")
    status = _status() + status0
    rc = _lib.lib().mural_eval_kmer_keys(dc.data_ptr(), n, ncols, left0, right0, d, region_size, n_regions, keys.data_ptr(), status.data_ptr(),
                                         None)
    torch.cuda.synchronize()
    keys = keys.cpu().numpy()
    assert (keys[n:] == D.KEY_SENTINEL).all()
    return rc, keys[:n], int(status.item())


@pytest.mark.parametrize("d", [1, 2, 3, 4, 5, 6])
def test_kmer_keys_equal_numpy(d):
    """d flanking codes a side on 2d and 2d + 3 columns (flanks from column 0 and up to the last column; the other columns hold values a
    flank would refuse), every row count, without regions and with regions of 100 rows (n is no multiple, and at d = 5 and 6 the 31 bits
    hold fewer regions than the rows fill: the rows past the last region get -1 and status stays 0)"""
    stats = _Stats(f"kmer d{d}", tag=TAG)
    for name, ncols, left0, right0 in D.kmer_layouts(d):
        for n in D.KMER_ROWS:
            codes = D.kmer_codes(n, ncols, left0, right0, d, 10 * d + n)
            for region_size, n_regions in ((0, 0), (100, D.kmer_regions(n, d))):
                case = f"d{d} {name} n{n} region {region_size}x{n_regions}"
                want, _ = D.kmer_keys_ref(codes, left0, right0, d, region_size, n_regions)
                rc, keys, status = _kmer(codes, left0, right0, d, region_size, n_regions)
                assert rc == 0 and status == 0, case
                _exact_check(keys, want, "keys", case, stats)
                if region_size:
                    assert (keys[n_regions * 100:] == -1).all() and n % 100
    stats.show()


def test_kmer_keys_bad_codes_and_the_31_bit_table():
    """a code of 5, -1 and 2^40 (its low 32 bits are a valid code) in a flank column: key -1 for that row alone and status 1; 8 regions of
    5^12 groups (1 953 125 000 keys, just under 2^31) with the largest key in the last region"""
    stats = _Stats("kmer bad", tag=TAG)
    for d in (1, 3, 6):
        for name, ncols, left0, right0 in D.kmer_layouts(d):
            cols = D.flank_cols(left0, right0, d)
            codes = D.kmer_codes(257, ncols, left0, right0, d, d)
            clean, _ = D.kmer_keys_ref(codes, left0, right0, d)
            for bad in D.BAD_CODES:
                for row, col in ((0, cols[0]), (100, cols[d - 1]), (256, cols[-1])):
                    c2 = codes.copy()
                    c2[row, col] = bad
                    rc, keys, status = _kmer(c2, left0, right0, d)
                    case = f"d{d} {name} code {bad} at ({row}, {col})"
                    assert rc == 0 and status == 1 and keys[row] == -1, case
                    _exact_check(np.delete(keys, row), np.delete(clean, row), "other keys", case, stats)
    n = 65537
    codes = D.kmer_codes(n, 12, 0, 6, 6, 99)
    codes[7 * 8192 + 5] = 4
    want, _ = D.kmer_keys_ref(codes, 0, 6, 6, 8192, 8)
    assert want[7 * 8192 + 5] == 8 * 5 ** 12 - 1 and want[-1] == -1
    rc, keys, status = _kmer(codes, 0, 6, 6, 8192, 8)
    assert rc == 0 and status == 0
    _exact_check(keys, want, "keys", "d6 8 regions x 5^12", stats)
    stats.show()


def _window(chrom, start, window, base, n_chrom):
    n = len(chrom)
    keys = torch.full((n + GUARD,), D.KEY_SENTINEL, dtype=torch.int32, device="cuda")
    status = _status()
    dc, ds, db = _dev(chrom), _dev(start), _dev(base)
    rc = _lib.lib().mural_eval_window_keys(dc.data_ptr(), ds.data_ptr(), n, window, db.data_ptr(), n_chrom, keys.data_ptr(), status.data_ptr(),
                                           None)
    torch.cuda.synchronize()
    keys = keys.cpu().numpy()
    assert (keys[n:] == D.KEY_SENTINEL).all()
    return rc, keys[:n], int(status.item())


def test_window_keys_equal_numpy():
    """windows of 1, 1000 and 10^12 (beyond every start), 1 and 25 chromosomes on a shuffled chrom_base, starts of 0, window - 1 and
    window among the rows; then a chromosome id of -1, one of n_chrom and a start of -1: key -1 and status 1, every other key intact"""
    stats = _Stats("window", tag=TAG)
    for window in (1, 1000, 10 ** 12):
        for n_chrom in (1, 25):
            for n in D.WINDOW_ROWS:
                case = f"window {window} n_chrom {n_chrom} n{n}"
                chrom, start, base = D.window_case(n, window, n_chrom, n)
                want, _ = D.window_keys_ref(chrom, start, window, base, n_chrom)
                rc, keys, status = _window(chrom, start, window, base, n_chrom)
                assert rc == 0 and status == 0, case
                _exact_check(keys, want, "keys", case, stats)
                for what, value in (("chrom", -1), ("chrom", n_chrom), ("start", -1)):
                    c2, s2 = chrom.copy(), start.copy()
                    (c2 if what == "chrom" else s2)[n // 2] = value
                    rc, keys, status = _window(c2, s2, window, base, n_chrom)
                    assert rc == 0 and status == 1 and keys[n // 2] == -1, (case, what, value)
                    _exact_check(np.delete(keys, n // 2), np.delete(want, n // 2), "other keys", f"{case} {what} {value}", stats)
    stats.show()


def test_key_entries_refuse_bad_arguments_and_leave_their_outputs():
    """d = 0 and 7, flank columns outside the row, window = 0, n_chrom = 0, a region table over 31 bits: a non-zero code, keys and status
    untouched; n = 0 with NULL pointers is OK"""
    lib = _lib.lib()
    codes = _dev(D.kmer_codes(300, 12, 0, 6, 6, 1))
    keys = torch.full((300,), D.KEY_SENTINEL, dtype=torch.int32, device="cuda")
    status = _status() + 4
    # (ncols, left0, right0, d, region_size, n_regions)
    for args in ((12, 0, 6, 0, 0, 0), (12, 0, 6, 7, 0, 0), (12, -1, 6, 6, 0, 0), (12, 1, 7, 6, 0, 0), (12, 7, 0, 6, 0, 0), (12, 0, 6, 6, 30, 9),
                 (12, 0, 6, 6, -1, 0), (0, 0, 0, 1, 0, 0)):
        ncols, left0, right0, d, region_size, n_regions = args
        rc = lib.mural_eval_kmer_keys(codes.data_ptr(), 300, ncols, left0, right0, d, region_size, n_regions, keys.data_ptr(), status.data_ptr(),
                                      None)
        assert rc != 0, args
        with pytest.raises(ValueError, match="kmer_keys"):
            _lib.check(rc)
    torch.cuda.synchronize()
    assert int(status.item()) == 4 and bool((keys == D.KEY_SENTINEL).all())
    assert lib.mural_eval_kmer_keys(codes.data_ptr(), 300, 12, 0, 6, 6, 30, 8, keys.data_ptr(), status.data_ptr(), None) == 0      # (8 fit)
    torch.cuda.synchronize()
    assert int(status.item()) == 4 and int(keys[299]) == -1 and int(keys[0]) >= 0
    keys.fill_(D.KEY_SENTINEL)
    chrom, start, base = (_dev(a) for a in D.window_case(300, 1000, 25, 1))
    for window, n_chrom in ((0, 25), (-5, 25), (1000, 0), (1000, -1)):
        rc = lib.mural_eval_window_keys(chrom.data_ptr(), start.data_ptr(), 300, window, base.data_ptr(), n_chrom, keys.data_ptr(),
                                        status.data_ptr(), None)
        assert rc != 0, (window, n_chrom)
        with pytest.raises(ValueError, match="window_keys"):
            _lib.check(rc)
    torch.cuda.synchronize()
    assert int(status.item()) == 4 and bool((keys == D.KEY_SENTINEL).all())
    assert lib.mural_eval_kmer_keys(None, 0, 12, 0, 6, 6, 0, 0, None, None, None) == 0
    assert lib.mural_eval_window_keys(None, None, 0, 1000, None, 25, None, None, None) == 0
    assert lib.mural_eval_kmer_keys(None, 300, 12, 0, 6, 6, 0, 0, keys.data_ptr(), status.data_ptr(), None) != 0
    torch.cuda.synchronize()
    assert int(status.item()) == 4 and bool((keys == D.KEY_SENTINEL).all())


# ================================================================================================================== group_obs_pred
def _group(keys, label, prob, nc, n_groups, table0=None):
    """the table (zeros, or table0, before the call) and the status after mural_eval_group_obs_pred"""
    n = len(keys)
    dk, dl, dp = _dev(np.asarray(keys, np.int32)), _dev(np.asarray(label, np.int32)), _dev(prob)
    table = torch.zeros((n_groups, 1 + 2 * nc), dtype=torch.float64, device="cuda") if table0 is None else _dev(table0)
    status = _status()
    rc = _lib.lib().mural_eval_group_obs_pred(dk.data_ptr(), dl.data_ptr(), dp.data_ptr(), int(prob.dtype == np.float64), n, nc, n_groups,
                                              table.data_ptr(), status.data_ptr(), None)
    assert rc == 0
    torch.cuda.synchronize()
    return table.cpu().numpy(), int(status.item())


def _group_all(keys, label, nc, n_groups, case, stats, seed, want_status=0):
    """the case with exact and with Dirichlet probabilities, in float32 and float64; returns the four tables"""
    out = []
    for kind in ("exact", "dirichlet"):
        p64, p32 = D.group_probs(len(keys), nc, kind, seed)
        for prob in (p32, p64):
            want, S, status = D.group_ref(keys, label, prob, nc, n_groups)
            got, got_status = _group(keys, label, prob, nc, n_groups)
            assert got_status == status == want_status, (case, got_status, status)
            _exact_check(got[:, :1 + nc], want[:, :1 + nc], "rows, label rows", f"{case} {kind} {prob.dtype}", stats)
            if kind == "exact":
                _exact_check(got[:, 1 + nc:], want[:, 1 + nc:], "2^-20 prob sums", f"{case} {prob.dtype}", stats)
            else:
                _vec_check(got[:, 1 + nc:], want[:, 1 + nc:], D.group_bound(want, S)[:, 1 + nc:], None, "prob sums", f"{case} {prob.dtype}", stats)
            out.append(got)
    return out


@pytest.mark.parametrize("nc", D.GROUP_CLASSES)
def test_group_obs_pred_on_each_accumulation_path(nc):
    """Every case in four forms (2^-20 and Dirichlet probabilities, float32 and float64), n_groups = 8 (LDS table) unless stated:
      * all keys equal, n = 1, 63 (per-lane rows only), 64 (one uniform wave, cnt = 64), 65 (one uniform wave + one row per lane), 256 (four
        uniform waves), 257, 2048 * 256 + 65 (8193 uniform waves over 257 workgroups, each thread eight rounds, 1 row per lane);
      * sorted keys in runs of 64, 96, 100 over 40 groups: uniform waves and waves that straddle two keys (per lane);
      * the same rows shuffled (per lane throughout): the same table, bit for bit where the sums are exact;
      * 256 equal keys with one hole (a key of -1 in lane 0 or mid-wave, a bad label, a key of n_groups): that wave falls to the per-lane
        path and counts 63 (host test: wave_paths == (3, 63))."""
    stats = _Stats(f"group nc{nc}", tag=TAG)
    for n in D.EQUAL_ROWS:
        keys, label = np.full(n, 5), np.arange(n) % nc
        for t in _group_all(keys, label, nc, 8, f"equal n{n}", stats, n):
            assert t[5, 0] == n and t[:, 0].sum() == n
    keys = D.run_keys(40)
    label = (np.arange(len(keys)) * 7 // 3) % nc
    tables = _group_all(keys, label, nc, 40, "runs 64/96/100", stats, 3)
    perm = np.random.default_rng(1).permutation(len(keys))
    shuffled = []
    for kind in ("exact", "dirichlet"):
        p64, p32 = D.group_probs(len(keys), nc, kind, 3)
        for prob in (p32, p64):
            got, status = _group(keys[perm], label[perm], prob[perm], nc, 40)
            assert status == 0
            shuffled.append(got)
    for i, (a, b) in enumerate(zip(tables, shuffled)):
        _exact_check(b[:, :1 + nc], a[:, :1 + nc], "shuffled: rows", "runs shuffled", stats)
        if i < 2:
            _exact_check(b, a, "shuffled: 2^-20", "runs shuffled", stats)
        else:
            S = np.abs(a)
            _vec_check(b[:, 1 + nc:], a[:, 1 + nc:], 2 * D.group_bound(a, S)[:, 1 + nc:], None, "shuffled: sums", "runs shuffled", stats)
    keys, label = np.full(256, 5), np.arange(256) % nc
    for at in (0, 70, 191):
        for hole_key, hole_label, st in ((-1, 0, 0), (-7, 0, 0), (5, -1, 2), (5, nc, 2), (8, 0, 2)):
            k2, l2 = keys.copy(), label.copy()
            k2[at], l2[at] = hole_key, hole_label
            for t in _group_all(k2, l2, nc, 8, f"hole at {at}: key {hole_key} label {hole_label}", stats, at, want_status=st):
                assert t[5, 0] == 255 and t[:, 0].sum() == 255
    stats.show()


@pytest.mark.parametrize("nc", D.GROUP_CLASSES)
def test_group_obs_pred_on_both_sides_of_the_lds_limit(nc):
    """n_groups = 4096 // (1 + 2 nc) (the last table privatised in LDS: 4095 cells at nc = 1, 4092 at nc = 16; 4096 itself cannot be reached
    with an odd row width) against one group more (global atomics): 20 000 rows over the groups both have, the last one among them, give
    the same group rows, and the extra group stays empty"""
    stats = _Stats(f"group lds nc{nc}", tag=TAG)
    lo, hi = D.lds_boundary_groups(nc)
    rng = np.random.default_rng(nc)
    n = 20000
    keys = rng.integers(0, lo, size=n)
    keys[:64] = lo - 1                                  # a uniform wave on the last group
    label = rng.integers(0, nc, size=n)
    a = _group_all(keys, label, nc, lo, f"{lo} groups (LDS)", stats, 5)
    b = _group_all(keys, label, nc, hi, f"{hi} groups (global)", stats, 5)
    for i, (ta, tb) in enumerate(zip(a, b)):
        assert not tb[lo].any()
        _exact_check(tb[:lo, :1 + nc], ta[:, :1 + nc], "LDS = global: rows", f"nc{nc}", stats)
        if i < 2:
            _exact_check(tb[:lo], ta, "LDS = global: 2^-20", f"nc{nc}", stats)
    # the group only the larger table has
    keys[100:200] = lo
    _group_all(keys, label, nc, hi, f"{hi} groups, the last one used", stats, 6)
    _group_all(keys, label, nc, lo, f"{lo} groups, a key of n_groups", stats, 6, want_status=2)
    stats.show()


@pytest.mark.parametrize("nc", D.GROUP_CLASSES)
def test_group_obs_pred_status_and_accumulation(nc):
    """keys of -1 and -7 are skipped with status 0; a key of n_groups, a label of -1 and a label of nc each set status 2 and only those rows
    are missing; two calls over the halves of the rows into one table, and a call into a table holding (cell index mod 97) / 4, add up to
    the one-call table (bit for bit with the 2^-20 probabilities)"""
    stats = _Stats(f"group += nc{nc}", tag=TAG)
    rng = np.random.default_rng(100 + nc)
    n, g = 3001, 11
    keys, label = rng.integers(0, g, size=n), rng.integers(0, nc, size=n)
    for rows, key, lab, st in (((3, 700, 2999), -1, None, 0), ((3, 700, 2999), -7, None, 0), ((4, 3000), g, None, 2), ((5,), None, -1, 2),
                               ((6, 2500), None, nc, 2)):
        k2, l2 = keys.copy(), label.copy()
        for r in rows:
            if key is not None:
                k2[r] = key
            if lab is not None:
                l2[r] = lab
        for t in _group_all(k2, l2, nc, g, f"rows {rows}: key {key} label {lab}", stats, 7, want_status=st):
            assert t[:, 0].sum() == n - len(rows)
    for kind in ("exact", "dirichlet"):
        p64, p32 = D.group_probs(n, nc, kind, 8)
        for prob in (p32, p64):
            want, S, _ = D.group_ref(keys, label, prob, nc, g)
            h = n // 2
            first, st1 = _group(keys[:h], label[:h], prob[:h], nc, g)
            both, st2 = _group(keys[h:], label[h:], prob[h:], nc, g, table0=first)
            fill = (np.arange(g * (1 + 2 * nc)) % 97).reshape(g, -1) / 4.0
            filled, st3 = _group(keys, label, prob, nc, g, table0=fill)
            assert st1 == st2 == st3 == 0
            case = f"{kind} {prob.dtype}"
            _exact_check(both[:, :1 + nc], want[:, :1 + nc], "two calls: rows", case, stats)
            _exact_check(filled[:, :1 + nc], (want + fill)[:, :1 + nc], "pre-filled: rows", case, stats)
            if kind == "exact":
                _exact_check(both, want, "two calls: 2^-20", case, stats)
                _exact_check(filled, want + fill, "pre-filled: 2^-20", case, stats)
            else:
                bound = D.group_bound(want, S)
                _vec_check(both[:, 1 + nc:], want[:, 1 + nc:], bound[:, 1 + nc:], None, "two calls: sums", case, stats)
                _vec_check(filled[:, 1 + nc:], (want + fill)[:, 1 + nc:], D.group_bound(want + 1.0, S + fill)[:, 1 + nc:], None, "pre-filled: sums",
                           case, stats)
    stats.show()


def test_group_obs_pred_beyond_one_round_of_its_grid():
    """2048 * 2048 + 300 rows of one class in float32, 1000 groups: the grid is capped at 2048 workgroups of 2048 rows, so 300 rows belong to
    a second round.  Keys and 2^-20 probabilities come from an integer formula evaluated on the device and, the same, by numpy: the table is
    np.bincount's bit for bit"""
    stats = _Stats("group long", tag=TAG)
    n = D.BIG_GROUP_ROWS
    k, lab, num = D.big_group_formula(torch.arange(n, dtype=torch.int64, device="cuda"))
    keys, label = k.to(torch.int32), lab.to(torch.int32)
    prob = (num.to(torch.float32) / 1048576.0).reshape(n, 1).contiguous()
    table = torch.zeros((D.BIG_GROUPS, 3), dtype=torch.float64, device="cuda")
    status = _status()
    _lib.check(_lib.lib().mural_eval_group_obs_pred(keys.data_ptr(), label.data_ptr(), prob.data_ptr(), 0, n, 1, D.BIG_GROUPS, table.data_ptr(),
                                                    status.data_ptr(), None))
    torch.cuda.synchronize()
    kn, labn, numn = D.big_group_formula(np.arange(n, dtype=np.int64))
    want, _, st = D.group_ref(kn, labn, (numn.astype(np.float32) / np.float32(1048576.0)).reshape(n, 1), 1, D.BIG_GROUPS)
    assert int(status.item()) == st == 0 and want[:, 0].sum() == n
    _exact_check(table.cpu().numpy(), want, "table", f"n{n}", stats)
    stats.show()


# ================================================================================================================== calib_metrics
def _calib(prob, label, nc, nb, out0=None, n=None):
    """(return code, out, status); prob / label numpy arrays or device tensors"""
    dp = prob if torch.is_tensor(prob) else _dev(prob)
    dl = label if torch.is_tensor(label) else _dev(np.asarray(label, np.int32))
    n = dp.shape[0] if n is None else n
    bounds = D.calib_bounds(nb).cuda()
    out = torch.zeros(D.calib_cells(nc, nb), dtype=torch.float64, device="cuda") if out0 is None else _dev(out0)
    status = _status()
    rc = _lib.lib().mural_eval_calib_metrics(dp.data_ptr(), int(dp.dtype == torch.float64), dl.data_ptr(), n, nc, nb, bounds.data_ptr(),
                                             out.data_ptr(), status.data_ptr(), None)
    torch.cuda.synchronize()
    return rc, out.cpu().numpy(), int(status.item())


def _calib_check(out, ref, case, stats, pre=""):
    want, bound, ref_err, exact = ref["want"], ref["bound"], ref["ref_err"], ref["exact"]
    _exact_check(out[exact], want[exact], pre + "rows, hits", case, stats)
    sums = ~exact
    sums[:2] = False
    _vec_check(out[sums], want[sums], bound[sums], ref_err[sums], pre + "score sums", case, stats)
    for at, what in ((0, "nll"), (1, "brier")):
        if math.isinf(want[at]):
            assert out[at] == want[at], f"{what} at {case}: {out[at]!r}, not {want[at]!r}"
        else:
            _vec_check(out[at:at + 1], want[at:at + 1], bound[at:at + 1], ref_err[at:at + 1], pre + what, case, stats)


@pytest.mark.parametrize("nc", D.CALIB_CLASSES)
@pytest.mark.parametrize("dtype", ["float32", "float64"])
def test_calib_metrics_every_cell_against_the_next_precision(dtype, nc):
    """The whole `out` vector for every n_bins x row count, Dirichlet(0.7) rows (at 257 rows also scaled by 0.5 and by 3: the softmax
    renormalises them), rows near a bin bound left out as the data module states.  Row and hit counts exactly; score sums, NLL and Brier
    within their rows' added-up bounds."""
    stats = _Stats(f"calib {dtype[5:]} nc{nc}", tag=TAG)
    for nb in D.CALIB_BINS:
        for n in D.CALIB_ROWS:
            for scale in (1.0,) if n != 257 else (1.0, 0.5, 3.0):
                case = f"nc{nc} nb{nb} n{n}" + (f" x{scale:g}" if scale != 1 else "")
                prob, label, _ = D.calib_case(dtype, nc, nb, n, scale)
                rc, out, status = _calib(prob, label, nc, nb)
                assert rc == 0 and status == 0, case
                _calib_check(out, D.calib_reference(prob, label, nb), case, stats)
    stats.show()


@pytest.mark.parametrize("dtype", ["float32", "float64"])
def test_calib_metrics_scores_that_are_exact(dtype):
    """Uniform rows of 2, 4, 8, 16 classes at 80 bins and of 2 classes at 50: the score 1 / k IS a float32 bound and belongs to the bin
    below it.  One-hot rows: the score 1 goes in the last bin, the scores 0 in none, and the NLL of a label on a zero class is +inf (the
    assertion is on inf).  One class: every score is 1."""
    stats = _Stats(f"calib exact {dtype[5:]}", tag=TAG)
    for nc, nb in ((2, 80), (4, 80), (8, 80), (16, 80), (2, 50)):
        prob, label = D.calib_exact_case("uniform", nc, dtype)
        rc, out, status = _calib(prob, label, nc, nb)
        assert rc == 0 and status == 0
        bins = out[2:].reshape(1 + nc, nb, 3)
        assert (bins[:, nb // nc - 1, 0] == 70).all() and bins[:, :, 0].sum() == 70 * (1 + nc), (nc, nb)
        assert (bins[:, nb // nc - 1, 1] == 70.0 / nc).all()
        _calib_check(out, D.calib_reference(prob, label, nb), f"uniform nc{nc} nb{nb}", stats)
    for nc in (2, 3, 4, 8, 16):
        for nb in (1, 15, 80):
            prob, label = D.calib_exact_case("onehot", nc, dtype)
            rc, out, status = _calib(prob, label, nc, nb)
            assert rc == 0 and status == 0
            assert out[0] == math.inf and out[2:].reshape(1 + nc, nb, 3)[:, :nb - 1].sum() == 0
            _calib_check(out, D.calib_reference(prob, label, nb), f"one-hot nc{nc} nb{nb}", stats)
        # labels on the hot class only: a finite NLL of exactly 0
        label = (np.arange(70) // 2) % nc
        rc, out, status = _calib(prob, label, nc, 15)
        assert rc == 0 and status == 0 and out[0] == 0 and out[1] == 0
        _calib_check(out, D.calib_reference(prob, label, 15), f"one-hot nc{nc}, labels on the 1", stats)
    for nb in D.CALIB_BINS:
        prob, label = D.calib_exact_case("single", 1, dtype)
        rc, out, status = _calib(prob, label, 1, nb)
        assert rc == 0 and status == 0
        _calib_check(out, D.calib_reference(prob, label, nb), f"one class nb{nb}", stats)
        assert out[0] == 0 and out[1] == 0 and out[2 + 3 * (nb - 1)] == 70 and out[2 + 3 * (2 * nb - 1) + 1] == 70
    stats.show()


@pytest.mark.parametrize("dtype", ["float32", "float64"])
def test_calib_metrics_status_accumulation_and_refusals(dtype):
    """a label of -1 and a label of n_class set status 2 and their rows are in no cell and in neither sum; two calls over the halves and a
    call into a vector holding 3.0 per cell add up; 81 bins of 16 classes (4133 cells), 0 and 17 classes are refused before any launch."""
    stats = _Stats(f"calib += {dtype[5:]}", tag=TAG)
    for nc, nb, n in ((3, 15, 257), (16, 80, 4099), (1, 2, 256)):
        prob, label, _ = D.calib_case(dtype, nc, nb, n)
        case = f"nc{nc} nb{nb} n{n}"
        bad = label.copy()
        bad[[0, n // 2, n - 1]] = (-1, nc, nc + 5)
        rc, out, status = _calib(prob, bad, nc, nb)
        ref = D.calib_reference(prob, bad, nb)
        assert rc == 0 and status == ref["status"] == 2 and ref["rows"] == n - 3
        _calib_check(out, ref, case + " bad labels", stats)
        assert out[2:2 + 3 * nb:3].sum() == n - 3
        ref = D.calib_reference(prob, label, nb)
        h = n // 2
        rc, first, st1 = _calib(prob[:h], label[:h], nc, nb)
        rc2, both, st2 = _calib(prob[h:], label[h:], nc, nb, out0=first)
        assert rc == rc2 == 0 and st1 == st2 == 0
        _calib_check(both, ref, case, stats, pre="two calls: ")
        rc, filled, st = _calib(prob, label, nc, nb, out0=np.full(D.calib_cells(nc, nb), 3.0))
        assert rc == 0 and st == 0
        shifted = dict(ref, want=ref["want"] + 3.0, bound=ref["bound"] + np.where(ref["exact"], 0.0, D.any_order_bound(1, 3.0 + np.abs(ref["want"]))))
        _calib_check(filled, shifted, case, stats, pre="pre-filled: ")
    prob, label, _ = D.calib_case(dtype, 16, 80, 257)
    sentinel = np.full(D.calib_cells(16, 81), 7.25)
    for nc, nb in ((16, 81), (0, 15), (17, 15), (16, 0)):
        rc, out, status = _calib(prob, label, nc, nb, out0=sentinel)
        assert rc != 0 and status == 0 and (out == 7.25).all(), (nc, nb)
        with pytest.raises(ValueError, match="calib_metrics"):
            _lib.check(rc)
    rc, out, status = _calib(prob, label, 16, 80)
    assert rc == 0 and status == 0
    assert _lib.lib().mural_eval_calib_metrics(None, 0, None, 0, 16, 80, None, None, None, None) == 0
    stats.show()


def test_calib_metrics_beyond_one_round_of_its_grid():
    """1024 * 2048 + 129 rows of 2 classes, 2 bins, float32: 129 rows belong to a second round of the capped grid.  Rows (m, 1024 - m) /
    1024 from an integer formula evaluated on the device and by numpy; m != 512, so no score is within 1 / 1024 of a bound"""
    stats = _Stats("calib long", tag=TAG)
    n = D.BIG_CALIB_ROWS
    m, lab = D.big_calib_formula(torch.arange(n, dtype=torch.int64, device="cuda"))
    prob = (torch.stack([m, 1024 - m], dim=1).to(torch.float32) / 1024.0).contiguous()
    rc, out, status = _calib(prob, lab.to(torch.int32), 2, 2)
    assert rc == 0 and status == 0
    mn, labn = D.big_calib_formula(np.arange(n, dtype=np.int64))
    probn = np.stack([mn, 1024 - mn], axis=1).astype(np.float32) / np.float32(1024)
    ref = D.calib_reference(probn, labn, 2)
    assert ref["want"][2::3].sum() == 3 * n
    _calib_check(out, ref, f"n{n}", stats)
    stats.show()


# ================================================================================================================== dirichlet_fit_terms
HESS_FILL = 7.25


def _fit(prob, label, k, w, need, reps=1, tail=0, out0=None):
    """(return code, out, status) over `reps` copies of the rows and the first `tail` once more (repeated on the device)"""
    dp, dl = _dev(prob), _dev(np.asarray(label, np.int32))
    if reps != 1 or tail:
        dp, dl = torch.cat([dp.repeat(reps, 1), dp[:tail]]).contiguous(), torch.cat([dl.repeat(reps), dl[:tail]]).contiguous()
    n = dp.shape[0]
    km = k * (k + 1)
    if out0 is None:
        out0 = np.zeros(1 + km + km * km)
        if not need:
            out0[1 + km:] = HESS_FILL
    out, dw, status = _dev(out0), _dev(np.asarray(w, np.float64)), _status()
    rc = _lib.lib().mural_eval_dirichlet_fit_terms(dp.data_ptr(), int(dp.dtype == torch.float64), dl.data_ptr(), n, k, dw.data_ptr(), int(need),
                                                   out.data_ptr(), status.data_ptr(), None)
    torch.cuda.synchronize()
    return rc, out.cpu().numpy(), int(status.item())


def _fit_check(out, ref, k, need, case, stats, pre=""):
    km = k * (k + 1)
    want, bound, ref_err = ref["want"], ref["bound"], ref["ref_err"]
    _vec_check(out[:1], want[:1], bound[:1], ref_err[:1], pre + "loss", case, stats)
    _vec_check(out[1:1 + km], want[1:1 + km], bound[1:1 + km], ref_err[1:1 + km], pre + "gradient", case, stats)
    if need:
        _vec_check(out[1 + km:], want[1 + km:], bound[1 + km:], ref_err[1 + km:], pre + "hessian", case, stats)
    else:
        assert (out[1 + km:] == HESS_FILL).all(), f"{case}: need_hessian = 0 wrote into the Hessian block"


@pytest.mark.parametrize("kind", D.FIT_WEIGHTS)
@pytest.mark.parametrize("k", D.FIT_CLASSES)
@pytest.mark.parametrize("dtype", ["float32", "float64"])
def test_dirichlet_fit_terms_against_float64(dtype, k, kind):
    """Loss, gradient and Hessian sums for every row count (1, around the 128-row tile, 1000, and 512 * 512 + 129: 129 rows into a second
    round of the capped grid, a base of 257 rows repeated) under the identity, a perturbed identity and weights of magnitude 40 (rows with
    s_y below eps and above 1 - eps, whose gradient and Hessian terms vanish, next to unclipped rows), with need_hessian 1 and 0.  Rows
    with an exact 0, an exact 1 and a subnormal are among the probabilities.  need_hessian = 0 leaves the Hessian block as it was and gives
    the same loss and gradient (the same bits while one workgroup does all the rows)."""
    stats = _Stats(f"fit {dtype[5:]} k{k}", tag=TAG)
    km = k * (k + 1)
    for n in D.FIT_ROWS:
        prob, label, w, reps, tail, ref = D.fit_case(dtype, k, kind, n)
        case = f"k{k} {kind} n{n}"
        rc, full, status = _fit(prob, label, k, w, 1, reps, tail)
        assert rc == 0 and status == 0, case
        _fit_check(full, ref, k, 1, case, stats)
        rc, lean, status = _fit(prob, label, k, w, 0, reps, tail)
        assert rc == 0 and status == 0, case
        _fit_check(lean, ref, k, 0, case, stats, pre="no hessian: ")
        if n <= 512:
            assert np.array_equal(lean[:1 + km], full[:1 + km]), case
    stats.show()


@pytest.mark.parametrize("dtype", ["float32", "float64"])
def test_dirichlet_fit_terms_status_accumulation_and_refusals(dtype):
    """a label of -1 and a label of k set status 2 and their rows are skipped; two calls over the halves add up to the one-call sums;
    k = 1 and k = 9 are refused before any launch"""
    stats = _Stats(f"fit += {dtype[5:]}", tag=TAG)
    for k in (2, 5, 8):
        prob, label, w, _, _, ref = D.fit_case(dtype, k, "perturbed", 1000)
        case = f"k{k} n1000"
        bad = label.copy()
        bad[[0, 127, 128, 999]] = (-1, k, k + 3, -2)
        rc, out, status = _fit(prob, bad, k, w, 1)
        bad_ref = D.fit_reference(prob, bad, w)
        assert rc == 0 and status == bad_ref["status"] == 2 and bad_ref["rows"] == 996
        _fit_check(out, bad_ref, k, 1, case + " bad labels", stats)
        rc, first, st1 = _fit(prob[:500], label[:500], k, w, 1)
        rc2, both, st2 = _fit(prob[500:], label[500:], k, w, 1, out0=first)
        assert rc == rc2 == 0 and st1 == st2 == 0
        _fit_check(both, ref, k, 1, case, stats, pre="two calls: ")
    prob, label, w, _, _, _ = D.fit_case(dtype, 8, "perturbed", 129)
    out0 = np.full(1 + 90 + 90 * 90, NAN)
    for k in (1, 9, 0):
        rc, out, status = _fit(prob, label, k, np.zeros((9, 10)), 1, out0=out0)
        assert rc != 0 and status == 0 and np.isnan(out).all(), k
        with pytest.raises(ValueError, match="dirichlet_fit_terms"):
            _lib.check(rc)
    assert _lib.lib().mural_eval_dirichlet_fit_terms(None, 0, None, 0, 4, None, 1, None, None, None) == 0
    stats.show()
