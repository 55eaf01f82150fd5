"""The fused local branch (csrc/snv_local_train.h) and the fused tower head (csrc/snv_head_train.h) of the composed SNV training step
on their own, through mural_debug_local_train_fwd / _bwd and mural_debug_head_train_fwd / _bwd, with dropout ON.

Every launch is judged against a float64 evaluation of ITS operation on the inputs it read: the reference of the next launch starts
from the tensors the device saved (xt, lin, state, dd, g, feat, arg, fd), so a ReLU mask or an arg-max is an exact function of
float32 values both sides see.  Dropout masks come from mural_op_dropout on a tensor of ones with the same p and seed (its own test:
test_dropout_values_mask_and_keep_rate).  Outputs are NaN before every call, the BatchNorm accumulators zero.

Tolerances are the two rules of tests/_parity.py or exact equality:
  * exact: xt[0] (gather x keep scale), arg, feat, and the zeros every dropout, every ReLU mask in g and the arg-max / ReLU mask of the
    head's dx must put (a kept element may be 0 by itself: at B = 2 a BatchNorm's backward cancels to 0; its value has its own check);
  * ``_sum_check`` with n = the reduction length: lin / logits (n = K, S includes |bias|), the Linear behind dd and dx (n = O: the
    multiplication by the keep scale is the "final rounding" of the rule), dW and db (n = B);
  * dE: see ``_check_dE``;
  * ``_loose``: state, running statistics, xt[1], xt[2], fd, g, dgamma, dbeta, the head's dx values."""
import ctypes as C

import numpy as np
import pytest
import torch

from mural_amd import _lib
from mural_amd.model import train_ops as T
from tests._parity import EPS, MOMENTUM, NAN, _Stats, _loose, _sum_check

pytestmark = pytest.mark.gpu

F64 = torch.float64
EPS32 = float(np.float32(EPS))              # what the kernels get: the float nearest 1e-5
FWD_Q, BWD_Q = (19, 24, 38, 64), (2, 19, 38, 64)      # the reduction runs lt_launch_fwd / lt_launch_bwd instantiate
DROP, DROP_OFF, DROP_HALF = (0.1, 0.1, 0.25), (0.0, 0.0, 0.0), (0.5, 0.5, 0.5)
SEEDS = (0x1234567890ABCDEF, 0x0FEDCBA987654321, 0x00C0FFEE12345678)

# (cols, emb_rows, h1, h2, nc, batches, dropout rates): in1 = 5 cols.  Between them (test_local_shapes_cover_...):
#   forward K on both sides of 76 | 96 | 152 (in1 5 75 80 95 100 150 155 255; h 76 77 96 97 152 153 256), K % 4 != 0 and tiny (1 3 9 75 130),
#   backward O on both sides of 8 | 76 | 152 (nc 1 8 9 16; h 8 9 76 77 152 153 256), output widths 1 15 16 17 64 65,
#   tables of 5 / 65 / 1025 rows (the last with h1 = 256: the bottom launch's largest LDS image);
#   batches: 513 = a ragged second 32-row pass of lt_wgrad_kernel's waves, 529 = 16 x 33 + 1 wraps the accumulator slots
LOCAL_CASES = [
    (1, 5, 1, 3, 1, (2, 17), DROP),
    (15, 65, 8, 9, 8, (15, 513), DROP),
    (16, 65, 9, 8, 9, (16, 37), DROP),
    (19, 65, 76, 77, 16, (2, 529), DROP),
    (20, 65, 77, 76, 1, (17, 513), DROP_OFF),
    (30, 5, 96, 97, 8, (15, 37), DROP),
    (31, 65, 97, 96, 9, (16, 529), DROP),
    (51, 1025, 256, 152, 16, (37, 1100), DROP),
    (19, 65, 152, 153, 9, (2, 513), DROP),
    (16, 5, 153, 256, 8, (17, 1100), DROP),
    (1, 65, 15, 16, 16, (15, 529), DROP),
    (15, 5, 17, 64, 1, (16, 37), DROP_HALF),
    (20, 65, 65, 130, 9, (2, 513), DROP),
    (31, 5, 75, 15, 8, (17, 37), DROP),
    (30, 65, 130, 17, 16, (15, 1100), DROP),
    (51, 65, 64, 65, 1, (16, 529), DROP),
]

HEAD_C = 32
# rows one round of each capped head launch covers (csrc/snv_head_train.h: head_train_fwd / head_train_bwd)
HEAD_CAPS = {"hd_gmax_stats_kernel": 1024 * 32, "hd_bn_drop_fc_kernel": 2048 * 8, "hd_bwd1_kernel": 2048 * 8, "hd_bwd2_kernel": 2048 * 32}
HEAD_SMALL = [(2, 1, 1), (2, 67, 5), (7, 2, 2), (7, 1, 16), (8, 7, 4), (8, 2, 1), (9, 67, 5), (9, 7, 2), (31, 1, 16), (31, 67, 4),
              (32, 2, 1), (32, 7, 5), (33, 7, 2), (33, 1, 4), (257, 67, 16), (257, 2, 5)]           # (B, L, nc)
HEAD_BIG = [(16384, 1, 4), (16385, 2, 5), (16392, 1, 16), (32768, 2, 1), (32769, 1, 2), (65536, 1, 5), (65537, 2, 4)]


def _nan(shape, dtype=torch.float32):
    return torch.full(shape, NAN, dtype=dtype, device="cuda")


def _bits(t):
    return t.detach().cpu().contiguous().view(torch.int32)


def _pp(tensors):
    """a host array of device pointers"""
    return (C.c_void_p * len(tensors))(*[t.data_ptr() for t in tensors])


def _ptr(t):
    return None if t is None else t.data_ptr()


def _acc(n):
    return torch.zeros((T.BN_SLOTS, 2, n), dtype=F64, device="cuda")


def _keep(shape, p, seed):
    """the float32 factor (1 / (1 - p) or 0) mural_op_dropout's draw gives each element of a tensor of this shape"""
    ones = torch.ones(shape, device="cuda")
    if p == 0:
        return ones.cpu()
    y = _nan(shape)
    _lib.check(_lib.lib().mural_op_dropout(ones.data_ptr(), ones.numel(), p, C.c_uint64(seed), None, y.data_ptr(), None))
    torch.cuda.synchronize()
    y = y.cpu()
    assert bool(((y == 0) | (y == y.max())).all()) and float(y.max()) > 1.0
    return y


def _no_nan(named):
    for name, t in named.items():
        for k, u in enumerate(t if isinstance(t, (list, tuple)) else [t]):
            assert not bool(torch.isnan(u).any()), f"{name}[{k}]: NaN left in a region the launch owns"


@pytest.fixture(scope="module")
def local_stats():
    stats = _Stats("local", tag="snv_fused")
    yield stats
    stats.show()


@pytest.fixture(scope="module")
def head_stats():
    stats = _Stats("head", tag="snv_fused")
    yield stats
    stats.show()


# ------------------------------------------------------------------------------------------------------- shared float64 references
def _check_linear(y, x, W, b, what, case, stats):
    """y = x W^T + b against float64 on the x the launch read: n = K terms, S = |x| |W|^T + |b|"""
    x64, W64 = x.double(), W.double()
    want, S = x64 @ W64.T, x64.abs() @ W64.abs().T
    if b is not None:
        want, S = want + b.double(), S + b.double().abs()
    _sum_check(y, want, S, x.shape[1], what, case, stats)


def _bn_forward(x, gamma, beta, rm, rv, keep, relu, dt):
    """training-mode BatchNorm1d over act(x) and the dropout behind it"""
    a = x.to(dt)
    a = a.clamp_min(0) if relu else a
    n = a.shape[0]
    var, mean = torch.var_mean(a, 0, unbiased=False)
    invstd = torch.rsqrt(var + EPS32)
    scale = gamma.to(dt) * invstd
    shift = beta.to(dt) - mean * scale
    return dict(scale=scale, shift=shift, mean=mean, invstd=invstd, y=(a * scale + shift) * keep.to(dt),
                running_mean=(1 - MOMENTUM) * rm.to(dt) + MOMENTUM * mean,
                running_var=(1 - MOMENTUM) * rv.to(dt) + MOMENTUM * var * (n / (n - 1)))


def _check_bn_forward(x, gamma, beta, rm, rv, keep, relu, got, prefix, case, stats):
    """state rows, running statistics and the dropped BatchNorm output of a launch that read x; got: state [4][C], running_mean,
    running_var, y"""
    want, ref = (_bn_forward(x, gamma, beta, rm, rv, keep, relu, dt) for dt in (F64, torch.float32))
    state = got["state"].cpu()
    for k, name in enumerate(("scale", "shift", "mean", "invstd")):
        _loose(state[k], want[name], ref[name], f"{prefix} {name}", case, stats)
    for name in ("running_mean", "running_var", "y"):
        _loose(got[name], want[name], ref[name], f"{prefix} {name}", case, stats)
    assert not bool(got["y"].cpu()[keep == 0].any()), f"{prefix}: the dropout's zeros at {case}"


def _bn_backward(du, x, state, gamma, relu, dt):
    """BatchNorm1d's backward behind act(x) with the saved mean / invstd: (d x, dgamma, dbeta)"""
    du, x, mean, invstd = du.to(dt), x.to(dt), state[2].to(dt), state[3].to(dt)
    xh = ((x.clamp_min(0) if relu else x) - mean) * invstd
    n = du.shape[0]
    s1, s2 = du.sum(0), (du * xh).sum(0)
    g = gamma.to(dt) * invstd * (du - s1 / n - xh * (s2 / n))
    return (torch.where(x > 0, g, torch.zeros_like(g)) if relu else g), s2, s1


def _check_masked_linear_bwd(dd, g, W, keep, what, case, stats):
    """dd = keep * (g W) against float64 on the g the launch read: n = O terms"""
    g64, W64, k64 = g.double(), W.double(), keep.double()
    _sum_check(dd, (g64 @ W64) * k64, (g64.abs() @ W64.abs()) * k64, g.shape[1], what, case, stats)
    assert not bool(dd.cpu()[keep == 0].any()), f"{what}: the dropout's zeros at {case}"


def _check_wgrad(dW, db, g, x, what, case, stats):
    g64, x64 = g.double(), x.double()
    _sum_check(dW, g64.T @ x64, g64.abs().T @ x64.abs(), g.shape[0], f"dW{what}", case, stats)
    _sum_check(db, g64.sum(0), g64.abs().sum(0), g.shape[0], f"db{what}", case, stats)


# ------------------------------------------------------------------------------------------------------------------ local branch
def _template(n, runs):
    kq = (n + 3) // 4               # the launchers' own rule
    return next(q for q in runs if kq <= q)


def test_local_shapes_cover_every_template_and_the_tail_path():
    """from the launchers' rule kq = (K + 3) / 4: the case list reaches all four forward runs with the gather and with the BatchNorm in
    front, all four backward runs in the middle and in the bottom launch and the two the top launch can take; each run length is met
    both full (K = 4 run: no lane's run crosses a row's end) and ragged (K < 4 run: the last row's lanes take lt_run's descriptor
    path, and K % 4 != 0 among them exercises the k0 + s < K masks); and the batches, output widths and tables the kernels' splits
    depend on are all there."""
    fwd_emb, fwd_bn, bwd_top, bwd_mid, bwd_bottom = set(), set(), set(), set(), set()
    full, ragged, odd = set(), set(), set()
    widths, batches, tables = set(), set(), set()
    for cols, emb_rows, h1, h2, nc, bs, _ in LOCAL_CASES:
        fwd_emb.add(_template(5 * cols, FWD_Q))
        fwd_bn |= {_template(h1, FWD_Q), _template(h2, FWD_Q)}
        bwd_top.add(_template(nc, BWD_Q))
        bwd_mid.add(_template(h2, BWD_Q))
        bwd_bottom.add(_template(h1, BWD_Q))
        for kind, runs, ks in (("fwd", FWD_Q, (5 * cols, h1, h2)), ("bwd", BWD_Q, (nc, h2, h1))):
            for k in ks:
                q = _template(k, runs)
                (full if k == 4 * q else ragged).add((kind, q))
                if k % 4:
                    odd.add((kind, q))
        widths |= {h1, h2, nc}
        batches |= set(bs)
        tables.add(emb_rows)
    assert fwd_emb == set(FWD_Q) and fwd_bn == set(FWD_Q)
    assert bwd_mid == set(BWD_Q) and bwd_bottom == set(BWD_Q) and bwd_top == {2, 19}
    every = {("fwd", q) for q in FWD_Q} | {("bwd", q) for q in BWD_Q}
    assert full == every and ragged == every and odd == every
    assert {1, 15, 16, 17, 64, 65} <= widths and {1, 3, 9, 75, 130} <= widths and {8, 9, 76, 77, 96, 97, 152, 153, 256} <= widths
    assert {2, 15, 16, 17, 37, 513, 529, 1100} == batches and tables == {5, 65, 1025}
    assert any(b == 1100 and h1 == 256 and e == 1025 for _, e, h1, _, _, bs, _ in LOCAL_CASES for b in bs)


def _local_params(cols, emb_rows, h1, h2, nc, seed):
    """float32 parameters on the host and the device.  Hidden unit N // 2 of both hidden layers (N >= 3) is dead: a zero weight row and a
    zero bias make its pre-activation exactly 0 in every row, the value at which `> 0` and `>= 0` part; running statistics start away
    from 0 / 1"""
    rng = torch.Generator().manual_seed(seed)
    dims = (5 * cols, h1, h2, nc)
    P = dict(cols=cols, emb_rows=emb_rows, dims=dims, E=torch.randn((emb_rows, 5), generator=rng))
    P["W"] = [torch.randn((dims[l + 1], dims[l]), generator=rng) / dims[l] ** 0.5 for l in range(3)]
    P["b"] = [0.3 * torch.randn(dims[l + 1], generator=rng) for l in range(3)]
    for l in range(2):
        if dims[l + 1] >= 3:
            P["W"][l][dims[l + 1] // 2] = 0.0
            P["b"][l][dims[l + 1] // 2] = 0.0
    P["gamma"] = [0.5 + torch.rand(dims[l + 1], generator=rng) for l in range(2)]
    P["beta"] = [0.3 * torch.randn(dims[l + 1], generator=rng) for l in range(2)]
    P["rm"] = [0.5 * torch.randn(dims[l + 1], generator=rng) for l in range(2)]
    P["rv"] = [0.5 + torch.rand(dims[l + 1], generator=rng) for l in range(2)]
    P["dev"] = {k: (v.cuda() if torch.is_tensor(v) else [t.cuda() for t in v]) for k, v in P.items() if k in ("E", "W", "b", "gamma", "beta")}
    return P


def _local_ids(B, cols, emb_rows, seed):
    """k-mer ids with the table's first and last row among them and half of all entries on three rows: the scatter collides"""
    rng = torch.Generator().manual_seed(seed)
    ids = torch.randint(0, emb_rows, (B, cols), generator=rng)
    hot = torch.tensor([0, emb_rows - 1, emb_rows // 2])[torch.randint(0, 3, (B, cols), generator=rng)]
    ids = torch.where(torch.rand((B, cols), generator=rng) < 0.5, hot, ids)
    ids[0, 0], ids[-1, -1] = 0, emb_rows - 1
    return ids


def _local_forward(P, cat_d, B, drop, seeds, seed_dev=None, alloc=None):
    """alloc: (rows, dims) the buffers are sized for, where the call's own B / dims will be refused"""
    d, D = P["dims"], P["dev"]
    R, a = alloc or (B, d)
    o = dict(xt=[_nan((R, a[l])) for l in range(3)], lin=[_nan((R, a[l + 1])) for l in range(2)], logits=_nan((R, a[3])),
             state=[_nan((4, a[l + 1])) for l in range(2)], rm=[t.cuda() for t in P["rm"]], rv=[t.cuda() for t in P["rv"]],
             _acc=[_acc(a[l + 1]) for l in range(2)])
    rc = _lib.lib().mural_debug_local_train_fwd(
        cat_d.data_ptr(), D["E"].data_ptr(), P["cols"], P["emb_rows"], B, (C.c_int32 * 4)(*d), _pp(D["W"]), _pp(D["b"]), _pp(D["gamma"]),
        _pp(D["beta"]), _pp(o["rm"]), _pp(o["rv"]), _pp(o["state"]), _pp(o["_acc"]), (C.c_float * 3)(*drop), (C.c_uint64 * 3)(*seeds),
        _ptr(seed_dev), EPS32, MOMENTUM, _pp(o["xt"]), _pp(o["lin"]), o["logits"].data_ptr(), None)
    torch.cuda.synchronize()
    return rc, o


def _local_backward(P, cat_d, B, fwd, dlogits_d, drop, seeds, seed_dev=None, alloc=None):
    d, D = P["dims"], P["dev"]
    R, a = alloc or (B, d)
    o = dict(dd=[_nan((R, a[l + 1])) for l in range(2)], g=[_nan((R, a[l + 1])) for l in range(2)],
             dW=[_nan((a[l + 1], a[l])) for l in range(3)], db=[_nan((a[l + 1],)) for l in range(3)],
             dgamma=[_nan((a[l + 1],)) for l in range(2)], dbeta=[_nan((a[l + 1],)) for l in range(2)], dE=_nan((P["emb_rows"], 5)),
             _acc=[_acc(a[l + 1]) for l in range(2)])
    rc = _lib.lib().mural_debug_local_train_bwd(
        cat_d.data_ptr(), P["cols"], P["emb_rows"], B, (C.c_int32 * 4)(*d), dlogits_d.data_ptr(), _pp(D["W"]), _pp(D["gamma"]),
        _pp(fwd["state"]), _pp(o["_acc"]), (C.c_float * 3)(*drop), (C.c_uint64 * 3)(*seeds), _ptr(seed_dev), _pp(fwd["xt"]), _pp(fwd["lin"]),
        _pp(o["dd"]), _pp(o["g"]), _pp(o["dW"]), _pp(o["db"]), _pp(o["dgamma"]), _pp(o["dbeta"]), o["dE"].data_ptr(), None)
    torch.cuda.synchronize()
    return rc, o


def _check_dE(dE, g0, W0, keep0, ids, emb_rows, case, stats):
    """dE[id][d] = sum over the (row, column) entries that hold id of t = keep * (g0 W0)[row][5 column + d].  Each t is a float32 sum of
    O = h1 terms times the keep scale: within 2 (O + 2) 2^-24 S_t of float64, S_t = keep |g0| |W0|.  A cell is a float32 atomic sum
    of its `hits` already-rounded kept terms (dropped ones add an exact 0) in whatever order the workgroups arrive:
    2 (hits + 2) 2^-24 sum |t| more.  The bound is the sum of both over the cell's terms; a cell nothing points at stays 0."""
    B, cols = ids.shape
    O = g0.shape[1]
    g64, W64, k64 = g0.double(), W0.double(), keep0.double()
    t, S_t = ((g64 @ W64) * k64).flatten(), ((g64.abs() @ W64.abs()) * k64).flatten()
    idx = ((ids.clamp(0, emb_rows - 1) * 5)[:, :, None] + torch.arange(5)).reshape(-1)
    cell = lambda v: torch.zeros(emb_rows * 5, dtype=F64).index_add_(0, idx, v)       # noqa: E731
    want, S_sum, S_abs, hits = cell(t), cell(S_t), cell(t.abs()), cell((k64 != 0).double().flatten())
    # 2 (O + 2) u S_sum + 2 (hits + 2) u S_abs, written as _sum_check's 2 (n + 2) u S with n = hits
    _sum_check(dE.flatten(), want, S_abs + S_sum * (O + 2.0) / (hits + 2.0), hits, "dE", case, stats)


def _check_local(P, ids, B, drop, seeds, fwd, dlogits, bwd, case, stats):
    d = P["dims"]
    keep = [_keep((B, d[l]), drop[l], seeds[l]) for l in range(3)]
    cpu = lambda v: [t.cpu() for t in v] if isinstance(v, list) else v.cpu()          # noqa: E731
    xt, lin, state, logits = cpu(fwd["xt"]), cpu(fwd["lin"]), cpu(fwd["state"]), cpu(fwd["logits"])
    _no_nan(dict(xt=xt, lin=lin, state=state, logits=logits, rm=cpu(fwd["rm"]), rv=cpu(fwd["rv"])))
    # F1: gather, dropout, Linear 1
    assert torch.equal(xt[0], P["E"][ids.clamp(0, P["emb_rows"] - 1)].reshape(B, d[0]) * keep[0]), f"xt0 at {case}"
    _check_linear(lin[0], xt[0], P["W"][0], P["b"][0], "lin0", case, stats)
    # F2, F3: BatchNorm of the launch before's output, dropout, Linear
    for l in (1, 2):
        got = dict(state=fwd["state"][l - 1], running_mean=fwd["rm"][l - 1], running_var=fwd["rv"][l - 1], y=xt[l])
        _check_bn_forward(lin[l - 1], P["gamma"][l - 1], P["beta"][l - 1], P["rm"][l - 1], P["rv"][l - 1], keep[l], True, got, f"bn{l - 1}", case, stats)
        _check_linear(logits if l == 2 else lin[1], xt[l], P["W"][l], P["b"][l], "logits" if l == 2 else "lin1", case, stats)
    dd, g = cpu(bwd["dd"]), cpu(bwd["g"])
    _no_nan({k: cpu(v) for k, v in bwd.items() if k != "_acc"})
    # B3: d logits W3, dropout mask; B2 / B1: BatchNorm backward + ReLU mask on the way in, Linear, dropout mask (B1: scatter)
    _check_masked_linear_bwd(dd[1], dlogits, P["W"][2], keep[2], "dd1", case, stats)
    for l in (1, 0):
        want, ref = (_bn_backward(dd[l], lin[l], state[l], P["gamma"][l], True, dt) for dt in (F64, torch.float32))
        for k, name in enumerate((f"g{l}", f"dgamma{l}", f"dbeta{l}")):
            _loose((g[l], bwd["dgamma"][l], bwd["dbeta"][l])[k], want[k], ref[k], name, case, stats)
        assert not bool(g[l][lin[l] <= 0].any()), f"g{l}: the ReLU mask at {case}"
        if l == 1:
            _check_masked_linear_bwd(dd[0], g[1], P["W"][1], keep[1], "dd0", case, stats)
        else:
            _check_dE(bwd["dE"].cpu(), g[0], P["W"][0], keep[0], ids, P["emb_rows"], case, stats)
    for l, gl in enumerate((g[0], g[1], dlogits)):
        _check_wgrad(bwd["dW"][l], bwd["db"][l], gl, xt[l], str(l), case, stats)


@pytest.mark.parametrize("cols,emb_rows,h1,h2,nc,batches,drop", LOCAL_CASES, ids=[f"c{c[0]}_e{c[1]}_h{c[2]}_{c[3]}_nc{c[4]}" for c in LOCAL_CASES])
def test_local_branch_launches_against_float64(cols, emb_rows, h1, h2, nc, batches, drop, local_stats):
    """the three forward launches, the three backward launches and the weight-gradient launch of the fused local branch, each against
    float64 on the tensors it read (module docstring), at the shapes of LOCAL_CASES.
    With the batch sums of relu(y) and relu(y)^2 taken in float before they reached the double accumulators, E[w^2] - mean^2 lost the
    variance of a channel whose spread is small against its mean: at B = 2 the kernel's scale was 1.06 from float64 (bound 2.6e-4;
    torch's float32: 3.3e-5) -- the sums are now taken in double, as bn_stats_kernel takes them.
    Observed on an MI355X, torch float32 / kernel error from float64 at the case nearest its bound: scale 7.1e-6 / 7.1e-6, invstd
    1.3e-5 / 1.3e-5, xt[2] 2.1e-6 / 7.0e-6 (B = 2), g1 1.0e-6 / 3.0e-6, dgamma1 6.5e-6 / 8.1e-6 (B = 1100); the sums at most 0.25 of
    their bounds (tests/CAPPED_LAUNCHES.md has every row)."""
    P = _local_params(cols, emb_rows, h1, h2, nc, seed=cols * 1000 + h1)
    for B in batches:
        case = f"cols{cols} emb{emb_rows} h{h1}/{h2} nc{nc} B{B} p{drop[0]:g}/{drop[1]:g}/{drop[2]:g}"
        ids = _local_ids(B, cols, emb_rows, seed=B)
        dlogits = torch.randn((B, nc), generator=torch.Generator().manual_seed(B + 7))
        cat_d, dl_d = ids.cuda(), dlogits.cuda()
        rc, fwd = _local_forward(P, cat_d, B, drop, SEEDS)
        _lib.check(rc)
        rc, bwd = _local_backward(P, cat_d, B, fwd, dl_d, drop, SEEDS)
        _lib.check(rc)
        _check_local(P, ids, B, drop, SEEDS, fwd, dlogits, bwd, case, local_stats)


def _flat(o):
    """every output tensor of a run (not its accumulators: their atomic sums depend on the order of arrival)"""
    return [t for k, v in o.items() if k != "_acc" for t in (v if isinstance(v, list) else [v])]


def test_local_branch_device_seed_offset_is_added_to_every_seed():
    """seed_dev holding v gives the bits of seeds + v with seed_dev = NULL, in every output of both directions -- and other masks than
    v = 0"""
    cols, emb_rows, h1, h2, nc, B, v = 15, 65, 8, 9, 8, 37, 0x5DEECE66D
    P = _local_params(cols, emb_rows, h1, h2, nc, seed=5)
    cat_d = _local_ids(B, cols, emb_rows, seed=6).cuda()
    dl_d = torch.randn((B, nc), generator=torch.Generator().manual_seed(8)).cuda()
    seed_dev = torch.tensor([v], dtype=torch.int64, device="cuda")
    runs = []
    for seeds, sd in ((SEEDS, seed_dev), (tuple(s + v for s in SEEDS), None), (SEEDS, None)):
        rc, fwd = _local_forward(P, cat_d, B, DROP, seeds, sd)
        _lib.check(rc)
        rc, bwd = _local_backward(P, cat_d, B, fwd, dl_d, DROP, seeds, sd)
        _lib.check(rc)
        del bwd["dE"]               # (float atomics in the order the waves arrive: not the same bits from one run to the next)
        runs.append(_flat(fwd) + _flat(bwd))
    for a, b in zip(runs[0], runs[1]):
        assert not bool(torch.isnan(a).any()) and torch.equal(_bits(a), _bits(b))
    assert not torch.equal(runs[0][0] == 0, runs[2][0] == 0)


def _last_error():
    return _lib.lib().mural_last_error().decode("utf-8", "replace")


def _all_nan(tensors):
    return all(bool(torch.isnan(t).all()) for t in tensors)


@pytest.mark.parametrize("cols,h1,h2,nc,B,what", [(52, 8, 8, 4, 3, "in1 260"), (2, 257, 8, 4, 3, "h1 257"), (2, 8, 257, 4, 3, "h2 257"),
                                                  (2, 8, 8, 257, 3, "nc 257"), (2, 8, 8, 0, 3, "nc 0"), (2, 8, 8, 4, 0, None)])
def test_local_branch_refusals_come_before_any_launch(cols, h1, h2, nc, B, what):
    """a Linear dimension of 257 (260 for in1) or 0: MURAL_E_INVALID with a message that names it; B = 0: MURAL_OK; either way every
    output is still NaN, the running statistics and the accumulators are as they were.  (Buffers have the size the shape would need.)"""
    P = _local_params(cols, 5, max(h1, 1), max(h2, 1), max(nc, 1), seed=9)
    alloc = (max(B, 1), P["dims"])
    P["dims"] = (5 * cols, h1, h2, nc)
    cat_d = _local_ids(alloc[0], cols, 5, seed=10).cuda()
    dl_d = torch.randn((alloc[0], alloc[1][3])).cuda()
    rc, fwd = _local_forward(P, cat_d, B, DROP, SEEDS, alloc=alloc)
    err_f = _last_error()
    rc_b, bwd = _local_backward(P, cat_d, B, fwd, dl_d, DROP, SEEDS, alloc=alloc)
    err_b = _last_error()
    for code, err in ((rc, err_f), (rc_b, err_b)):
        assert code == (_lib.MURAL_OK if what is None else _lib.MURAL_E_INVALID)
        assert what is None or ("local branch" in err and what in err), err
    assert _all_nan(fwd["xt"] + fwd["lin"] + fwd["state"] + [fwd["logits"]]) and _all_nan(_flat(bwd))
    for l in range(2):
        assert torch.equal(fwd["rm"][l].cpu(), P["rm"][l]) and torch.equal(fwd["rv"][l].cpu(), P["rv"][l])
        assert not bool(fwd["_acc"][l].any()) and not bool(bwd["_acc"][l].any())


# ------------------------------------------------------------------------------------------------------------------ tower head
def test_head_batches_cross_every_capped_launch():
    """each of the four capped launches meets a batch of exactly one round and one beyond it (two beyond for the launches of 8 rows per
    workgroup: 16385 leaves the second round one row, 16392 a whole workgroup)"""
    big = [B for B, _, _ in HEAD_BIG]
    for launch, rows in HEAD_CAPS.items():
        assert rows in big and rows + 1 in big, launch
    assert 16392 in big and {L for _, L, _ in HEAD_BIG} == {1, 2}
    assert {L for _, L, _ in HEAD_SMALL} == {1, 2, 7, 67} and {n for _, _, n in HEAD_SMALL} == {1, 2, 4, 5, 16}
    assert {B for B, _, _ in HEAD_SMALL} == {2, 7, 8, 9, 31, 32, 33, 257}


def _head_params(nc, seed):
    rng = torch.Generator().manual_seed(seed)
    P = dict(nc=nc, W=torch.randn((nc, HEAD_C), generator=rng) / HEAD_C ** 0.5, b=0.3 * torch.randn(nc, generator=rng),
             gamma=0.5 + torch.rand(HEAD_C, generator=rng), beta=0.3 * torch.randn(HEAD_C, generator=rng),
             rm=0.5 * torch.randn(HEAD_C, generator=rng), rv=0.5 + torch.rand(HEAD_C, generator=rng))
    P["dev"] = {k: v.cuda() for k, v in P.items() if torch.is_tensor(v)}
    return P


def _head_input(B, L, seed):
    """c3 [B][L][32] in tenths, so that columns hold their maximum more than once; a third of the (row, channel) columns are <= 0
    throughout, a third of those with an exact 0 as their maximum (at a random place, possibly twice); every other column has a
    positive value"""
    rng = torch.Generator().manual_seed(seed)
    x = (5.0 * torch.randn((B, L, HEAD_C), generator=rng)).round() / 10.0
    kind = torch.rand((B, 1, HEAD_C), generator=rng)
    x = torch.where(kind < 1 / 3, -x.abs(), x) + 0.0                # (+ 0.0: no negative zeros)
    at = torch.randint(0, L, (B, 1, HEAD_C), generator=rng)
    zero = (kind < 1 / 9) & (torch.arange(L)[None, :, None] == at)
    x = torch.where(zero, torch.zeros_like(x), x)
    lift = (kind >= 1 / 3) & (torch.arange(L)[None, :, None] == at)            # the other columns: at least one positive value
    return torch.where(lift, x.abs() + 0.1, x).contiguous()


def _head_forward(P, c3_d, B, L, p, seed, seed_dev=None, nc=None):
    nc = P["nc"] if nc is None else nc
    D, rows, ncb = P["dev"], max(B, 1), max(P["nc"], 1)
    o = dict(feat=_nan((rows, HEAD_C)), arg=torch.full((rows, HEAD_C), -1, dtype=torch.int32, device="cuda"), state=_nan((4, HEAD_C)),
             fd=_nan((rows, HEAD_C)), logits=_nan((rows, ncb)), rm=P["rm"].cuda(), rv=P["rv"].cuda())
    acc = _acc(HEAD_C)
    rc = _lib.lib().mural_debug_head_train_fwd(c3_d.data_ptr(), B, L, o["feat"].data_ptr(), o["arg"].data_ptr(), acc.data_ptr(),
                                               D["gamma"].data_ptr(), D["beta"].data_ptr(), EPS32, MOMENTUM, o["rm"].data_ptr(),
                                               o["rv"].data_ptr(), o["state"].data_ptr(), p, C.c_uint64(seed), _ptr(seed_dev),
                                               o["fd"].data_ptr(), D["W"].data_ptr(), D["b"].data_ptr(), nc, o["logits"].data_ptr(), None)
    torch.cuda.synchronize()
    return rc, o, acc


def _head_backward(P, c3_d, B, L, fwd, dl_d, p, seed, seed_dev=None, nc=None):
    nc = P["nc"] if nc is None else nc
    D, rows, ncb = P["dev"], max(B, 1), max(P["nc"], 1)
    o = dict(dd=_nan((rows, HEAD_C)), dx=_nan((rows, L, HEAD_C)), dgamma=_nan((HEAD_C,)), dbeta=_nan((HEAD_C,)), dW=_nan((ncb, HEAD_C)),
             db=_nan((ncb,)))
    acc = _acc(HEAD_C)
    rc = _lib.lib().mural_debug_head_train_bwd(dl_d.data_ptr(), D["W"].data_ptr(), nc, B, L, fwd["feat"].data_ptr(), fwd["state"].data_ptr(),
                                               D["gamma"].data_ptr(), p, C.c_uint64(seed), _ptr(seed_dev), o["dd"].data_ptr(), acc.data_ptr(),
                                               fwd["arg"].data_ptr(), c3_d.data_ptr(), o["dx"].data_ptr(), o["dgamma"].data_ptr(),
                                               o["dbeta"].data_ptr(), fwd["fd"].data_ptr(), o["dW"].data_ptr(), o["db"].data_ptr(), None)
    torch.cuda.synchronize()
    return rc, o, acc


def _check_head(P, c3, B, L, p, seed, fwd, dlogits, bwd, case, stats):
    keep = _keep((B, HEAD_C), p, seed)
    f = {k: v.cpu() for k, v in fwd.items()}
    _no_nan({k: v for k, v in f.items() if k != "arg"})
    # forward 1: global max, first arg-max, ReLU
    assert torch.equal(f["arg"], torch.from_numpy(np.argmax(c3.numpy(), axis=1).astype(np.int32))), f"arg at {case}"
    assert torch.equal(f["feat"], c3.max(1).values.clamp_min(0)), f"feat at {case}"
    # forward 2: BatchNorm of feat, dropout, Linear
    got = dict(state=fwd["state"], running_mean=f["rm"], running_var=f["rv"], y=f["fd"])
    _check_bn_forward(f["feat"], P["gamma"], P["beta"], P["rm"], P["rv"], keep, False, got, "fc_bn", case, stats)
    _check_linear(f["logits"], f["fd"], P["W"], P["b"], "logits", case, stats)
    b = {k: v.cpu() for k, v in bwd.items()}
    _no_nan(b)
    # backward 1: d logits W, dropout mask; backward 2: BatchNorm backward, through the arg-max and the ReLU mask
    _check_masked_linear_bwd(b["dd"], dlogits, P["W"], keep, "dd", case, stats)
    want, ref = (_bn_backward(b["dd"], f["feat"], f["state"], P["gamma"], False, dt) for dt in (F64, torch.float32))
    _loose(b["dgamma"], want[1], ref[1], "dgamma", case, stats)
    _loose(b["dbeta"], want[2], ref[2], "dbeta", case, stats)
    sel = (torch.arange(L)[None, :, None] == f["arg"][:, None, :]) & (c3 > 0)
    assert not bool(b["dx"][~sel].any()), f"dx: non-zero only at l == arg && c3 > 0, at {case}"
    spread = lambda v: torch.where(sel, v[:, None, :], torch.zeros((), dtype=v.dtype))       # noqa: E731
    _loose(b["dx"], spread(want[0]), spread(ref[0]), "dx", case, stats)
    _check_wgrad(b["dW"], b["db"], dlogits, f["fd"], "", case, stats)


def _head_case(B, L, nc, p, stats):
    case = f"B{B} L{L} nc{nc} p{p:g}"
    P = _head_params(nc, seed=100 * nc + L)
    c3 = _head_input(B, L, seed=B + L)
    dlogits = torch.randn((B, nc), generator=torch.Generator().manual_seed(B + 11))
    c3_d, dl_d = c3.cuda(), dlogits.cuda()
    rc, fwd, _ = _head_forward(P, c3_d, B, L, p, SEEDS[0])
    _lib.check(rc)
    rc, bwd, _ = _head_backward(P, c3_d, B, L, fwd, dl_d, p, SEEDS[0])
    _lib.check(rc)
    _check_head(P, c3, B, L, p, SEEDS[0], fwd, dlogits, bwd, case, stats)


@pytest.mark.parametrize("B", sorted({B for B, _, _ in HEAD_SMALL}))
def test_head_launches_against_float64(B, head_stats):
    """the two forward launches, the two backward launches and the weight gradient of the fused tower head, each against float64 on the
    tensors it read (module docstring); p = 0.25, and 0 and 0.5 once each.
    hd_gmax_stats_kernel took its batch sums in float like the local branch did: scale 0.11 from float64 at B = 2 (bound 1.9e-4), 2.5e-6
    at B = 31 (bound 1.6e-6); now in double.  Observed on an MI355X, torch float32 / kernel error at the case nearest its bound: scale
    1.6e-5 / 1.4e-5, fd 9.5e-6 / 2.3e-5 (B = 2), dgamma 7.9e-7 / 1.1e-6, dx 1.5e-7 / 1.5e-7."""
    for k, (_, L, nc) in enumerate(c for c in HEAD_SMALL if c[0] == B):
        _head_case(B, L, nc, 0.25, head_stats)
        if (B, k) in ((9, 0), (33, 1)):
            _head_case(B, L, nc, 0.0 if B == 9 else 0.5, head_stats)


@pytest.mark.parametrize("B,L,nc", HEAD_BIG)
def test_head_launches_beyond_their_capped_grids(B, L, nc, head_stats):
    """the same checks at batches of one round of each capped launch and one row (or one workgroup) beyond it: 16384 / 16385 / 16392 rows
    for hd_bn_drop_fc_kernel and hd_bwd1_kernel, 32768 / 32769 for hd_gmax_stats_kernel, 65536 / 65537 for hd_bwd2_kernel"""
    _head_case(B, L, nc, 0.25, head_stats)


def test_head_device_seed_offset_is_added_to_the_seed():
    B, L, nc, v = 33, 7, 5, 0x5DEECE66D
    P = _head_params(nc, seed=3)
    c3_d = _head_input(B, L, seed=4).cuda()
    dl_d = torch.randn((B, nc), generator=torch.Generator().manual_seed(5)).cuda()
    seed_dev = torch.tensor([v], dtype=torch.int64, device="cuda")
    runs = []
    for seed, sd in ((SEEDS[1], seed_dev), (SEEDS[1] + v, None), (SEEDS[1], None)):
        rc, fwd, _ = _head_forward(P, c3_d, B, L, 0.25, seed, sd)
        _lib.check(rc)
        rc, bwd, _ = _head_backward(P, c3_d, B, L, fwd, dl_d, 0.25, seed, sd)
        _lib.check(rc)
        runs.append({**fwd, **bwd})
    for name in runs[0]:
        assert torch.equal(_bits(runs[0][name]), _bits(runs[1][name])), name
        assert name == "arg" or not bool(torch.isnan(runs[0][name]).any())
    assert not torch.equal(runs[0]["fd"] == 0, runs[2]["fd"] == 0)


@pytest.mark.parametrize("nc,B", [(0, 3), (17, 3), (4, 0)])
def test_head_refusals_come_before_any_launch(nc, B):
    """0 and 17 classes: MURAL_E_INVALID with a message that names the count; B = 0: MURAL_OK; either way every output is still NaN
    (arg: -1), the running statistics and the accumulators are as they were.  (Buffers are sized for 17 classes.)"""
    L = 2
    P = _head_params(17, seed=6)
    c3_d = _head_input(max(B, 1), L, seed=7).cuda()
    dl_d = torch.randn((max(B, 1), 17)).cuda()
    rc, fwd, acc_f = _head_forward(P, c3_d, B, L, 0.25, SEEDS[0], nc=nc)
    err_f = _last_error()
    rc_b, bwd, acc_b = _head_backward(P, c3_d, B, L, fwd, dl_d, 0.25, SEEDS[0], nc=nc)
    err_b = _last_error()
    for code, err in ((rc, err_f), (rc_b, err_b)):
        assert code == (_lib.MURAL_OK if B == 0 else _lib.MURAL_E_INVALID)
        assert B == 0 or ("tower head" in err and f"got {nc}" in err), err
    assert _all_nan([fwd[k] for k in ("feat", "state", "fd", "logits")]) and _all_nan(list(bwd.values()))
    assert bool((fwd["arg"] == -1).all()) and torch.equal(fwd["rm"].cpu(), P["rm"]) and torch.equal(fwd["rv"].cpu(), P["rv"])
    assert not bool(acc_f.any()) and not bool(acc_b.any())
