"""The training-mode first layer of a tower, MaxPool1d(Conv1d(4 -> C, k = 3, pad 1)(BatchNorm1d(4)(one-hot))) evaluated from window symbols
(sym_hist_kernel -> first_tables_kernel -> first_train_kernel / first_pool_fwd_kernel, backwards through pooled_scatter,
first_bwd_cl_kernel or first_pool_bwd_kernel and first_part_reduce_kernel / first_param_grad_kernel), against float64 torch on the CPU:
the public entries mural_op_first_fwd / mural_op_first_bwd in the [B][C][L2] layout and the channel-last forms of the composed step
through the hooks mural_debug_first_fwd_cl / mural_debug_first_bwd_cl.

Reference: one-hot through the oracle's table (tests/_util.onehot), cropped, F.batch_norm in training mode, F.conv1d, F.max_pool1d with
indices, gradients from autograd.  Tolerances are the two rules of tests/_parity.py, with S the same float64 expression with every factor
replaced by its absolute value.

Near-ties: a float32 kernel may choose another maximum where two DISTINCT window values differ by rounding.  gap = float64 distance
between a window's maximum and its largest other value; an output is a flip candidate when gap < T = 8 * 2^-24 * (|bias| + sum|W . bn|)
at the maximum (the summation bound of the 13-term value for both competitors).  Outside the candidates the recorded position equals
torch's index (first maximum wins on exact ties); at a candidate it lies in the window and its float64 value is within T of the
maximum.  y is compared with the float64 value at the recorded position, the backward reference routes the gradient through the
recorded (validated) positions.  Candidates may be at most 0.1 % of the outputs of any case (asserted; checked on the CPU for the seeds
in use before any GPU run: the largest share over all cases is 0.0325 %, seeds 31000 .. 31107 = 31000 + 3 * geometry + input kind)."""
import functools
import math

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from mural_amd import _lib
from mural_amd.model import train_ops as T
from tests import _util as U
from tests._parity import EPS, MOMENTUM, NAN, U24, _Stats, _loose, _sum_check

pytestmark = pytest.mark.gpu

MAX_FLIP_SHARE = 1e-3

# (B, Lwin, col0, L1, C, pk, ps, pp) by group; a group is one test
_G = {
    # SLOT 16 (windows 4 .. 15): the table fast path needs pk == 15 and an interior ACGTN window, everything else is the in-kernel loop
    "slot16": [(37, 201, 0, 201, 32, 15, 15, 7), (37, 201, 50, 101, 32, 15, 15, 7), (37, 130, 0, 130, 32, 15, 15, 0)] +
              [(37, 97, 0, 97, 32, k, k, p) for k in (4, 8, 14) for p in (0, k // 2)],
    # SLOT 4 (windows 1 .. 3)
    "slot4": [(37, 97, 0, 97, 32, k, k, p) for k in (1, 2, 3) for p in sorted({0, k // 2})] + [(37, 97, 13, 64, 32, 3, 3, 1)],
    "stride": [(37, 97, 0, 97, 32, 3, 2, 1), (37, 97, 0, 97, 32, 2, 3, 0), (37, 201, 0, 201, 32, 15, 10, 7), (37, 201, 0, 201, 32, 8, 15, 4)],
    # a wave stages 512 bytes of the padded row (Lwin + 2) per round
    "staging": [(5, L, 0, L, 32, 15, 15, 7) for L in (509, 510, 511, 1023)],
    "batch": [(B, 61, 0, 61, 32, 15, 15, 7) for B in (1, 15, 16, 17)],
    # one row past 256 workgroups x 16 waves: a second round of the persistent loop, all 256 partial tables in the reduce
    "batch4097": [(4097, 31, 0, 31, 32, 3, 3, 1)],
    "generic": [(37, 200, 0, 200, 32, 16, 16, 8), (37, 200, 0, 200, 32, 20, 20, 10)] +
               [(37, 97, 0, 97, Cn, k, k, k // 2) for Cn in (16, 24, 64) for k in (15, 3)],
    # 125 x 64 x 33 = 264 000 pooled outputs: beyond one round of the generic backward's scatter launch (1024 workgroups of 256)
    "generic_batch125": [(125, 97, 0, 97, 64, 3, 3, 1)],
}
GEOMS = [g for grp in _G.values() for g in grp]
KINDS = ("acgt", "iupac", "ties")
_flip_share = {}        # case -> share of flip candidates (every case this process has evaluated)


def _L2(L1, pk, ps, pp):
    return (L1 + 2 * pp - pk) // ps + 1


def _symbols(seed, kind, B, Lwin, col0, L1, pk, ps, pp):
    g = np.random.default_rng(seed)
    sym = g.integers(0, 4, (B, Lwin)).astype(np.uint8)
    L2 = _L2(L1, pk, ps, pp)
    if kind == "iupac":         # 2 % N, 0.3 % of each code 5 .. 14, and planted ones where the kernels treat a column specially
        r = g.random((B, Lwin))
        sym[r < 0.02] = 4
        for k in range(10):
            sym[(r >= 0.02 + 0.003 * k) & (r < 0.023 + 0.003 * k)] = 5 + k
        for b in range(0, B, 2):
            code = 4 + (b // 2) % 11
            j2 = (L2 // 2 + b) % L2
            first, last = max(j2 * ps - pp, 0), min(j2 * ps - pp + pk - 1, L1 - 1)
            where = [(0, L1 - 1), (-1, L1), (L1 // 2, L1 // 2 + 1), (first, last), (first,), (last, last + 1)][(b // 2) % 6]
            for j in where:         # crop edges | just outside the crop | an adjacent pair | both ends of a pool window | ...
                if 0 <= col0 + j < Lwin:
                    sym[b, col0 + j] = code
    elif kind == "ties":        # every window holds its maximum several times: homopolymers, dinucleotide repeats, one all-N row
        for b in range(B):
            if b % 4 == 0:
                sym[b] = (b // 4) % 4
            elif b % 4 == 1:
                sym[b] = np.where((np.arange(Lwin) + b // 8) % 2 == 0, (b // 4) % 4, (b // 4 + 1 + b // 16) % 4)
            elif b % 4 == 2 and b % 8 == 2:
                sym[b] = np.resize(np.array([0, 1, 2], np.uint8) + (b % 2), Lwin)
        sym[min(2, B - 1)] = 4
    return torch.from_numpy(sym)


def _conv3(x, W, bias):
    """F.conv1d(x, W, bias, padding=1) in float64 as twelve element-wise multiply-adds in a fixed order.  F.conv1d runs a GEMM whose
    edge tiles round differently: the same 3-mer at two columns gave values one ulp apart, and the exact ties the first-maximum rule is
    tested on became near-ties (up to 5 % of a tie case's outputs).  Here equal inputs give equal values at every column."""
    xp = F.pad(x, (1, 1))
    L = x.shape[2]
    z = bias.view(1, -1, 1).expand(x.shape[0], -1, L)
    for t in range(3):
        for ci in range(4):
            z = z + W[:, ci, t].view(1, -1, 1) * xp[:, ci, t:t + L].unsqueeze(1)
    return z


def _routed(bn, W, bias, cols, dy):
    """sum of dy * conv(bn) at the columns `cols`: its autograd gradients are the layer's parameter gradients"""
    return (F.conv1d(bn, W, bias, padding=1).gather(2, cols) * dy).sum()


class _Case:
    """inputs and the float64 forward of one (geometry, symbol kind); computed once, shared by the tests, never modified"""

    def __init__(self, geom, kind):
        B, Lwin, col0, L1, Cn, pk, ps, pp = geom
        self.geom, self.kind, self.L2 = geom, kind, _L2(L1, pk, ps, pp)
        self.name = dict(B=B, Lwin=Lwin, col0=col0, L1=L1, C=Cn, pool=(pk, ps, pp), sym=kind)
        self.seed = 31000 + 3 * GEOMS.index(geom) + KINDS.index(kind)
        rng = torch.Generator().manual_seed(self.seed)
        self.sym = _symbols(self.seed, kind, B, Lwin, col0, L1, pk, ps, pp)
        self.W = torch.randn((Cn, 4, 3), generator=rng) / math.sqrt(12)
        self.bias = torch.randn(Cn, generator=rng) / math.sqrt(12)
        self.gamma = 1 + 0.3 * torch.randn(4, generator=rng)
        self.beta = 0.3 * torch.randn(4, generator=rng)
        self.rm, self.rv = 0.1 * torch.randn(4, generator=rng), 1 + 0.2 * torch.rand(4, generator=rng)
        self.dy = torch.randn((B, Cn, self.L2), generator=rng)
        crop = self.sym[:, col0:col0 + L1]
        self.counts = torch.bincount(crop.flatten().long(), minlength=16)
        self.x32 = U.onehot(self.sym.numpy())[:, :, col0:col0 + L1].contiguous()
        x = self.x32.double()
        rm, rv = self.rm.double(), self.rv.double()
        bn = F.batch_norm(x, rm, rv, self.gamma.double(), self.beta.double(), True, MOMENTUM, EPS)
        self.running = (rm, rv)
        rm32, rv32 = self.rm.clone(), self.rv.clone()
        F.batch_norm(self.x32, rm32, rv32, self.gamma, self.beta, True, MOMENTUM, EPS)
        self.running32 = (rm32, rv32)
        self.xhat = F.batch_norm(x, None, None, None, None, True, MOMENTUM, EPS)
        self.bn = bn
        W, bias = self.W.double(), self.bias.double()
        self.z = _conv3(bn, W, bias)
        assert float((self.z - F.conv1d(bn, W, bias, padding=1)).abs().max()) <= 1e-13, self.name
        self.Sz = _conv3(bn.abs(), W.abs(), bias.abs())
        self.ymax, self.idx = F.max_pool1d(self.z, pk, ps, pp, return_indices=True)
        win = F.pad(self.z, (pp, pp), value=-math.inf).unfold(-1, pk, ps)
        assert win.shape[2] == self.L2 and torch.equal(win.max(-1).values, self.ymax)
        other = win.masked_fill(win == self.ymax.unsqueeze(-1), -math.inf).max(-1).values
        self.T = 8.0 * U24 * self.Sz.gather(2, self.idx)
        self.cand = (self.ymax - other) < self.T
        self.tied = (win == self.ymax.unsqueeze(-1)).sum(-1) >= 2
        self.share = float(self.cand.double().mean())
        _flip_share[str(self.name)] = self.share

    def check_positions(self, cols):
        """the kernel's columns [B][C][L2]: in the window and the row, torch's index outside the flip candidates, within T at them"""
        B, Lwin, col0, L1, Cn, pk, ps, pp = self.geom
        lo = (torch.arange(self.L2) * ps - pp).view(1, 1, -1)
        assert bool(((cols >= lo) & (cols < lo + pk) & (cols >= 0) & (cols < L1)).all()), ("position outside its window", self.name)
        same = cols == self.idx
        assert bool((same | self.cand).all()), (f"{int((~same & ~self.cand).sum())} positions differ from torch's first maximum away from any "
                                                 f"near-tie", self.name)
        short = self.ymax - self.z.gather(2, cols)
        assert bool((short <= self.T)[self.cand].all()), ("a flipped position is no near-maximum", self.name)
        return int((~same).sum())

    def backward(self, cols, dy, dy_abs=None):
        """float64 gradients of the parameters with the pooled gradient dy routed through `cols`, and their absolute-value sums"""
        W, bias, gamma, beta = [t.double().requires_grad_() for t in (self.W, self.bias, self.gamma, self.beta)]
        bn = self.xhat * gamma.view(1, 4, 1) + beta.view(1, 4, 1)
        want = dict(zip(("dW", "dbias", "dgamma", "dbeta"), torch.autograd.grad(_routed(bn, W, bias, cols, dy), (W, bias, gamma, beta))))
        dy_abs = dy.abs() if dy_abs is None else dy_abs
        Wl, bl = torch.zeros_like(W).requires_grad_(), torch.zeros_like(bias).requires_grad_()
        S = dict(zip(("dW", "dbias"), torch.autograd.grad(_routed(self.bn.abs(), Wl, bl, cols, dy_abs), (Wl, bl))))
        gl, tl = torch.zeros(4, dtype=torch.float64, requires_grad=True), torch.zeros(4, dtype=torch.float64, requires_grad=True)
        bn_l = self.xhat.abs() * gl.view(1, 4, 1) + tl.view(1, 4, 1)
        S["dgamma"], S["dbeta"] = torch.autograd.grad(_routed(bn_l, W.detach().abs(), None, cols, dy_abs), (gl, tl))
        return want, S


@functools.lru_cache(maxsize=None)
def _case(geom, kind):
    return _Case(geom, kind)


def _check_share(cases):
    worst = max(cases, key=lambda c: c.share)
    print(f"[first_layer] flip candidates: at most {100 * worst.share:.4f} % of the outputs of a case (at {worst.name}); "
          f"largest share seen so far {100 * max(_flip_share.values()):.4f} %")
    assert worst.share <= MAX_FLIP_SHARE, (worst.share, worst.name)


# ------------------------------------------------------------------------------------------------------------------ device side
class _Dev:
    """device buffers of one case, outputs poisoned: NaN in tab / y / scratch / every gradient, 0xFF in arg, counts zeroed"""

    def __init__(self, c, cl=False):
        B, Lwin, col0, L1, Cn, pk, ps, pp = c.geom
        tab_f, arg_b, scr_f = T._first_plan(Cn, pk)
        self.c, self.cl, self.fast = c, cl, arg_b == 1
        self.sym = c.sym.cuda()
        self.p = [t.cuda() for t in (c.gamma, c.beta, c.W, c.bias)]
        self.rm, self.rv = c.rm.cuda(), c.rv.cuda()
        self.counts = torch.zeros(16, dtype=torch.int64, device="cuda")
        self.tab = torch.full((tab_f,), NAN, device="cuda")
        self.y = torch.full((B, c.L2, Cn) if cl else (B, Cn, c.L2), NAN, device="cuda")
        self.arg = torch.full((B * Cn * c.L2 * arg_b,), 0xFF, dtype=torch.uint8, device="cuda")
        self.scratch = torch.full((scr_f,), NAN, device="cuda")
        self.stat = torch.zeros((T.BN_SLOTS, 2, 32), dtype=torch.float64, device="cuda")
        self.st = T._stream(self.sym)

    def forward(self):
        """returns the entry's status (0 = done)"""
        c = self.c
        B, Lwin, col0, L1, Cn, pk, ps, pp = c.geom
        lib = _lib.lib()
        _lib.check(lib.mural_debug_poison_lds(self.st))
        ptr = [t.data_ptr() for t in self.p]
        if self.cl:
            return lib.mural_debug_first_fwd_cl(self.sym.data_ptr(), B, Lwin, col0, L1, pk, ps, pp, *ptr, EPS, MOMENTUM, self.rm.data_ptr(),
                                                self.rv.data_ptr(), self.counts.data_ptr(), self.tab.data_ptr(), self.y.data_ptr(),
                                                self.arg.data_ptr(), self.stat.data_ptr(), self.st)
        return lib.mural_op_first_fwd(self.sym.data_ptr(), B, Lwin, col0, L1, Cn, pk, ps, pp, *ptr, EPS, MOMENTUM, self.rm.data_ptr(),
                                      self.rv.data_ptr(), self.counts.data_ptr(), self.tab.data_ptr(), self.y.data_ptr(), self.arg.data_ptr(),
                                      self.st)

    def untouched(self):
        c = self.c
        return bool(self.y.isnan().all() and self.tab.isnan().all() and (self.arg == 0xFF).all() and (self.counts == 0).all()
                    and torch.equal(self.rm.cpu(), c.rm) and torch.equal(self.rv.cpu(), c.rv))

    def y_ncl(self):
        return (self.y.transpose(1, 2) if self.cl else self.y).cpu()

    def columns(self):
        """the recorded positions as tower columns [B][C][L2]"""
        B, Lwin, col0, L1, Cn, pk, ps, pp = self.c.geom
        if not self.fast:
            return self.arg.view(torch.int32).view(B, Cn, self.c.L2).cpu().long()
        w = self.arg.view(B, self.c.L2, Cn).cpu().long()            # window offsets, channel-last in both layouts
        assert int(w.max()) < pk, ("window offset beyond the window (or never written)", self.c.name)
        return (w + (torch.arange(self.c.L2) * ps - pp).view(1, -1, 1)).transpose(1, 2).contiguous()

    def backward(self, dy, fold=None):
        """dy [B][C][L2] (CPU), handed over in the layout of this form; fold: dict of device tensors + n.  Returns the gradients (CPU)"""
        c = self.c
        B, Lwin, col0, L1, Cn, pk, ps, pp = c.geom
        lib = _lib.lib()
        out = [torch.full(s, NAN, device="cuda") for s in ((Cn, 4, 3), (Cn,), (4,), (4,))]
        self.scratch.fill_(NAN)
        dyd = None if dy is None else (dy.transpose(1, 2) if self.cl else dy).contiguous().float().cuda()
        _lib.check(lib.mural_debug_poison_lds(self.st))
        args = [None if dyd is None else dyd.data_ptr(), self.arg.data_ptr(), self.sym.data_ptr(), B, Lwin, col0, L1]
        tail = [self.tab.data_ptr(), self.p[2].data_ptr(), self.scratch.data_ptr()] + [t.data_ptr() for t in out]
        if self.cl:
            f = fold or {}
            fp = [None if f.get(k) is None else f[k].data_ptr() for k in ("dz", "x", "add1", "add2", "state", "gamma", "acc")]
            fo = [None if f.get(k) is None else f[k].data_ptr() for k in ("dgamma", "dbeta")]
            rc = lib.mural_debug_first_bwd_cl(*args, pk, ps, pp, *tail, *fp, float(f.get("n", 0.0)), *fo, self.st)
        else:
            rc = lib.mural_op_first_bwd(*args, Cn, pk, ps, pp, *tail, self.st)
        _lib.check(rc)
        return dict(zip(("dW", "dbias", "dgamma", "dbeta"), [t.cpu() for t in out]))


def _check_grads(got, want, S, c, stats, tag="", extra=0, names=("dW", "dbias", "dgamma", "dbeta")):
    B, Cn = c.geom[0], c.geom[4]
    n = {"dW": B * c.L2 + 16, "dbias": B * c.L2 + 16, "dgamma": 3 * Cn * B * c.L2 + 16, "dbeta": 3 * Cn * B * c.L2 + 16}
    for k in names:
        _sum_check(got[k], want[k], S[k], n[k] + extra, k + tag, c.name, stats)


def _check_forward(d, stats, tag=""):
    """counts, running statistics, positions and y of a finished forward; returns the validated columns"""
    c = d.c
    assert torch.equal(d.counts.cpu()[:15], c.counts[:15]) and int(d.counts[15]) == 0, ("counts", c.name)
    for got, want, ref, k in ((d.rm, c.running[0], c.running32[0], "running_mean"), (d.rv, c.running[1], c.running32[1], "running_var")):
        _loose(got, want, ref, k + tag, c.name, stats)
    cols = d.columns()
    c.check_positions(cols)
    _sum_check(d.y_ncl(), c.z.gather(2, cols), c.Sz.gather(2, cols), 16, "y" + tag, c.name, stats)
    return cols


def _entry_case(c, stats, may_refuse=False):
    d = _Dev(c)
    rc = d.forward()
    if rc != 0:
        assert may_refuse and d.untouched(), ("refused" if may_refuse else "failed", rc, c.name)
        return 0, 0
    cols = _check_forward(d, stats)
    want, S = c.backward(cols, c.dy.double())
    _check_grads(d.backward(c.dy), want, S, c, stats)
    return int((cols != c.idx).sum()), int(c.tied.sum())


@pytest.mark.parametrize("group", list(_G))
def test_first_layer_entries_against_torch_float64(group):
    """mural_op_first_fwd / mural_op_first_bwd, [B][C][L2]: counts == bincount of the crop; running statistics (_loose against torch's
    float32 BatchNorm); positions (module docstring); y (summation bound, n = 16); dW, dbias (n = B L2 + 16), dgamma, dbeta
    (n = 3 C B L2 + 16) -- every output NaN / 0xFF before the call, LDS NaN in front of each call, for ACGT-only rows, rows with N and
    IUPAC codes planted at the crop edges, just outside the crop, as adjacent pairs and at both ends of a pool window, and
    rows of repeats (+ one all-N row) whose windows hold their maximum several times.  A stride that differs from the window may
    be refused, but then with a status and untouched outputs."""
    stats = _Stats(group, tag="first_layer")
    cases = [_case(g, kind) for g in _G[group] for kind in KINDS]
    _check_share(cases)
    flips = tied = 0
    for c in cases:
        f, t = _entry_case(c, stats, may_refuse=group == "stride")
        flips, tied = flips + f, tied + t
    print(f"[first_layer] {group}: {flips} positions flipped at near-ties; {tied} outputs with an exactly tied maximum")
    assert tied > 0, "the tie rows tie nothing"
    stats.show()


def test_first_layer_refuses_a_window_beyond_the_lds_working_set():
    """Lwin = 8001 with 15-wide windows: 16 per-wave rows and their window indices do not fit 160 KB.  Refused on the host in front of
    the first launch, forward and backward: a status, and no output (the running statistics included) is touched."""
    B, Lwin, pk = 3, 8001, 15
    geom = (B, Lwin, 0, Lwin, 32, pk, pk, 7)
    L2 = _L2(Lwin, pk, pk, 7)
    tab_f, arg_b, scr_f = T._first_plan(32, pk)
    sym = torch.zeros((B, Lwin), dtype=torch.uint8, device="cuda")
    w = [torch.ones(s, device="cuda") for s in ((4,), (4,), (32, 4, 3), (32,))]
    rm, rv, counts = torch.zeros(4, device="cuda"), torch.ones(4, device="cuda"), torch.zeros(16, dtype=torch.int64, device="cuda")
    tab, y, scratch = torch.full((tab_f,), NAN, device="cuda"), torch.full((B, 32, L2), NAN, device="cuda"), torch.full((scr_f,), NAN, device="cuda")
    arg = torch.full((B * 32 * L2,), 0xFF, dtype=torch.uint8, device="cuda")
    grads = [torch.full(s, NAN, device="cuda") for s in ((32, 4, 3), (32,), (4,), (4,))]
    st = T._stream(sym)
    with pytest.raises(ValueError, match="LDS"):
        T._call("mural_op_first_fwd", sym, *geom, *w, EPS, MOMENTUM, rm, rv, counts, tab, y, arg, st)
    with pytest.raises(ValueError, match="LDS"):
        T._call("mural_op_first_bwd", torch.zeros_like(y), arg, sym, *geom, tab, w[2], scratch, *grads, st)
    torch.cuda.synchronize()
    assert bool(tab.isnan().all() and y.isnan().all() and scratch.isnan().all() and (arg == 0xFF).all() and (counts == 0).all())
    assert bool((rm == 0).all() and (rv == 1).all()) and all(bool(g.isnan().all()) for g in grads)


# ------------------------------------------------------------------------------------------------------------------ channel-last
def _fold_inputs(c, y_cl, rng, with_res):
    """a BatchNorm(relu(x)) behind the first layer, x = the kernel's own y [B][L2][32]: its state from the float64 batch statistics
    rounded to float32, a random input gradient dz, the exact float64 sums, and the float64 pooled gradient of the documented formula
    with its absolute-value twin"""
    B, L2 = y_cl.shape[0], y_cl.shape[1]
    x = y_cl.double()
    a = torch.relu(x)
    gamma = 1 + 0.3 * torch.randn(32, generator=rng)
    beta = 0.3 * torch.randn(32, generator=rng)
    mean, invstd = a.mean((0, 1)).float(), (a.var((0, 1), unbiased=False) + EPS).rsqrt().float()
    state = torch.stack([gamma * invstd, beta, mean, invstd])
    dz = torch.randn((B, L2, 32), generator=rng)
    add = [torch.randn((B, L2, 32), generator=rng) if with_res else None for _ in range(2)]
    xhat = (x - mean.double()) * invstd.double()
    mask = x > 0
    dzm = dz.double()
    s1, s2 = dzm.sum((0, 1)), (dzm * xhat).sum((0, 1))          # (the sums the layer behind hands over; any values serve the formula)
    n = float(B * L2)
    k0 = gamma.double() * invstd.double()
    dy = torch.where(mask, k0 * (dzm - s1 / n - xhat * (s2 / n)), torch.zeros_like(x))
    dy_abs = torch.where(mask, k0.abs() * (dzm.abs() + (s1 / n).abs() + xhat.abs() * (s2 / n).abs()), torch.zeros_like(x))
    for t in add:
        if t is not None:
            dy, dy_abs = dy + t.double(), dy_abs + t.double().abs()
    acc = torch.zeros((T.BN_SLOTS, 2, 32), dtype=torch.float64)
    acc[0], acc[T.BN_SLOTS - 1] = 0.25 * torch.stack([s1, s2]), 0.75 * torch.stack([s1, s2])      # the reader sums every copy
    dev = dict(dz=dz.cuda(), x=y_cl.cuda(), add1=None if add[0] is None else add[0].cuda(), add2=None if add[1] is None else add[1].cuda(),
               state=state.cuda(), gamma=gamma.cuda(), acc=acc.cuda(), n=n, dgamma=torch.full((32,), NAN, device="cuda"),
               dbeta=torch.full((32,), NAN, device="cuda"))
    return dev, dy.transpose(1, 2).contiguous(), dy_abs.transpose(1, 2).contiguous(), acc.sum(0)


CL_GROUPS = ("slot16", "slot4", "batch", "batch4097")


@pytest.mark.parametrize("group", CL_GROUPS)
def test_first_layer_channel_last_forms(group, monkeypatch):
    """mural_debug_first_fwd_cl / mural_debug_first_bwd_cl on the table-path geometries (both SLOTs, odd and even L2, B = 17 and 4097)
    with the N / IUPAC rows and the tie rows: y and positions bit for bit the [B][C][L2] entry's; stat summed over its slots against
    the float64 sums of relu(y), relu(y)^2 of the kernel's own y (n = B L2); the unfolded backward (first_bwd_cl_kernel<false>) and,
    with MURAL_DEBUG_FIRST_SCATTER set for the call, pooled_scatter at cl = 1 within the entry's bounds; the folded backward
    (first_bwd_cl_kernel<true>) with both residuals and with neither against the float64 formula (x = the kernel's y, exact sums in
    acc; S from the formula with absolute values, 8 more roundings), against the unfolded kernel fed that gradient rounded to
    float32 (the two bounds added), and its dgamma / dbeta == the sums of acc rounded once."""
    stats = _Stats(group, tag="first_layer cl")
    cases = [_case(g, kind) for g in _G[group] for kind in ("iupac", "ties")]
    _check_share(cases)
    for c in cases:
        B, Cn = c.geom[0], c.geom[4]
        ref = _Dev(c)
        assert ref.forward() == 0, c.name
        d = _Dev(c, cl=True)
        assert d.forward() == 0, c.name
        assert torch.equal(d.y.transpose(1, 2), ref.y) and torch.equal(d.arg, ref.arg), ("channel-last forward differs from the entry's", c.name)
        cols = _check_forward(d, stats)
        yk = d.y.cpu()
        a = torch.relu(yk.double())
        sums = torch.stack([a.sum((0, 1)), (a * a).sum((0, 1))])
        _sum_check(d.stat.sum(0), sums, sums, B * c.L2, "stat", c.name, stats)
        want, S = c.backward(cols, c.dy.double())
        _check_grads(d.backward(c.dy), want, S, c, stats, " (cl)")
        monkeypatch.setenv("MURAL_DEBUG_FIRST_SCATTER", "1")         # (read by the library at every call)
        _check_grads(d.backward(c.dy), want, S, c, stats, " (cl scatter)")
        monkeypatch.delenv("MURAL_DEBUG_FIRST_SCATTER")
        rng = torch.Generator().manual_seed(c.seed + 500000)
        for with_res in (True, False):
            tag = " (fold + res)" if with_res else " (fold)"
            fold, dy64, dy_abs, acc_sum = _fold_inputs(c, yk, rng, with_res)
            want_f, S_f = c.backward(cols, dy64, dy_abs)
            got_f = d.backward(None, fold)
            _check_grads(got_f, want_f, S_f, c, stats, tag, extra=8)
            assert torch.equal(fold["dbeta"].cpu(), acc_sum[0].float()) and torch.equal(fold["dgamma"].cpu(), acc_sum[1].float()), (tag, c.name)
            got_u = d.backward(dy64.float())
            n_u = {"dW": B * c.L2 + 16, "dbias": B * c.L2 + 16, "dgamma": 3 * Cn * B * c.L2 + 16, "dbeta": 3 * Cn * B * c.L2 + 16}
            for k in got_f:         # both are within their bounds of float64: 2 (n_f + 2) + 2 (n_u + 2) = 2 ((n_f + n_u + 2) + 2)
                _sum_check(got_f[k], got_u[k].double(), S_f[k], 2 * n_u[k] + 8 + 2, k + tag + " vs unfolded", c.name, stats)
    stats.show()
