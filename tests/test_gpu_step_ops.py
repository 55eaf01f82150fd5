"""The criterion, the gradient clipping and the optimiser of the training step one by one through their C entries
(csrc/train_ops.hip: mural_op_ce_sum_fwd / _bwd, mural_op_clip_grad_norm, mural_op_adam_flat; csrc/train_state.hip:
mural_op_adam_flat_state) against the same operation in float64, at the sizes where their loops change course: the four-rows-per-thread
unroll of the 4-class criterion and its 1024-thread stride, the 64 shares of the clipping rounded up to four floats with their scalar
tail, the float4 groups of the Adam step beyond one round of its capped grid.  Outputs and scratch are NaN before every call.

Tolerances (tests/_parity.py) are derived, never tuned: ``_loose`` (8 x the distance of torch's float32 CPU result from float64, at
least 4 ulp) for everything with expf / logf / sqrt / a division in it, one float32 rounding for the norm, bit equality for the rest."""
import math

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from mural_amd import _lib
from tests._parity import NAN, _Stats, _loose

pytestmark = pytest.mark.gpu


def _nan(shape, dtype=torch.float32):
    return torch.full(shape if isinstance(shape, tuple) else (shape,), NAN, dtype=dtype, device="cuda")


def _bits(t):
    return t.detach().cpu().contiguous().view(torch.int32)


# ------------------------------------------------------------------------------------------------------------------ criterion
CE_ROWS = [1, 2, 1023, 1024, 1025, 4095, 4096, 4097, 8193, 65536]       # around the 1024 threads and the 4 x 1024 rows of one unrolled round
CE_SCALES = [1.0, 30.0, 1e3]


CE_SINGLE = ("equal", "spread", "near tie")       # what the one row of B = 1 is


def _ce_case(B, nc, scale, seed, single="equal"):
    """logits scale * randn; row 0: all logits equal (1.5 * scale); the last row (B >= 2): one logit at +88, the others at -88, the
    label on one of the others; row 1 (B >= 3): the label on the maximum and the runner-up 0.5 below it -- a small term from large
    logits.  B = 1: the row `single` names."""
    tg = torch.Generator().manual_seed(seed)
    x = scale * torch.randn((B, nc), generator=tg)
    y = torch.randint(0, nc, (B,), generator=tg)
    kinds = {0: "equal", B - 1: "spread", 1: "near tie"} if B >= 3 else {0: "equal", B - 1: "spread"} if B == 2 else {0: single}
    for row, kind in kinds.items():
        if kind == "equal":
            x[row] = 1.5 * scale
        elif kind == "spread":
            x[row] = -88.0
            x[row, (B + 1) % nc] = 88.0
            y[row] = B % nc
        else:
            top = float(x[row].abs().max()) + 1.5 * scale
            x[row, B % nc], x[row, (B + 1) % nc], y[row] = top, top - 0.5, B % nc
    return x, y


def _ce_fwd(x, y):
    B, nc = x.shape
    prob, loss = _nan((B, nc)), _nan(1)
    _lib.check(_lib.lib().mural_op_ce_sum_fwd(x.data_ptr(), y.data_ptr(), B, nc, prob.data_ptr(), loss.data_ptr(), None))
    torch.cuda.synchronize()
    return prob, loss


def _ce_bwd(prob, y, g):
    B, nc = prob.shape
    dx = _nan((B, nc))
    _lib.check(_lib.lib().mural_op_ce_sum_bwd(prob.data_ptr(), y.data_ptr(), g.data_ptr(), B, nc, dx.data_ptr(), None))
    torch.cuda.synchronize()
    return dx


def _ce_loss_bound(x, y):
    """(float64 loss, torch float32's error, bound): the rows' ``_loose`` bounds of lse - x_t added up (the kernel adds the rows in
    double) + one rounding of the total to float32"""
    rows64 = F.cross_entropy(x.double(), y, reduction="none")
    rows32 = F.cross_entropy(x, y, reduction="none").double()
    per_row = torch.maximum(8.0 * (rows32 - rows64).abs(), 4.0 * torch.from_numpy(np.spacing(rows64.float().numpy())).double())
    want = float(rows64.sum())
    return want, abs(float(rows32.sum()) - want), float(per_row.sum()) + 0.5 * float(np.spacing(np.float32(want)))


@pytest.mark.parametrize("nc", [4, 2, 3, 5, 16])
def test_ce_sum_forward_and_backward_against_torch_float64(nc):
    """prob, loss and dx (upstream gradient 0.37) of every row count x logit scale; prob and dx by ``_loose`` against softmax in
    float64, the loss within the sum of its rows' bounds.  The single row of B = 1 is in turn the row of equal logits, the +-88 row and
    a row whose label sits on the maximum half a unit above the runner-up: with the term formed as (m + log(sum)) - x_t in float the
    kernel was 6e-5 from a term of 1.39 at logits of 1500 (bound 5.4e-7; torch's float32: 4e-9).
    Observed on an MI355X, torch float32 / kernel error from float64 at the case nearest its bound: prob 1.0e-7 / 2.2e-7, dx
    4.5e-8 / 8.1e-8 (65536 rows of 16 classes)."""
    stats = _Stats(f"ce nc{nc}", tag="step_ops")
    g = torch.tensor([0.37])
    for B, single in [(1, s) for s in CE_SINGLE] + [(B, None) for B in CE_ROWS[1:]]:
        for scale in CE_SCALES:
            case = f"B{B} nc{nc} x{scale:g}" + (f" ({single})" if single else "")
            x, y = _ce_case(B, nc, scale, 1000 * nc + B, single)
            xd, yd = x.cuda(), y.cuda()
            prob, loss = _ce_fwd(xd, yd)
            want_p, ref_p = torch.softmax(x.double(), 1), torch.softmax(x, 1)
            _loose(prob, want_p, ref_p, "prob", case, stats)
            want, ref_err, bound = _ce_loss_bound(x, y)
            err = abs(float(loss.double().item()) - want)
            stats.add("loss", ref_err, err, bound, case)
            assert err <= bound, f"loss at {case}: {err:.3e} from float64, allowed {bound:.3e} (torch float32: {ref_err:.3e})"
            hot = F.one_hot(y, nc)
            dx = _ce_bwd(prob, yd, g.cuda())
            _loose(dx, g.double() * (want_p - hot.double()), g * (ref_p - hot.float()), "dx", case, stats)
    stats.show()


@pytest.mark.parametrize("nc", [4, 2, 3, 5, 16])
def test_ce_sum_label_outside_the_classes_gives_a_nan_loss(nc):
    """a label of -1 and a label of nc, in a row of the first unrolled round, of its ragged end and of a later round: the loss is NaN
    (built from its bits: the file is compiled without NaN semantics), every row of prob is what it is with the label inside"""
    for B, row in ((1, 0), (1025, 1024), (4097, 5), (4097, 4096), (8193, 3000)):
        x, y = _ce_case(B, nc, 1.0, 77 * nc + B)
        xd = x.cuda()
        prob_ok, loss_ok = _ce_fwd(xd, y.cuda())
        assert bool(torch.isfinite(loss_ok).all()) and bool(torch.isfinite(prob_ok).all())
        for bad in (-1, nc):
            yb = y.clone()
            yb[row] = bad
            prob, loss = _ce_fwd(xd, yb.cuda())
            assert math.isnan(float(loss.item())), (B, nc, row, bad, float(loss.item()))
            assert torch.equal(_bits(prob), _bits(prob_ok)), (B, nc, row, bad)


def test_ce_sum_four_class_and_run_time_kernels_give_the_same_bits():
    """The compile-time 4-class form against the run-time form on the same rows: the same logits widened to five classes by a column of
    -inf (its exponential is 0: it adds nothing to a row's sum, and no label points at it).  prob and loss bit for bit."""
    for B in CE_ROWS:
        for scale in CE_SCALES:
            x, y = _ce_case(B, 4, scale, 4000 + B)
            prob4, loss4 = _ce_fwd(x.cuda(), y.cuda())
            x5 = torch.cat([x, torch.full((B, 1), -math.inf)], 1).contiguous()
            prob5, loss5 = _ce_fwd(x5.cuda(), y.cuda())
            assert torch.equal(_bits(prob5[:, :4]), _bits(prob4)), (B, scale)
            assert not prob5[:, 4].any(), (B, scale)
            assert torch.equal(_bits(loss5), _bits(loss4)), (B, scale, float(loss4.item()), float(loss5.item()))


# ------------------------------------------------------------------------------------------------------------------ clipping
GUARD = 64
CLIP_LENGTHS = [0, 1, 3, 4, 5, 252, 255, 256, 257, 64 * 4 * 1024 - 1, 64 * 4 * 1024 + 5, 1_000_003]
U23 = 2.0 ** -23


def _clip(buf, n, max_norm):
    flat = buf.cuda()
    scratch, total = _nan(64, torch.float64), _nan(1)
    assert flat.data_ptr() % 16 == 0
    _lib.check(_lib.lib().mural_op_clip_grad_norm(flat.data_ptr(), n, float(max_norm), scratch.data_ptr(), total.data_ptr(), None))
    torch.cuda.synchronize()
    return flat.cpu(), np.float32(total.item())


def _clip_check(buf, n, max_norm, case, stats):
    """the norm to one float32 rounding of the float64 one; the n gradients g * coef bit for bit (untouched where coef >= 1), coef from
    the RETURNED norm in numpy float32; the guard floats behind them unchanged.  Returns (norm, coef)."""
    got, norm = _clip(buf, n, max_norm)
    want = math.sqrt(float((buf[:n].double() ** 2).sum()))
    err = abs(float(norm) - want)
    stats.add("norm", None, err, U23 * want, case)
    assert err <= U23 * want, f"norm at {case}: {float(norm)!r} against {want!r}"
    coef = np.float32(max_norm) / (norm + np.float32(1e-6))
    assert isinstance(coef, np.float32)
    g = buf[:n].numpy()
    expect = g if coef >= 1 else g * coef
    assert expect.dtype == np.float32
    diff = np.abs(got[:n].numpy().view(np.int32).astype(np.int64) - expect.view(np.int32).astype(np.int64))
    worst = int(diff.max()) if n else 0
    stats.add("g * coef (ulp)", None, float(worst), 0.0, case)
    assert worst == 0, f"gradients at {case}: {int((diff != 0).sum())} of {n} differ from g * {coef!r}, by up to {worst} ulp"
    assert torch.equal(_bits(got[n:]), _bits(buf[n:])), f"guard floats at {case}"
    return norm, coef


@pytest.mark.parametrize("n", CLIP_LENGTHS)
def test_clip_grad_norm_against_float64(n):
    """max_norm far above the norm (coef >= 1: nothing may change), far below it, equal to the returned norm and one float below that.
    coef = max_norm / (norm + 1e-6f) is two correctly rounded float32 operations and g * coef a third (the library is built without
    contraction and with correctly rounded division), so the scaled gradients are asserted bit for bit.
    Observed on an MI355X: bit for bit at every length."""
    stats = _Stats(f"clip n{n}", tag="step_ops")
    tg = torch.Generator().manual_seed(5000 + n)
    buf = torch.randn(n + GUARD, generator=tg)
    norm, coef = _clip_check(buf, n, 1e9, f"n{n} max_norm 1e9", stats)
    assert coef >= 1
    _, coef = _clip_check(buf, n, 0.37 * float(norm), f"n{n} max_norm 0.37 norm", stats)
    assert n == 0 or coef < 1
    _clip_check(buf, n, float(norm), f"n{n} max_norm = norm", stats)
    if n:
        _, coef = _clip_check(buf, n, float(np.nextafter(norm, np.float32(0))), f"n{n} max_norm just below the norm", stats)
        assert coef < 1
        # a small norm, where norm + 1e-6f is not the norm: max_norm = norm scales as well
        small = torch.cat([buf[:n] * (1e-3 / float(norm)), buf[n:]])
        norm_s, coef = _clip_check(small, n, 1e9, f"n{n} small", stats)
        _, coef = _clip_check(small, n, float(norm_s), f"n{n} small, max_norm = norm", stats)
        assert coef < 1
        # a zero gradient: norm 0, nothing changes (the guard is not zero)
        zero = torch.cat([torch.zeros(n), buf[n:]])
        norm_z, _ = _clip_check(zero, n, 0.37, f"n{n} zero gradient", stats)
        assert norm_z == 0
    stats.show()


# ------------------------------------------------------------------------------------------------------------------ Adam
ADAM_LENGTHS = [4, 8, 1020, 1024, 1028]
ADAM_LONG = 16384 * 256 * 4 + 4          # one float4 group beyond one round of the capped grid (16384 workgroups of 256 threads)
ADAM_SETTINGS = [(betas, eps, wd, step) for betas in ((0.9, 0.999), (0.5, 0.9)) for eps in (1e-8, 0.0) for wd in (0.0, 1e-2)
                 for step in (1, 2, 10_000)]
LR = 1e-3


def _adam_inputs(n, steps, seed):
    tg = torch.Generator().manual_seed(seed)
    p, m = torch.randn(n, generator=tg), 0.1 * torch.randn(n, generator=tg)
    v = 0.01 * torch.rand(n, generator=tg)
    v[0] = 0.0
    gs = [torch.randn(n, generator=tg) for _ in range(steps)]
    return p, gs, m, v


def _adam_float64(p, gs, m, v, betas, eps, wd, step):
    """the header comment of csrc/train_ops.h in float64"""
    p, m, v = p.double(), m.double(), v.double()
    b1, b2 = betas
    for i, g in enumerate(gs):
        t = step + i
        g = g.double() + wd * p
        m = m + (g - m) * (1.0 - b1)
        v = b2 * v + (1.0 - b2) * g * g
        step_size, bc2_sqrt = LR / (1.0 - b1 ** t), math.sqrt(1.0 - b2 ** t)
        p = p - step_size * m / (v.sqrt() / bc2_sqrt + eps)
    return p, m, v


def _adam_torch32(p, gs, m, v, betas, eps, wd, step):
    q = torch.nn.Parameter(p.clone())
    opt = torch.optim.Adam([q], lr=LR, betas=betas, eps=eps, weight_decay=wd, fused=False, foreach=False)
    opt.state[q] = dict(step=torch.tensor(float(step - 1)), exp_avg=m.clone(), exp_avg_sq=v.clone())
    for g in gs:
        q.grad = g.clone()
        opt.step()
    st = opt.state[q]
    assert int(st["step"]) == step - 1 + len(gs)
    return q.detach(), st["exp_avg"], st["exp_avg_sq"]


def _adam_device(p, gs, m, v, betas, eps, wd, step, state=None):
    """mural_op_adam_flat with step, step + 1, ...; or mural_op_adam_flat_state on a block ticked to the same step before every update"""
    lib = _lib.lib()
    pd, md, vd = p.cuda(), m.cuda(), v.cuda()
    n = p.numel()
    for i, g in enumerate(gs):
        gd = g.cuda()
        if state is None:
            _lib.check(lib.mural_op_adam_flat(pd.data_ptr(), gd.data_ptr(), md.data_ptr(), vd.data_ptr(), n, LR, betas[0], betas[1], eps, wd,
                                              step + i, None))
        else:
            _lib.check(lib.mural_op_train_state_tick(state.data_ptr(), None, 0, betas[0], betas[1], 0, 1.0, 0.0, 0.0, None))
            _lib.check(lib.mural_op_adam_flat_state(pd.data_ptr(), gd.data_ptr(), md.data_ptr(), vd.data_ptr(), n, state.data_ptr(), betas[0],
                                                    betas[1], eps, wd, None))
    torch.cuda.synchronize()
    return pd, md, vd


def _state_block(step):
    """a MuralTrainState (128 bytes: include/mural_hip.h) with rate LR and `step` updates done"""
    buf = torch.zeros(16, dtype=torch.int64)
    buf.view(torch.float64)[0] = LR
    buf[1] = step
    return buf.cuda()


@pytest.mark.parametrize("steps", [1, 10])
def test_adam_flat_against_float64(steps):
    """p, exp_avg and exp_avg_sq after one and after ten updates, each by ``_loose`` against the formula in float64, torch's
    single-tensor Adam in float32 on the CPU as the measure.
    Observed on an MI355X, torch float32 / kernel error from float64 at the case nearest its bound, one update: p 1.2e-7 / 1.2e-7,
    exp_avg 5.7e-9 / 6.5e-8 (bound 2.4e-7: 4 ulp), exp_avg_sq 1.0e-9 / 2.9e-9; ten updates: p 5.3e-7 / 5.3e-7, exp_avg 1.2e-8 / 2.7e-8,
    exp_avg_sq 2.8e-9 / 6.5e-9."""
    stats = _Stats(f"adam x{steps}", tag="step_ops")
    for n in ADAM_LENGTHS:
        for k, (betas, eps, wd, step) in enumerate(ADAM_SETTINGS):
            case = f"n{n} betas{betas} eps{eps:g} wd{wd:g} step{step}"
            ins = _adam_inputs(n, steps, 100 * n + k)
            want = _adam_float64(*ins, betas, eps, wd, step)
            ref = _adam_torch32(*ins, betas, eps, wd, step)
            got = _adam_device(*ins, betas, eps, wd, step)
            for name, a, w, r in zip(("p", "exp_avg", "exp_avg_sq"), got, want, ref):
                _loose(a, w, r, name, case, stats)
    stats.show()


def test_adam_flat_beyond_one_round_of_its_grid():
    """16384 x 256 x 4 + 4 floats (67 MB a buffer), one update: the buffers repeat a base of 4099 floats, so the reference is computed
    once, every repetition must carry the bits of the first, and the first is judged as above"""
    stats = _Stats("adam long", tag="step_ops")
    base_n = 4099
    reps, tail = divmod(ADAM_LONG, base_n)
    assert tail and reps * base_n + tail == ADAM_LONG

    def long(t):
        return torch.cat([t.repeat(reps), t[:tail]])

    for betas, eps, wd, step in (((0.9, 0.999), 1e-8, 0.0, 1), ((0.5, 0.9), 0.0, 1e-2, 10_000)):
        case = f"n{ADAM_LONG} betas{betas} eps{eps:g} wd{wd:g} step{step}"
        p, gs, m, v = _adam_inputs(base_n, 1, step)
        want = _adam_float64(p, gs, m, v, betas, eps, wd, step)
        ref = _adam_torch32(p, gs, m, v, betas, eps, wd, step)
        got = _adam_device(long(p), [long(gs[0])], long(m), long(v), betas, eps, wd, step)
        for name, a, w, r in zip(("p", "exp_avg", "exp_avg_sq"), got, want, ref):
            assert a.shape == (ADAM_LONG,)
            folded = a[:reps * base_n].view(reps, base_n)
            assert torch.equal(folded, folded[:1].expand_as(folded)), (name, case)
            assert torch.equal(a[reps * base_n:], a[:tail]), (name, case)
            _loose(a[:base_n], w, r, name, case, stats)
    stats.show()


@pytest.mark.parametrize("n", ADAM_LENGTHS)
def test_adam_flat_state_equals_adam_flat_bit_for_bit(n):
    """a MuralTrainState ticked to step t, then mural_op_adam_flat_state: the three buffers carry the bits mural_op_adam_flat leaves for
    step = t and the same rate, after one update and after ten"""
    for k, (betas, eps, wd, step) in enumerate(ADAM_SETTINGS):
        for steps in (1, 10):
            ins = _adam_inputs(n, steps, 7 * n + k)
            want = _adam_device(*ins, betas, eps, wd, step)
            state = _state_block(step - 1)
            got = _adam_device(*ins, betas, eps, wd, step, state=state)
            words = state.cpu()
            assert int(words[1]) == step - 1 + steps and float(words.view(torch.float64)[0]) == LR
            for name, a, w in zip(("p", "exp_avg", "exp_avg_sq"), got, want):
                f = words.view(torch.float32)
                assert torch.equal(_bits(a), _bits(w)), (name, n, betas, eps, wd, step, steps, float(f[12]), float(f[13]))


def test_adam_flat_refuses_bad_arguments_and_leaves_the_buffers():
    """a length that is no multiple of 4, a buffer 4 bytes off its alignment, beta = 1, step = 0: the library's error (a ValueError) from
    both entries, and no buffer is touched"""
    lib = _lib.lib()
    n = 1024
    p, gs, m, v = _adam_inputs(n + 4, 1, 9)
    bufs = [t.cuda() for t in (p, gs[0], m, v)]
    before = [t.clone() for t in bufs]
    state = _state_block(3)
    _lib.check(lib.mural_op_train_state_tick(state.data_ptr(), None, 0, 0.9, 0.999, 0, 1.0, 0.0, 0.0, None))
    ptr = [t.data_ptr() for t in bufs]
    assert all(q % 16 == 0 for q in ptr)
    off = [[q + 4 if i == j else q for i, q in enumerate(ptr)] for j in range(4)]
    # (pointers, n, beta1, beta2, step)
    bad = [(ptr, n - 1, 0.9, 0.999, 1), (ptr, n + 2, 0.9, 0.999, 1), (ptr, n, 1.0, 0.999, 1), (ptr, n, 0.9, 1.0, 1), (ptr, n, 0.9, 0.999, 0)]
    bad += [(o, n, 0.9, 0.999, 1) for o in off]
    for ptrs, nn, b1, b2, step in bad:
        with pytest.raises(ValueError, match="adam_flat"):
            _lib.check(lib.mural_op_adam_flat(*ptrs, nn, LR, b1, b2, 1e-8, 0.0, step, None))
        if step != 0:       # (the state entry takes its step from the block)
            with pytest.raises(ValueError, match="adam_flat"):
                _lib.check(lib.mural_op_adam_flat_state(*ptrs, nn, state.data_ptr(), b1, b2, 1e-8, 0.0, None))
    torch.cuda.synchronize()
    for t, t0 in zip(bufs, before):
        assert torch.equal(_bits(t), _bits(t0))
