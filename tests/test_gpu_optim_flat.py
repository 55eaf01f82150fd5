"""The flat AdamW (amsgrad) and SGD (momentum, nesterov) steps through their C entries (csrc/train_ops.hip: mural_op_adamw_amsgrad_flat,
mural_op_sgd_flat; csrc/train_state.hip: their _state twins) against torch's own optimisers stepped on float64 CPU tensors: three
consecutive updates from the same start, at 4 floats, at 4 x 257 (past one workgroup) and at 16384 x 256 x 4 + 4 (one float4 group past
the capped grid, the length tests/CAPPED_LAUNCHES.md gives for adam_flat_kernel, whose grid these launches use).

Tolerances are the rule of tests/_parity.py that the Adam case of tests/test_gpu_step_ops.py uses: ``_loose`` -- 8 x the distance of torch's
single-tensor float32 CPU result from float64, at least 4 ulp of the output's largest magnitude; bit equality between the state entries
and the host-argument entries, and for the padding, which stays +0."""
import numpy as np
import pytest
import torch

from mural_amd import _lib
from tests._parity import _Stats, _loose

pytestmark = pytest.mark.gpu

LR = 1e-3
STEPS = 3
LENGTHS = [4, 4 * 257]
LONG = 16384 * 256 * 4 + 4
# (betas, eps, weight_decay, first step): a fresh optimiser, and one far into training with decay on
ADAMW_SETTINGS = [((0.9, 0.999), 1e-8, 0.0, 1), ((0.9, 0.999), 1e-8, 1e-2, 1), ((0.5, 0.9), 1e-8, 1e-2, 10_000)]
SGD_SETTINGS = [(0.98, 0.0), (0.98, 1e-2), (0.5, 1e-6)]            # (momentum, weight_decay)


def _bits(t):
    return t.detach().cpu().contiguous().view(torch.int32)


def _inputs(n, seed, fresh):
    """p, [g] * STEPS, m, v, vmax, buf and the padding mask.  The last quarter of every buffer is padding (all zero); among the rest every
    seventh gradient element is exactly 0 in every step; the gradients shrink 30-fold after the first step, so exp_avg_sq falls below
    max_exp_avg_sq from the second update on; with a history (`fresh` False) a third of max_exp_avg_sq starts well above exp_avg_sq."""
    tg = torch.Generator().manual_seed(seed)
    pad = torch.zeros(n, dtype=torch.bool)
    pad[n - n // 4:] = True
    p = torch.randn(n, generator=tg)
    gs = [torch.randn(n, generator=tg) * (1.0 if i == 0 else 1.0 / 30) for i in range(STEPS)]
    for g in gs:
        g[::7] = 0.0
    if fresh:
        m, v, vmax, buf = (torch.zeros(n) for _ in range(4))
    else:
        m = 0.1 * torch.randn(n, generator=tg)
        v = 0.01 * torch.rand(n, generator=tg)
        vmax = v.clone()
        vmax[::3] *= 4.0
        buf = torch.randn(n, generator=tg)
    for t in [p, m, v, vmax, buf] + gs:
        t[pad] = 0.0
    return p, gs, m, v, vmax, buf, pad


def _torch_adamw(dtype, p, gs, m, v, vmax, betas, eps, wd, step):
    q = torch.nn.Parameter(p.to(dtype).clone())
    opt = torch.optim.AdamW([q], lr=LR, betas=betas, eps=eps, weight_decay=wd, amsgrad=True, foreach=False, fused=False)
    if step > 1:
        opt.state[q] = dict(step=torch.tensor(float(step - 1)), exp_avg=m.to(dtype).clone(), exp_avg_sq=v.to(dtype).clone(),
                            max_exp_avg_sq=vmax.to(dtype).clone())
    for g in gs:
        q.grad = g.to(dtype).clone()
        opt.step()
    st = opt.state[q]
    assert int(st["step"]) == step - 1 + len(gs)
    return q.detach(), st["exp_avg"], st["exp_avg_sq"], st["max_exp_avg_sq"]


def _torch_sgd(dtype, p, gs, buf, fresh, momentum, wd):
    q = torch.nn.Parameter(p.to(dtype).clone())
    opt = torch.optim.SGD([q], lr=LR, momentum=momentum, nesterov=True, weight_decay=wd, foreach=False)
    if not fresh:
        opt.state[q] = dict(momentum_buffer=buf.to(dtype).clone())
    for g in gs:
        q.grad = g.to(dtype).clone()
        opt.step()
    return q.detach(), opt.state[q]["momentum_buffer"]


def _state_block(step, lr=LR):
    """a MuralTrainState (128 bytes: include/mural_hip.h) with rate `lr` and `step` updates done"""
    buf = torch.zeros(16, dtype=torch.int64)
    buf.view(torch.float64)[0] = lr
    buf[1] = step
    return buf.cuda()


def _tick(state, betas=(0.9, 0.999)):
    _lib.check(_lib.lib().mural_op_train_state_tick(state.data_ptr(), None, 0, betas[0], betas[1], 0, 1.0, 0.0, 0.0, None))


def _device_adamw(p, gs, m, v, vmax, betas, eps, wd, step, state=None):
    lib = _lib.lib()
    bufs = [t.cuda() for t in (p, m, v, vmax)]
    pd, md, vd, xd = (t.data_ptr() for t in bufs)
    for i, g in enumerate(gs):
        gd = g.cuda()
        if state is None:
            _lib.check(lib.mural_op_adamw_amsgrad_flat(pd, gd.data_ptr(), md, vd, xd, p.numel(), LR, betas[0], betas[1], eps, wd, step + i, None))
        else:
            _tick(state, betas)
            _lib.check(lib.mural_op_adamw_amsgrad_flat_state(pd, gd.data_ptr(), md, vd, xd, p.numel(), state.data_ptr(), betas[0], betas[1], eps,
                                                             wd, None))
    torch.cuda.synchronize()
    return bufs


def _device_sgd(p, gs, buf, momentum, wd, state=None):
    lib = _lib.lib()
    bufs = [t.cuda() for t in (p, buf)]
    pd, bd = (t.data_ptr() for t in bufs)
    for g in gs:
        gd = g.cuda()
        if state is None:
            _lib.check(lib.mural_op_sgd_flat(pd, gd.data_ptr(), bd, p.numel(), LR, momentum, wd, None))
        else:
            _tick(state)
            _lib.check(lib.mural_op_sgd_flat_state(pd, gd.data_ptr(), bd, p.numel(), state.data_ptr(), momentum, wd, None))
    torch.cuda.synchronize()
    return bufs


ADAMW_NAMES = ("p", "exp_avg", "exp_avg_sq", "max_exp_avg_sq")
SGD_NAMES = ("p", "momentum_buffer")


def _judge(names, got, want, ref, pad, case, stats):
    for name, a, w, r in zip(names, got, want, ref):
        assert not bool(_bits(a)[pad].any()), f"{name} at {case}: the padding did not stay +0"
        _loose(a, w, r, name, case, stats)


@pytest.mark.parametrize("n", LENGTHS)
def test_adamw_amsgrad_flat_against_torch_float64(n):
    stats = _Stats(f"adamw n{n}", tag="optim_flat")
    for k, (betas, eps, wd, step) in enumerate(ADAMW_SETTINGS):
        case = f"n{n} betas{betas} eps{eps:g} wd{wd:g} step{step}"
        p, gs, m, v, vmax, _, pad = _inputs(n, 100 * n + k, fresh=step == 1)
        want = _torch_adamw(torch.float64, p, gs, m, v, vmax, betas, eps, wd, step)
        ref = _torch_adamw(torch.float32, p, gs, m, v, vmax, betas, eps, wd, step)
        live = ~pad
        assert bool((want[3][live] > want[2][live]).any()), "amsgrad's max must matter in this case"
        got = _device_adamw(p, gs, m, v, vmax, betas, eps, wd, step)
        _judge(ADAMW_NAMES, got, want, ref, pad, case, stats)
    stats.show()


@pytest.mark.parametrize("n", LENGTHS)
def test_sgd_flat_against_torch_float64(n):
    stats = _Stats(f"sgd n{n}", tag="optim_flat")
    for k, (momentum, wd) in enumerate(SGD_SETTINGS):
        for fresh in (True, False):
            case = f"n{n} momentum{momentum:g} wd{wd:g} {'first step' if fresh else 'with a buffer'}"
            p, gs, _, _, _, buf, pad = _inputs(n, 200 * n + k, fresh)
            want = _torch_sgd(torch.float64, p, gs, buf, fresh, momentum, wd)
            ref = _torch_sgd(torch.float32, p, gs, buf, fresh, momentum, wd)
            got = _device_sgd(p, gs, buf, momentum, wd)
            _judge(SGD_NAMES, got, want, ref, pad, case, stats)
    stats.show()


def test_both_steps_beyond_one_round_of_the_grid():
    """16384 x 256 x 4 + 4 floats a buffer: the buffers repeat a base of 4099 floats, so torch steps the base once, every repetition must
    carry the bits of the first, and the first is judged as above (the scheme of test_adam_flat_beyond_one_round_of_its_grid)."""
    stats = _Stats("long", tag="optim_flat")
    base_n = 4099
    reps, tail = divmod(LONG, base_n)
    assert tail and reps * base_n + tail == LONG

    def long(t):
        return torch.cat([t.repeat(reps), t[:tail]])

    def folded_equal(a, name, case):
        assert a.shape == (LONG,)
        f = a[:reps * base_n].view(reps, base_n)
        assert torch.equal(f, f[:1].expand_as(f)), (name, case)
        assert torch.equal(a[reps * base_n:], a[:tail]), (name, case)

    betas, eps, wd, step = (0.9, 0.999), 1e-8, 1e-2, 10_000
    p, gs, m, v, vmax, buf, pad = _inputs(base_n, 5, fresh=False)
    case = f"adamw n{LONG}"
    want = _torch_adamw(torch.float64, p, gs, m, v, vmax, betas, eps, wd, step)
    ref = _torch_adamw(torch.float32, p, gs, m, v, vmax, betas, eps, wd, step)
    got = _device_adamw(long(p), [long(g) for g in gs], long(m), long(v), long(vmax), betas, eps, wd, step)
    for name, a in zip(ADAMW_NAMES, got):
        folded_equal(a, name, case)
    _judge(ADAMW_NAMES, [a[:base_n] for a in got], want, ref, pad, case, stats)
    del got
    case = f"sgd n{LONG}"
    want = _torch_sgd(torch.float64, p, gs, buf, False, 0.98, wd)
    ref = _torch_sgd(torch.float32, p, gs, buf, False, 0.98, wd)
    got = _device_sgd(long(p), [long(g) for g in gs], long(buf), 0.98, wd)
    for name, a in zip(SGD_NAMES, got):
        folded_equal(a, name, case)
    _judge(SGD_NAMES, [a[:base_n] for a in got], want, ref, pad, case, stats)
    stats.show()


@pytest.mark.parametrize("n", LENGTHS)
def test_state_entries_equal_host_argument_entries_bit_for_bit(n):
    """a MuralTrainState filled with lr and step - 1, a tick, then the state entry: every buffer carries the bits the host-argument entry
    leaves for the same lr and step, over three updates"""
    for k, (betas, eps, wd, step) in enumerate(ADAMW_SETTINGS):
        p, gs, m, v, vmax, _, _ = _inputs(n, 7 * n + k, fresh=step == 1)
        want = _device_adamw(p, gs, m, v, vmax, betas, eps, wd, step)
        state = _state_block(step - 1)
        got = _device_adamw(p, gs, m, v, vmax, betas, eps, wd, step, state=state)
        words = state.cpu()
        assert int(words[1]) == step - 1 + STEPS and float(words.view(torch.float64)[0]) == LR
        for name, a, w in zip(ADAMW_NAMES, got, want):
            assert torch.equal(_bits(a), _bits(w)), ("adamw", name, n, betas, eps, wd, step)
    for k, (momentum, wd) in enumerate(SGD_SETTINGS):
        p, gs, _, _, _, buf, _ = _inputs(n, 9 * n + k, fresh=False)
        want = _device_sgd(p, gs, buf, momentum, wd)
        state = _state_block(0)
        got = _device_sgd(p, gs, buf, momentum, wd, state=state)
        assert int(state.cpu()[1]) == STEPS
        for name, a, w in zip(SGD_NAMES, got, want):
            assert torch.equal(_bits(a), _bits(w)), ("sgd", name, n, momentum, wd)


def _refused(call, what):
    with pytest.raises(ValueError, match=what):
        _lib.check(call())
    assert what in _lib.lib().mural_last_error().decode()


def test_bad_arguments_are_refused_and_nothing_is_launched():
    """a NULL buffer, a length that is no multiple of 4, a buffer 4 bytes off its alignment, a negative lr (host-argument entries), a NULL
    state block (state entries): the library's error with mural_last_error set, and no buffer is touched"""
    lib = _lib.lib()
    n = 1024
    p, gs, m, v, vmax, buf, _ = _inputs(n + 4, 3, fresh=False)
    state = _state_block(3)
    _tick(state)
    for which, tensors in (("adamw_amsgrad_flat", (p, gs[0], m, v, vmax)), ("sgd_flat", (p, gs[0], buf))):
        bufs = [t.cuda() for t in tensors]
        before = [t.clone() for t in bufs]
        ptr = [t.data_ptr() for t in bufs]
        assert all(q % 16 == 0 for q in ptr)
        if which == "sgd_flat":
            host = lambda ps, nn, lr: lib.mural_op_sgd_flat(*ps, nn, lr, 0.98, 0.0, None)                                       # noqa: E731
            dev = lambda ps, nn, st: lib.mural_op_sgd_flat_state(*ps, nn, st, 0.98, 0.0, None)                                  # noqa: E731
        else:
            host = lambda ps, nn, lr: lib.mural_op_adamw_amsgrad_flat(*ps, nn, lr, 0.9, 0.999, 1e-8, 0.0, 1, None)              # noqa: E731
            dev = lambda ps, nn, st: lib.mural_op_adamw_amsgrad_flat_state(*ps, nn, st, 0.9, 0.999, 1e-8, 0.0, None)            # noqa: E731
        bad = [(ptr, n - 1), (ptr, n + 2)]
        bad += [([q + 4 if i == j else q for i, q in enumerate(ptr)], n) for j in range(len(ptr))]
        bad += [([None if i == j else q for i, q in enumerate(ptr)], n) for j in range(len(ptr))]
        for ps, nn in bad:
            _refused(lambda: host(ps, nn, LR), which)
            _refused(lambda: dev(ps, nn, state.data_ptr()), which)
        _refused(lambda: host(ptr, n, -LR), which)
        _refused(lambda: dev(ptr, n, None), which)
        torch.cuda.synchronize()
        for t, t0 in zip(bufs, before):
            assert torch.equal(_bits(t), _bits(t0)), which
        assert np.isfinite(float(bufs[0].sum()))
