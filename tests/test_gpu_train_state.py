"""The training loop's step state on the device (csrc/train_state.hip, mural_amd.train.DeviceStepState): the tick kernel against the host
expressions and the host mirror of its scheduler, Adam(device_state=...) against torch.optim.Adam on a shadow copy, the step replayed as
a HIP graph with a moving step count and a scheduled rate, and train_epoch_device against train_epoch."""
import functools
import math

import numpy as np
import pytest
import torch
import torch.nn as nn

from tests import _util as U
from tests.test_gpu_snv import product_from_hp
from tests.test_train_state_host import STEPLR

pytestmark = pytest.mark.gpu

BETAS = (0.9, 0.999)
# (5000 * 128) // 320000 == 2: the rate halves every second step, falls below min_lr at the fourth tick and restarts there (once in 6 steps)
STEP2 = dict(lr_scheduler="StepLR", batch_size=320000, LR_gamma=0.5, min_lr=3e-4, restart_lr=1e-3, learning_rate=1e-3)


@functools.lru_cache(maxsize=None)
def fixture():
    fx = U.load("snv_train_T.npz")
    return (fx, torch.from_numpy(fx["cat"]).cuda(), U.onehot(fx["codes"]).cuda(), torch.from_numpy(fx["y"]).cuda(),
            torch.zeros(len(fx["cat"]), 1, device="cuda"))


def make_model(fx, dropout=True):
    model, _ = product_from_hp(fx["hp"])
    model.load_state_dict(U.snv_state_for(fx, U.snv_oracle_from_hp(fx["hp"])))
    if not dropout:
        for m in model.modules():
            if isinstance(m, nn.Dropout):
                m.p = 0.0
    return model.cuda().train()


def bound(lr):
    """The existing flat-Adam test's bar (2e-7 at lr 1e-3: an update is lr-sized, a rounding of it 1e-10), scaled with a larger rate."""
    return 2e-7 * max(lr, 1e-3) / 1e-3


def assert_same(params, shadow, names, lr, what):
    for k, a, b in zip(names, params, shadow):
        d = float((a.detach() - b.detach()).abs().max())
        assert d <= bound(lr), (what, k, d)


def test_tick_factors_scheduler_and_loss_sum():
    from mural_amd.train import DeviceStepState
    lr = 1e-3
    st = DeviceStepState("cuda", lr, BETAS)
    # the two floats the Adam kernel consumes: within 1 float ulp of mural_op_adam_flat's host expressions in double (a double pow is off
    # by a few double ulps, which can move the rounding to float by at most one step)
    for step in (1, 2, 3, 10, 1000, 100000):
        st.set_step(step - 1)
        st.tick()
        r = st.read()
        want_ss = np.float32(lr / (1.0 - BETAS[0] ** step))
        want_bc = np.float32(math.sqrt(1.0 - BETAS[1] ** step))
        print(f"[train_state] step {step}: step_size {r['step_size']!r} (host {float(want_ss)!r}), bc2_sqrt {r['bc2_sqrt']!r} (host {float(want_bc)!r})")
        assert r["step"] == step and r["lr"] == lr
        assert abs(np.float32(r["step_size"]) - want_ss) <= np.spacing(want_ss), (step, r["step_size"], want_ss)
        assert abs(np.float32(r["bc2_sqrt"]) - want_bc) <= np.spacing(want_bc), (step, r["bc2_sqrt"], want_bc)
    # forty ticks of the StepLR config (every third tick, restart below min_lr): lr, ticks, step equal the host mirror and the counts
    st = DeviceStepState("cuda", lr, BETAS)
    assert st.set_schedule(STEPLR) == (3, 0.5, 1e-4, 8e-4)
    want = DeviceStepState.lr_sequence(STEPLR, lr, 41)
    losses = torch.from_numpy(np.random.default_rng(3).uniform(0.5, 90.0, size=40).astype(np.float32)).cuda()
    total = 0.0
    for i in range(40):
        st.observe(losses[i], 5)
        st.tick()
        total += float(losses[i].item())
        r = st.read()
        assert r["lr"] == want[i + 1] and r["ticks"] == i + 1 and r["step"] == i + 1, (i, r, want[i + 1])
        ss = np.float32(want[i] / (1.0 - BETAS[0] ** (i + 1)))      # from the rate BEFORE this tick's scheduler
        assert abs(np.float32(r["step_size"]) - ss) <= np.spacing(ss), (i, r["step_size"], ss)
    assert len(set(want)) > 4 and want.count(8e-4) >= 2          # the restart fired
    assert r["loss_sum"] == total and r["rows"] == 200 and r["steps_done"] == 40
    st.reset_epoch()
    st.tick()                                                     # (no loss observed: the sum and the rows stay)
    r = st.read()
    assert (r["loss_sum"], r["rows"], r["steps_done"], r["step"], r["ticks"]) == (0.0, 0, 1, 41, 41)
    st.set_lr(0.25)
    assert st.read()["lr"] == 0.25
    with pytest.raises(ValueError, match="float32 scalar"):
        st.observe(torch.zeros((), dtype=torch.float64, device="cuda"), 1)


def test_adam_with_device_state_matches_torch_adam_and_falls_back():
    """The shadow-copy scheme of test_flat_adam_matches_torch_adam_and_falls_back with a schedule active: the shadow's rate is set from
    lr_sequence before every step."""
    from mural_amd.train import Adam, DeviceStepState, clip_grad_norm_
    fx, cat, x, y, cont = fixture()
    crit = nn.CrossEntropyLoss(reduction="sum")
    seq = DeviceStepState.lr_sequence(STEP2, 1e-3, 7)
    assert seq[:6] == [1e-3, 1e-3, 5e-4, 5e-4, 1e-3, 1e-3]          # halved at tick 2, restarted at tick 4
    for wd in (0.0, 1e-2):
        model = make_model(fx)
        params = [p for p in model.parameters() if p.numel()]
        shadow = [p.detach().clone().requires_grad_() for p in params]
        names = [k for k, p in model.named_parameters() if p.numel()]
        state = DeviceStepState("cuda", 1e-3, BETAS)
        state.set_schedule(STEP2)
        opt = Adam(model.parameters(), lr=1e-3, weight_decay=wd, device_state=state)
        ref = torch.optim.Adam(shadow, lr=1e-3, weight_decay=wd, fused=True)

        def one_step(t, spoil=False):
            torch.manual_seed(10 + t)
            loss = crit(model((cont, cat), x), y)
            opt.zero_grad()
            loss.backward()
            clip_grad_norm_(model, 10)
            if spoil:
                w = model.conv1_2[1].weight
                w.grad = w.grad.clone()
            for p, q in zip(params, shadow):
                q.grad = p.grad.detach().clone()
            ref.param_groups[0]["lr"] = seq[t]
            state.observe(loss, len(y))
            opt.step()
            ref.step()
            assert_same(params, shadow, names, seq[t], (wd, t))

        for t in range(4):
            one_step(t)
        # the block counted, not the host: the block-free launch never ran
        assert opt._flat is not None and opt._flat_t == 0 and state.read()["step"] == 4
        one_step(4, spoil=True)          # a gradient that is not the backward's view: torch's own step, on the block's count and rate
        assert opt._flat is None and opt._flat_t == 4 and opt.param_groups[0]["lr"] == seq[4]
        assert all(float(opt.state[p]["step"]) == 5.0 for p in params)
        one_step(5)
        assert opt._flat is not None
        r = state.read()
        assert r["step"] == 6 and r["ticks"] == 6 and r["steps_done"] == 6 and r["rows"] == 6 * len(y) and r["lr"] == seq[6]
        assert all(float(st["step"]) == 6.0 for st in opt.state_dict()["state"].values())


def shadow_of(opt, params):
    """torch.optim.Adam(fused=True) on clones of `params` with clones of opt's moments and its step count."""
    shadow = [p.detach().clone().requires_grad_() for p in params]
    ref = torch.optim.Adam(shadow, lr=1e-3, fused=True)
    opt.state_dict()                                     # (materialises the step counters from the block)
    for p, q in zip(params, shadow):
        ref.state[q] = {k: opt.state[p][k].detach().clone() for k in ("step", "exp_avg", "exp_avg_sq")}
    return shadow, ref


def test_replayed_step_reads_step_and_rate_from_the_device():
    """GraphedTrainStep on Adam(device_state=...): after each replay the shadow (moments and step count taken over after the three warm-up
    steps) is stepped with the gradients the replay left in p.grad, at the rate lr_sequence gives -- a graph that replayed the captured
    step count or rate would miss the bar at the first replay (another bias correction) and at the third (a rate halved)."""
    from mural_amd.train import Adam, DeviceStepState, GraphedTrainStep
    fx, cat, x, y, cont = fixture()
    B = len(y)
    crit = nn.CrossEntropyLoss(reduction="sum")
    model = make_model(fx, dropout=False)
    params = [p for p in model.parameters() if p.numel()]
    names = [k for k, p in model.named_parameters() if p.numel()]
    state = DeviceStepState("cuda", 1e-3, BETAS)
    state.set_schedule(STEP2)
    opt = Adam(model.parameters(), lr=1e-3, device_state=state)
    step = GraphedTrainStep(model, opt, crit, cont, cat, x, y)
    assert opt._flat is not None
    seq = DeviceStepState.lr_sequence(STEP2, 1e-3, 8)
    shadow, ref = shadow_of(opt, params)
    assert all(float(st["step"]) == 3.0 for st in ref.state.values())
    assert_same(params, shadow, names, 1e-3, "taken over")
    for i in range(4):
        step(cont, cat, x, y)
        for p, q in zip(params, shadow):
            q.grad = p.grad.detach().clone()
        ref.param_groups[0]["lr"] = seq[3 + i]
        ref.step()
        assert_same(params, shadow, names, seq[3 + i], ("replay", i))
    step.finish()
    r = state.read()
    assert r["step"] == 3 + 4 and r["ticks"] == 7 and r["lr"] == seq[7] and r["rows"] == 7 * B and r["steps_done"] == 7
    assert len(set(seq[3:7])) > 1                                      # the rate moved between the replays


def test_train_epoch_device_matches_train_epoch():
    from mural_amd.train import Adam, DeviceStepState, make_scheduler, train_epoch, train_epoch_device
    fx, cat, x, y, cont = fixture()
    B = len(y)
    # StepLR2 with train_size // batch_size == 4: the rate decays every batch and restarts after the fifth
    cfg = dict(lr_scheduler="StepLR2", batch_size=B, LR_gamma=0.5, min_lr=1e-4, restart_lr=1e-3, learning_rate=1e-3)
    train_size = 4 * B + B // 2

    def rows(idx):
        return y[idx], cont[idx], cat[idx], x[idx]

    g = torch.Generator().manual_seed(4)
    batches = [rows(torch.randperm(B, generator=g).cuda()) for _ in range(8)]
    batches.insert(2, rows(torch.tensor([7]).cuda()))                  # one row: skipped
    batches.insert(5, rows(torch.randperm(B, generator=g)[:B // 2].cuda()))      # half size: the same kernels, eagerly
    crit = nn.CrossEntropyLoss(reduction="sum")
    eager = make_model(fx, dropout=False)
    opt_e = torch.optim.Adam(eager.parameters(), lr=1e-3)
    want = train_epoch(eager, batches, crit, opt_e, make_scheduler(cfg, opt_e, train_size), cfg, "cuda")
    model = make_model(fx, dropout=False)
    opt = Adam(model.parameters(), lr=1e-3, device_state=DeviceStepState("cuda", 1e-3, BETAS))
    got = train_epoch_device(model, batches, crit, opt, cfg, "cuda", train_size=train_size)
    r = opt.device_state.read()
    print(f"[train_state] epoch loss: device {got!r}, eager {want!r}; lr {r['lr']!r} / {opt_e.param_groups[0]['lr']!r}")
    assert abs(got - want) <= 1e-3 * abs(want)
    assert r["steps_done"] == 9 and r["rows"] == 8 * B + B // 2 and r["step"] == 9
    assert opt.param_groups[0]["lr"] == opt_e.param_groups[0]["lr"] == r["lr"]
    assert opt.param_groups[0]["lr"] == DeviceStepState.lr_sequence(cfg, 1e-3, 10, train_size)[9] != 1e-3
    steps = model._device_epoch_steps
    assert list(steps) == [B]                                           # one graph; the half-size batch ran eagerly
    first = steps[B][0]
    # the next epoch replays the same graph; StepLR2 starts it at restart_lr
    got2 = train_epoch_device(model, batches[:2], crit, opt, cfg, "cuda", epoch=1, train_size=train_size)
    assert model._device_epoch_steps[B][0] is first and math.isfinite(got2) and got2 > 0
    r = opt.device_state.read()
    assert r["steps_done"] == 2 and r["step"] == 11 and r["lr"] == DeviceStepState.lr_sequence(cfg, 1e-3, 3, train_size, ticks0=9)[2]
    # refusals name the loop that takes the case
    hp = np.array(fx["hp"]).copy()
    hp[5] = 16                                                          # CNN_out_channels != 32: the per-layer path
    other, _ = product_from_hp(hp)
    other = other.cuda().train()
    with pytest.raises(ValueError, match="use train_epoch"):
        train_epoch_device(other, batches, crit, Adam(other.parameters(), device_state=DeviceStepState("cuda", 1e-3, BETAS)), cfg, "cuda")
    with pytest.raises(ValueError, match="use train_epoch"):
        train_epoch_device(model, batches, crit, torch.optim.Adam(model.parameters()), cfg, "cuda")
    with pytest.raises(ValueError, match="use train_epoch"):
        train_epoch_device(model, batches, nn.MSELoss(), opt, cfg, "cuda")


def test_replayed_step_takes_symbol_windows():
    """The SNV GraphedTrainStep on the form EpochLoader yields: a static uint8 tensor, the same loss as the dense form of the same windows."""
    from mural_amd.data import SymbolWindows
    from mural_amd.model import train_ops as T
    from mural_amd.train import Adam, DeviceStepState, GraphedTrainStep
    fx, cat, x, y, cont = fixture()
    crit = nn.CrossEntropyLoss(reduction="sum")
    sym = SymbolWindows(T.dense_to_symbols(x))
    T.flush_input_checks()
    losses = []
    for distal in (x, sym):
        model = make_model(fx, dropout=False)
        opt = Adam(model.parameters(), lr=1e-3, device_state=DeviceStepState("cuda", 1e-3, BETAS))
        step = GraphedTrainStep(model, opt, crit, cont, cat, distal, y)
        loss = step(cont, cat, distal, y)
        step.finish()
        losses.append(float(loss.item()))
        assert opt.device_state.read()["step"] == 4
    assert step.x.dtype is torch.uint8 and tuple(step.x.shape) == tuple(sym.sym.shape)
    assert abs(losses[0] - losses[1]) <= 1e-3 * abs(losses[0])


def test_default_path_is_untouched():
    """Adam(...) without device_state: the host counts the updates and mural_op_adam_flat is the launch (the attributes the existing test reads)."""
    from mural_amd.train import Adam, clip_grad_norm_
    fx, cat, x, y, cont = fixture()
    crit = nn.CrossEntropyLoss(reduction="sum")
    model = make_model(fx)
    params = [p for p in model.parameters() if p.numel()]
    shadow = [p.detach().clone().requires_grad_() for p in params]
    names = [k for k, p in model.named_parameters() if p.numel()]
    opt = Adam(model.parameters(), lr=1e-3)
    ref = torch.optim.Adam(shadow, lr=1e-3, fused=True)
    assert opt.device_state is None and opt._flat_t == 0
    torch.manual_seed(1)
    loss = crit(model((cont, cat), x), y)
    opt.zero_grad()
    loss.backward()
    clip_grad_norm_(model, 10)
    for p, q in zip(params, shadow):
        q.grad = p.grad.detach().clone()
    opt.step()
    ref.step()
    assert opt._flat is not None and opt._flat_t == 1
    assert_same(params, shadow, names, 1e-3, "default")
    assert all(float(st["step"]) == 1.0 for st in opt.state_dict()["state"].values())
