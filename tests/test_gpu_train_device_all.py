"""The device-state training loop beyond Adam on an SNV model: mural_amd.train.AdamW / SGD (the one-launch steps of
mural_op_adamw_amsgrad_flat / mural_op_sgd_flat) against the torch classes on shadow copies, train_epoch_device with each of them, and
UNet_Small on the flat step -- direct gradients, the two-launch clip, train_epoch_device(model_type="indel") on dense and symbol windows.

Bars: parameters by ``_loose`` of tests/_parity.py (8 x the distance of the torch class in float32 from the torch class in float64, both
stepped on copies with the same gradients; at least 4 ulp); epoch losses 1e-3 relative, the bar tests/test_gpu_train_state.py holds with
dropout off; learning rates with ``==``."""
import copy

import numpy as np
import pytest
import torch
import torch.nn as nn

from tests import _loader_data as D
from tests import test_gpu_train_state as G
from tests._parity import _Stats, _loose
from tests.test_gpu_indel_train_symbols import DOWN

pytestmark = pytest.mark.gpu

TORCH_CLASS = {"AdamW": torch.optim.AdamW, "SGD": torch.optim.SGD}
KW = {"AdamW": dict(amsgrad=True), "SGD": dict(momentum=0.98, nesterov=True)}


def _config(optim, **kw):
    return dict(optim=optim, learning_rate=1e-3, weight_decay=1e-2, **kw)


def _snv_step(model, crit, opt, batch, seed):
    from mural_amd.train import clip_grad_norm_
    fx, cat, x, y, cont = batch
    torch.manual_seed(seed)
    loss = crit(model((cont, cat), x), y)
    opt.zero_grad()
    loss.backward()
    clip_grad_norm_(model, 10)
    return loss


@pytest.mark.parametrize("optim", ["AdamW", "SGD"])
@pytest.mark.parametrize("on_device", [False, True], ids=["host_count", "device_state"])
def test_flat_optimisers_match_the_torch_classes_on_shadow_copies(optim, on_device):
    """Three eager steps: the same gradients go to this module's optimiser (on the model), to the torch class on a float32 copy of the
    parameters and to the torch class on a float64 copy.  With a device state the schedule halves the rate at the second tick, and the
    copies are given the rate of tests' host mirror before every step (SGD: the update runs at the rate the previous tick left; AdamW
    runs without decay there: its decoupled decay takes the rate AFTER the tick, see mural_amd.train.AdamW)."""
    from mural_amd.train import DeviceStepState, make_optimizer
    batch = G.fixture()
    crit = nn.CrossEntropyLoss(reduction="sum")
    model = G.make_model(batch[0])
    params = [p for p in model.parameters() if p.numel()]
    names = [k for k, p in model.named_parameters() if p.numel()]
    wd = 0.0 if (on_device and optim == "AdamW") else 1e-2
    state = None
    seq = [1e-3] * 4
    if on_device:
        state = DeviceStepState("cuda", 1e-3, G.BETAS)
        state.set_schedule(G.STEP2)
        seq = DeviceStepState.lr_sequence(G.STEP2, 1e-3, 4)
        assert seq == [1e-3, 1e-3, 5e-4, 5e-4]
    opt = make_optimizer(dict(_config(optim), weight_decay=wd), model.parameters(), device_state=state)
    assert isinstance(opt, TORCH_CLASS[optim])
    shadow32 = [p.detach().clone().requires_grad_() for p in params]
    shadow64 = [p.detach().double().clone().requires_grad_() for p in params]
    ref32 = TORCH_CLASS[optim](shadow32, lr=1e-3, weight_decay=wd, **KW[optim])
    ref64 = TORCH_CLASS[optim](shadow64, lr=1e-3, weight_decay=wd, **KW[optim])
    for t in range(3):
        loss = _snv_step(model, crit, opt, batch, 10 + t)
        for p, q, r in zip(params, shadow32, shadow64):
            q.grad = p.grad.detach().clone()
            r.grad = p.grad.detach().double()
        for ref in (ref32, ref64):
            ref.param_groups[0]["lr"] = seq[t]
            ref.step()
        if on_device:
            state.observe(loss, len(batch[3]))
        opt.step()
    assert opt._flat is not None, "the one-launch step did not run"
    stats = _Stats(f"{optim} x3", tag="train_device_all")
    for k, a, r, w in zip(names, params, shadow32, shadow64):
        _loose(a, w.detach().cpu(), r.detach().cpu(), k, f"{optim} {'device state' if on_device else 'host count'}", stats)
    stats.show()
    if on_device:
        r = state.read()
        assert r["step"] == 3 and r["ticks"] == 3 and r["lr"] == seq[3] and r["rows"] == 3 * len(batch[3])
    # state_dict() round-trips into the plain torch class
    sd = opt.state_dict()
    held = opt.param_groups[0]["params"]          # (parameters without elements included: they have no slot and no state)
    plain = TORCH_CLASS[optim]([p.detach().clone().requires_grad_() for p in held], lr=1e-3, weight_decay=wd, **KW[optim])
    plain.load_state_dict(copy.deepcopy(sd))
    assert len(plain.state) == len(params)
    for q, p in zip(plain.param_groups[0]["params"], held):
        for key, val in opt.state.get(p, {}).items():
            assert torch.equal(plain.state[q][key].cpu(), val.detach().cpu()), (optim, key)
        if optim == "AdamW" and p.numel():
            assert float(plain.state[q]["step"]) == 3.0
    assert opt._flat is not None                  # (reading the state left the flat layout in place)


@pytest.mark.parametrize("optim", ["AdamW", "SGD"])
def test_train_epoch_device_with_each_optimiser(optim):
    from mural_amd.train import DeviceStepState, make_optimizer, make_scheduler, train_epoch, train_epoch_device
    fx, cat, x, y, cont = G.fixture()
    B = len(y)
    cfg = _config(optim, lr_scheduler="StepLR", batch_size=B, LR_gamma=0.5, min_lr=1e-4, restart_lr=1e-3)

    def rows(idx):
        return y[idx], cont[idx], cat[idx], x[idx]

    g = torch.Generator().manual_seed(4)
    batches = [rows(torch.randperm(B, generator=g).cuda()) for _ in range(4)]
    batches.insert(2, rows(torch.randperm(B, generator=g)[:B // 2].cuda()))      # half size: the same kernels, eagerly
    crit = nn.CrossEntropyLoss(reduction="sum")
    eager = G.make_model(fx, dropout=False)
    opt_e = make_optimizer(cfg, eager.parameters())
    want = train_epoch(eager, batches, crit, opt_e, make_scheduler(cfg, opt_e), cfg, "cuda")
    model = G.make_model(fx, dropout=False)
    opt = make_optimizer(cfg, model.parameters(), device_state=DeviceStepState("cuda", 1e-3, G.BETAS))
    got = train_epoch_device(model, batches, crit, opt, cfg, "cuda")
    r = opt.device_state.read()
    print(f"[train_device_all] {optim} epoch loss: device {got!r}, eager {want!r}; lr {r['lr']!r}")
    assert abs(got - want) <= 1e-3 * abs(want)
    assert r["steps_done"] == 5 and r["rows"] == 4 * B + B // 2 and r["step"] == 5
    assert opt.param_groups[0]["lr"] == DeviceStepState.lr_sequence(cfg, 1e-3, 6)[5] == opt_e.param_groups[0]["lr"]
    assert opt._flat is not None and list(model._device_epoch_steps) == [B]      # one graph; the half-size batch ran eagerly


# ------------------------------------------------------------------------------------------------------------------ UNet_Small
@pytest.fixture(scope="module")
def files(tmp_path_factory):
    return D.write_fixture(tmp_path_factory.mktemp("device_all"))


INDEL_CFG = dict(local_radius=D.R_LOCAL, local_order=D.ORDER, distal_radius=D.R_DISTAL, CNN_kernel_size=7, CNN_out_channels=8, down_list=DOWN,
                 use_reverse=True, n_class=4, model_no=0, optim="Adam", learning_rate=1e-3, weight_decay=1e-6, lr_scheduler="StepLR",
                 LR_gamma=0.9, batch_size=D.BATCH, min_lr=1e-7, restart_lr=1e-4)


def _unet():
    from mural_amd.model import model_choice, weights_init
    torch.manual_seed(0)
    m = model_choice(0, INDEL_CFG, dict(n_class=4), "indel")
    m.apply(weights_init)
    m = m.cuda().train()
    m.out_fc[1].p = 0.0
    return m


def _indel_batches(files, symbols):
    from mural_amd.data import EpochLoader, SymbolWindows
    loader = EpochLoader(*files, D.BATCH, D.R_LOCAL, D.ORDER, D.R_DISTAL, segment_center=D.SEGMENT, sampled_segments=D.SAMPLED,
                         model_type="indel", symbols=symbols)
    full = [b for b in loader.epoch(shuffle=True, generator=torch.Generator().manual_seed(3)) if b[0].shape[0] == D.BATCH]
    assert len(full) >= 3
    y, cont, cat, x = full[-1]
    h = D.BATCH // 2
    half = (y[:h], cont[:h], cat[:h], SymbolWindows(x.sym[:h].contiguous()) if symbols else x[:h].contiguous())
    return full[:2] + [half] + full[2:3]            # full, full, half-size carry batch, full


def _indel_step(model, x, y):
    loss = nn.CrossEntropyLoss(reduction="sum")(model(x), y.long().squeeze())
    model.zero_grad()
    loss.backward()
    return loss


def test_unet_small_gradients_are_views_of_one_flat_buffer_and_clip_in_two_launches(files):
    from mural_amd.train import Adam, DeviceStepState, clip_grad_norm_
    y, _, _, x = _indel_batches(files, symbols=False)[0]
    model = _unet()
    opt = Adam(model.parameters(), lr=1e-3, device_state=DeviceStepState("cuda", 1e-3))
    plain = Adam(model.parameters(), lr=1e-3)
    _indel_step(model, x, y)
    lay = model._train_layout
    assert lay.last_flat is not None and lay.own_flat is lay.last_flat
    base = lay.last_flat.data_ptr()
    offs = {id(p): o for p, o in zip(lay.plist, lay.poffs)}
    for k, p in model.named_parameters():
        assert p.grad is not None and p.grad.data_ptr() == base + 4 * offs[id(p)] and p.grad.shape == p.shape, k
        assert p.grad.untyped_storage().data_ptr() == lay.last_flat.untyped_storage().data_ptr(), k
    grads = [p.grad.detach().double().clone() for p in model.parameters()]
    want = float(torch.sqrt(sum((g * g).sum() for g in grads)))
    max_norm = 0.5 * want                                                          # (the clip scales)
    got = clip_grad_norm_(model, max_norm)
    assert got.shape == () and abs(float(got) - want) <= 2.0 ** -22 * want, (float(got), want)
    assert lay.clip_scratch is not None                                            # the library's two launches, not torch's foreach
    coef = max_norm / (want + 1e-6)
    for p, g in zip(model.parameters(), grads):
        assert float((p.grad.double() - coef * g).abs().max()) <= 2.0 ** -22 * float(g.abs().max()) + 1e-30
    before = [p.detach().clone() for p in model.parameters()]
    plain.step()                                                                   # without a device state: torch's step, as before
    assert plain._flat is None and any(not torch.equal(p, q) for p, q in zip(model.parameters(), before))
    opt.step()
    assert opt._flat is not None and opt._flat[0] is lay                           # on a device state: the one-launch step
    assert opt.device_state.read()["step"] == 1


@pytest.mark.parametrize("symbols", [False, True], ids=["dense", "symbols"])
def test_train_epoch_device_indel_matches_train_epoch(files, symbols):
    from mural_amd.train import DeviceStepState, make_optimizer, make_scheduler, train_epoch, train_epoch_device
    batches = _indel_batches(files, symbols)
    steps = len(batches)
    crit = nn.CrossEntropyLoss(reduction="sum")
    eager = _unet()
    opt_e = make_optimizer(INDEL_CFG, eager.parameters())
    want = train_epoch(eager, batches, crit, opt_e, make_scheduler(INDEL_CFG, opt_e), INDEL_CFG, "cuda", model_type="indel")
    model = _unet()
    opt = make_optimizer(INDEL_CFG, model.parameters(), device_state=DeviceStepState("cuda", 1e-3))
    got = train_epoch_device(model, batches, crit, opt, INDEL_CFG, "cuda", model_type="indel")
    r = opt.device_state.read()
    print(f"[train_device_all] indel {'symbols' if symbols else 'dense'} epoch loss: device {got!r}, eager {want!r}")
    assert np.isfinite(got) and abs(got - want) <= 1e-3 * abs(want)
    assert r["steps_done"] == steps and r["step"] == steps and r["rows"] == 3 * D.BATCH + D.BATCH // 2
    assert list(model._device_epoch_steps) == [D.BATCH]                            # one graph; the carry batch ran eagerly
    graphed = model._device_epoch_steps[D.BATCH][0]
    assert graphed.x.dtype is (torch.uint8 if symbols else torch.float32)
    assert int(model.conv[1].num_batches_tracked) == 2 * steps == int(eager.conv[1].num_batches_tracked)
    assert opt.param_groups[0]["lr"] == DeviceStepState.lr_sequence(INDEL_CFG, 1e-3, steps + 1)[steps] == opt_e.param_groups[0]["lr"]
    with pytest.raises(ValueError, match="use train_epoch"):                       # an SNV loop for a UNet_Small: refused
        train_epoch_device(model, batches, crit, opt, INDEL_CFG, "cuda")


def test_frozen_parameter_sends_the_indel_step_through_autograd(files):
    y, _, _, x = _indel_batches(files, symbols=False)[0]
    free = _unet()
    _indel_step(free, x, y)
    assert free._train_layout.own_flat is not None
    frozen = _unet()
    frozen.out_fc[2].bias.requires_grad_(False)
    _indel_step(frozen, x, y)
    lay = frozen._train_layout
    assert lay.own_flat is None and lay.last_flat is not None                      # autograd handed the gradients out, from a fresh buffer
    assert frozen.out_fc[2].bias.grad is None
    for (k, p), q in zip(frozen.named_parameters(), free.parameters()):
        if p.requires_grad:
            assert torch.equal(p.grad, q.grad), k
