"""The host mirror of the device step state's scheduler (mural_amd.train.DeviceStepState.lr_sequence / .schedule) against a real torch
loop: torch.optim.Adam + make_scheduler(config, opt) stepped per batch with train_epoch's restart rule.  Equal with ==, not close: the
tick kernel performs the same double operations in the same order (tests/test_gpu_train_state.py compares it with this mirror)."""
import pytest
import torch

# (5000 * 128) // 213333 == 3: StepLR every third batch
STEPLR = dict(lr_scheduler="StepLR", batch_size=213333, LR_gamma=0.5, min_lr=1e-4, restart_lr=8e-4, learning_rate=1e-3)
# train_size // batch_size == 7: per-batch decay from restart_lr to min_lr over seven batches
STEPLR2 = dict(lr_scheduler="StepLR2", batch_size=10, LR_gamma=0.5, min_lr=1e-4, restart_lr=1e-3, learning_rate=1e-3)
ROP = dict(lr_scheduler="ROP", batch_size=128, LR_gamma=0.5, min_lr=1e-4, restart_lr=8e-4, learning_rate=1e-3)
CASES = [(STEPLR, None), (STEPLR2, 75), (ROP, None)]


def torch_loop(config, n, train_size=None):
    """(the learning rate of each of n optimizer steps, the number of restarts) of train_epoch's per-batch policy."""
    from mural_amd.train import make_scheduler
    p = torch.nn.Parameter(torch.zeros(1))
    opt = torch.optim.Adam([p], lr=config["learning_rate"])
    sched = make_scheduler(config, opt, train_size)
    lrs, restarts = [], 0
    for _ in range(n):
        p.grad = torch.ones(1)
        lrs.append(opt.param_groups[0]["lr"])
        opt.step()
        if config["lr_scheduler"] != "ROP":
            sched.step()
            if opt.param_groups[0]["lr"] < config["min_lr"]:
                restarts += 1
                for g in opt.param_groups:
                    g["lr"] = config["restart_lr"]
    return lrs, restarts


@pytest.mark.parametrize("config,train_size", CASES, ids=[c["lr_scheduler"] for c, _ in CASES])
def test_lr_sequence_equals_the_torch_loop(config, train_size):
    from mural_amd.train import DeviceStepState
    want, restarts = torch_loop(config, 40, train_size)
    got = DeviceStepState.lr_sequence(config, config["learning_rate"], 40, train_size)
    assert got == want
    if config["lr_scheduler"] == "ROP":
        assert restarts == 0 and got == [config["learning_rate"]] * 40
    else:
        assert restarts >= 2 and len(set(got)) > 3


def test_schedule_maps_the_reference_config():
    from mural_amd.train import DeviceStepState
    assert DeviceStepState.schedule(STEPLR) == (3, 0.5, 1e-4, 8e-4)
    assert DeviceStepState.schedule(dict(STEPLR, batch_size=128)) == (5000, 0.5, 1e-4, 8e-4)
    assert DeviceStepState.schedule(STEPLR2, 75) == (1, (1e-4 / 1e-3) ** (1 / 7), 1e-4, 1e-3)
    k, gamma, min_lr, _ = DeviceStepState.schedule(ROP)
    assert (k, gamma) == (0, 1.0) and not 0.0 < min_lr           # no per-batch scheduler, no restart rule
    with pytest.raises(ValueError, match="unknown lr_scheduler cosine"):
        DeviceStepState.schedule(dict(STEPLR, lr_scheduler="cosine"))
    # a block that has ticked before carries on where it stood
    seq = DeviceStepState.lr_sequence(STEPLR, 1e-3, 12)
    assert DeviceStepState.lr_sequence(STEPLR, seq[5], 7, ticks0=5) == seq[5:]
