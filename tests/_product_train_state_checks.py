"""Run by tests/test_product_train_state.py in a subprocess WITHOUT MURAL_HIP_FLAVOR: Adam(device_state=...) through the product library
(libmural_hip.so) -- two steps of the shadow-copy check of tests/test_gpu_train_state.py with the schedule active."""
import ctypes
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    import torch
    import torch.nn as nn
    from mural_amd import _lib
    from mural_amd.train import Adam, DeviceStepState, clip_grad_norm_
    from tests import test_gpu_train_state as G
    assert _lib.flavor() == "product"
    handle = ctypes.CDLL(_lib.LIB_PATH)
    assert hasattr(handle, "mural_op_train_state_tick") and hasattr(handle, "mural_op_adam_flat_state")
    assert _lib.lib()._name == _lib.LIB_PATH
    fx, cat, x, y, cont = G.fixture()
    crit = nn.CrossEntropyLoss(reduction="sum")
    config = dict(G.STEP2, batch_size=640000)          # step_size 1: the second step runs at half the rate
    seq = DeviceStepState.lr_sequence(config, 1e-3, 3)
    assert seq == [1e-3, 5e-4, 1e-3]
    model = G.make_model(fx)
    params = [p for p in model.parameters() if p.numel()]
    shadow = [p.detach().clone().requires_grad_() for p in params]
    names = [k for k, p in model.named_parameters() if p.numel()]
    state = DeviceStepState("cuda", 1e-3, G.BETAS)
    state.set_schedule(config)
    opt = Adam(model.parameters(), lr=1e-3, weight_decay=1e-2, device_state=state)
    ref = torch.optim.Adam(shadow, lr=1e-3, weight_decay=1e-2, fused=True)
    for t in range(2):
        torch.manual_seed(10 + t)
        loss = crit(model((cont, cat), x), y)
        opt.zero_grad()
        loss.backward()
        clip_grad_norm_(model, 10)
        for p, q in zip(params, shadow):
            q.grad = p.grad.detach().clone()
        ref.param_groups[0]["lr"] = seq[t]
        state.observe(loss, len(y))
        opt.step()
        ref.step()
        G.assert_same(params, shadow, names, seq[t], t)
    r = state.read()
    assert opt._flat is not None and opt._flat_t == 0 and r["step"] == 2 and r["lr"] == seq[2] and r["rows"] == 2 * len(y)
    print("PRODUCT_TRAIN_STATE_OK")


if __name__ == "__main__":
    main()
