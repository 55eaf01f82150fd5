"""What the flat AdamW / SGD steps need to hold without a GPU: the library exports their entries in both flavours, and
``make_optimizer`` hands out the torch classes, which step through torch on CPU parameters."""
import copy
import subprocess

import pytest
import torch

ENTRIES = ("mural_op_adamw_amsgrad_flat", "mural_op_adamw_amsgrad_flat_state", "mural_op_sgd_flat", "mural_op_sgd_flat_state")
TORCH_CLASS = {"Adam": torch.optim.Adam, "AdamW": torch.optim.AdamW, "AdamW2": torch.optim.AdamW, "SGD": torch.optim.SGD}


def test_both_flavours_export_the_flat_optimiser_entries():
    from mural_amd import _lib
    for path in (_lib.LIB_PATH, _lib.DEBUG_LIB_PATH):
        out = subprocess.run(["nm", "-D", "--defined-only", path], capture_output=True, text=True, check=True).stdout
        defined = {ln.split()[-1] for ln in out.splitlines() if ln.strip()}
        assert set(ENTRIES) <= defined, (path, set(ENTRIES) - defined)
    assert set(ENTRIES) <= set(_lib.PROTOTYPES)


@pytest.mark.parametrize("name", sorted(TORCH_CLASS))
def test_make_optimizer_returns_the_torch_classes_and_they_step_on_the_cpu(name):
    from mural_amd import train as TR
    lin = torch.nn.Linear(3, 2)
    model, twin = copy.deepcopy(lin), copy.deepcopy(lin)
    config = dict(optim=name, learning_rate=1e-2, weight_decay=1e-3)
    opt = TR.make_optimizer(config, model.parameters(), device_state=None)
    assert isinstance(opt, TORCH_CLASS[name]) and isinstance(opt, getattr(TR, "AdamW" if name == "AdamW2" else name))
    assert opt.device_state is None and opt.defaults["lr"] == 1e-2 and opt.defaults["weight_decay"] == 1e-3
    kw = dict(SGD=dict(momentum=0.98, nesterov=True), Adam={}).get(name, dict(amsgrad=True))
    assert all(opt.defaults[k] == v for k, v in kw.items())
    ref = TORCH_CLASS[name](twin.parameters(), lr=1e-2, weight_decay=1e-3, **kw)
    x = torch.arange(12.0).view(4, 3)
    for _ in range(2):
        for m, o in ((model, opt), (twin, ref)):
            o.zero_grad()
            m(x).square().sum().backward()
            o.step()
    assert opt._flat is None                                   # no HIP model behind these parameters: torch's own step
    for p, q in zip(model.parameters(), twin.parameters()):
        assert torch.equal(p, q)
    ref.load_state_dict(opt.state_dict())


def test_make_optimizer_still_refuses_an_unknown_name():
    from mural_amd import train as TR
    with pytest.raises(ValueError, match="unsupported optimization method"):
        TR.make_optimizer(dict(optim="RMSprop", learning_rate=1e-3, weight_decay=0.0), torch.nn.Linear(2, 2).parameters())
