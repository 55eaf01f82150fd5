"""The flat-gradient layout and the parameter-struct fillers of mural_amd/model/step_layout.py on CPU models: the training layout
and the eval-path fill put the same tensors into the same pointer slots, the structs carry the addresses they should, the gradient
offsets tile one flat buffer, and the two cache / registry policies (SNV: registered, no identity check; INDEL: identity check, not
registered) hold.  No GPU here: nothing is launched, the structs are only built and read back."""
import ctypes as C

import numpy as np
import pytest
import torch

CASES = ["net0", "net1", "net2", "unet_rev", "unet_norev"]


def _build(case):
    from mural_amd.model import model_choice
    if case.startswith("unet"):
        cfg = dict(CNN_out_channels=8, CNN_kernel_size=3, down_list=[2, 2, 2, 5, 5, 5], use_reverse=case == "unet_rev")
        model = model_choice(0, cfg, dict(n_class=3), "indel")
    else:
        r, R = 7, 200
        cfg = dict(local_radius=r, local_order=3, local_hidden1_size=150, local_hidden2_size=75, distal_radius=R, emb_dropout=0.1,
                   local_dropout=0.1, CNN_kernel_size=3, CNN_out_channels=32, distal_fc_dropout=0.25)
        common = dict(emb_dims=[(65, 2)] * (2 * r + 1 - 2), n_cont=0, n_class=4, distal_order=1, in_channels=4)
        model = model_choice(int(case[-1]), cfg, common, "snv")
    with torch.no_grad():      # tensor i holds values of [i + 1, i + 2): no two tensors share a value
        for i, t in enumerate(list(model.parameters()) + list(model.buffers())):
            n = t.numel()
            if t.is_floating_point():
                t.copy_((i + 1 + torch.arange(n, dtype=torch.float64) / (n + 1)).reshape(t.shape))
            else:
                t.fill_(i + 1)
    return model


class _Case:
    def __init__(self, case):
        from mural_amd.model import indel_train_step, train_step
        self.model = _build(case)
        self.indel = case.startswith("unet")
        self.step_model = self.model.model if case == "net0" else self.model      # Network0 wraps the module that trains
        self.layout_of = (indel_train_step if self.indel else train_step)._layout
        self.lay = self.layout_of(self.step_model)
        if self.indel:
            self.keep = []
            eval_struct = self.step_model._params(self.keep)
        else:
            _, eval_struct, hp = self.step_model._shape_and_params()
            self.keep = hp.keep
        self.eval_raw = np.frombuffer(bytes(eval_struct), dtype=np.int64).tolist()


@pytest.fixture(scope="module", params=CASES)
def case(request):
    return _Case(request.param)


def _raw(struct):
    return np.frombuffer(bytes(struct), dtype=np.int64).tolist()


def test_layout_and_eval_fill_put_the_same_tensors_into_the_same_slots(case):
    host = {a.ctypes.data: a for a in case.keep}
    assert len(case.eval_raw) == len(case.lay.slot_tensor) == C.sizeof(case.lay.struct_type) // 8
    filled = 0
    for s, (addr, t) in enumerate(zip(case.eval_raw, case.lay.slot_tensor)):
        assert (addr == 0) == (t is None), f"slot {s}"
        if t is not None:
            filled += 1
            a = host[addr]
            assert a.shape == tuple(t.shape) and np.array_equal(a, t.detach().numpy()), f"slot {s}"
    floats = [t for t in list(case.step_model.parameters()) + list(case.step_model.buffers()) if t.is_floating_point() and t.numel()]
    assert filled == len(floats)      # every non-empty float tensor of the model sits in exactly one slot
    assert len({id(t) for t in case.lay.slot_tensor if t is not None}) == filled


def test_params_struct_carries_the_tensors_addresses(case):
    raw = _raw(case.lay.params_struct())
    for s, t in enumerate(case.lay.slot_tensor):
        assert raw[s] == (0 if t is None else t.data_ptr()), f"slot {s}"


def test_grads_struct_points_into_the_flat_buffer(case):
    lay, base = case.lay, 1 << 32
    off = {id(p): o for p, o in zip(lay.plist, lay.poffs)}
    raw = _raw(lay.grads_struct(base))
    n_param_slots = 0
    for s, t in enumerate(lay.slot_tensor):
        if t is not None and id(t) in off:
            n_param_slots += 1
            assert raw[s] == base + 4 * off[id(t)], f"slot {s}"
        else:
            assert raw[s] == 0, f"slot {s}: running statistics and unused slots have no gradient"
    assert n_param_slots == len(lay.plist)


def test_gradient_offsets_tile_one_flat_buffer(case):
    lay = case.lay
    assert [id(p) for p in lay.plist] == [id(p) for p in case.step_model.parameters() if p.numel()]
    end = 0
    for p, o in zip(lay.plist, lay.poffs):
        assert o % 64 == 0 and o >= end
        end = o + p.numel()
    assert lay.total == (end + 63) // 64 * 64 and lay.total % 64 == 0
    assert sum(v.numel() for v in lay.grad_views(torch.zeros(lay.total))) == sum(p.numel() for p in lay.plist)


def test_registry_serves_snv_layouts_only(case):
    from mural_amd.model.step_layout import layout_of_params
    from mural_amd.model.train_step import layout_of_params as from_train_step
    assert from_train_step is layout_of_params
    found = layout_of_params(list(case.model.parameters()))
    assert found is (None if case.indel else case.lay)


def test_cached_layout_identity_policy(case):
    assert case.layout_of(case.step_model) is case.lay
    if not case.indel:
        return
    model = _build("unet_rev")
    from mural_amd.model.indel_train_step import _layout
    first = _layout(model)
    assert _layout(model) is first
    conv = model.uplblocks[0][0]
    conv.weight = torch.nn.Parameter(conv.weight.detach().clone())
    second = _layout(model)
    assert second is not first and any(t is conv.weight for t in second.slot_tensor)
