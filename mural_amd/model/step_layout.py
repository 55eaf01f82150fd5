"""What the two one-call training steps (train_step.py: SNV, indel_train_step.py: INDEL) and the eval handles share on the host.

* The parameter-struct fillers: ONE walk of each model family's modules (``_HostParams`` for MuralSnvParams, ``fill_indel`` for
  MuralIndelParams).  What lands in a pointer slot is decided by the ``ptr`` callable: a host copy for the eval handle, a slot token for
  the training layout -- so training and eval cannot read different tensors.
* ``FlatGradLayout``: which tensor sits in which pointer slot, and where each parameter's gradient lives in ONE flat float32 buffer.
  ``mural_amd.train.clip_grad_norm_`` and ``mural_amd.train.Adam`` read its attributes.
* The lines the two ``ModelStep`` autograd nodes have in common (workspace and output allocation, BatchNorm counters, the
  one-backward rule) and their direct-gradient mode (train_step.py's docstring): when it is safe (``want_direct``), which buffer a
  backward writes (``backward_flat``) and how its slots become ``p.grad`` (``hand_out``).
"""
import ctypes as C
import os
import sys
import weakref

import numpy as np
import torch

from .. import _lib


# ---------------------------------------------------------------------------------------------------------------
# parameter hand-over to the C ABI
# ---------------------------------------------------------------------------------------------------------------
def host_copy_ptr(keep):
    """``ptr`` of the eval handles: a contiguous fp32 host copy, kept alive in `keep` while the C side reads it."""
    def ptr(t):
        a = np.ascontiguousarray(t.detach().to("cpu", torch.float32).numpy())
        keep.append(a)
        return a.ctypes.data_as(C.c_void_p)
    return ptr


class _HostParams:
    """Fills MuralSnvParams from a Network0 body / Network1 / Network2; by default with host copies it keeps alive."""

    def __init__(self, ptr=None):
        self.keep = []
        self.ptr = ptr if ptr is not None else host_copy_ptr(self.keep)

    def bn(self, m):
        return _lib.MuralBN(self.ptr(m.weight), self.ptr(m.bias), self.ptr(m.running_mean), self.ptr(m.running_var))

    def affine(self, m):
        return _lib.MuralAffine(self.ptr(m.weight), self.ptr(m.bias))

    def resblock(self, rb):
        return _lib.MuralResBlock(self.bn(rb.bn1), self.affine(rb.conv1), self.bn(rb.bn2), self.affine(rb.conv2))

    def tower(self, mod, sfx):
        g = lambda n: getattr(mod, n + sfx)
        fc = mod.distal_fc1 if sfx == "" else mod.distal_fc2
        t = _lib.MuralTower()
        t.bn_in, t.conv_in = self.bn(g("conv1")[0]), self.affine(g("conv1")[1])
        t.rbs1[0], t.rbs1[1] = self.resblock(g("RBs1")[0]), self.resblock(g("RBs1")[1])
        t.bn_mid, t.conv_mid = self.bn(g("conv2")[0]), self.affine(g("conv2")[1])
        t.rbs2[0], t.rbs2[1] = self.resblock(g("RBs2")[0]), self.resblock(g("RBs2")[1])
        t.bn_out, t.conv_out = self.bn(g("conv3")[0]), self.affine(g("conv3")[1])
        t.fc_bn, t.fc = self.bn(fc[0]), self.affine(fc[2])
        return t

    def local(self, mod, out_layer):
        l = _lib.MuralLocal()
        l.emb = self.ptr(mod.emb_layer.weight)
        l.lin[0], l.lin[1] = self.affine(mod.lin_layers[0]), self.affine(mod.lin_layers[1])
        l.bn[0], l.bn[1] = self.bn(mod.bn_layers[0]), self.bn(mod.bn_layers[1])
        l.out = self.affine(out_layer)
        return l

    def fill(self, model):
        params = _lib.MuralSnvParams()
        if model.model_no != 1:
            params.local = self.local(model, model.output_layer if model.model_no == 0 else model.local_fc[0])
        if model.model_no != 0:
            params.mid, params.large = self.tower(model, ""), self.tower(model, "_2")
        return params


def fill_snv(model, ptr):
    return _HostParams(ptr).fill(model)


def fill_indel(model, ptr):
    """MuralIndelParams of a UNet_Small."""
    bn = lambda m: _lib.MuralBN(ptr(m.weight), ptr(m.bias), ptr(m.running_mean), ptr(m.running_var))      # noqa: E731
    aff = lambda m: _lib.MuralAffine(ptr(m.weight), ptr(m.bias))                                             # noqa: E731
    convbn = lambda conv, b: _lib.MuralConvBN(aff(conv), bn(b))                                              # noqa: E731
    block = lambda cb: _lib.MuralConvBlock(ptr(cb.conv[0].weight), bn(cb.conv[1]), ptr(cb.conv[3].weight), bn(cb.conv[4]))   # noqa: E731
    p = _lib.MuralIndelParams()
    if model.use_reverse:
        p.sym = convbn(model.conv[0], model.conv[1])
    for i in range(model.N_LEVELS):
        p.up_l[i] = convbn(model.uplblocks[i][0], model.uplblocks[i][1])
        p.up_b[i] = block(model.upblocks[i][0])
    for j in range(model.N_LEVELS - 1):
        p.down_l[j] = convbn(model.downlblocks[j][1], model.downlblocks[j][2])
        p.down_b[j] = block(model.downblocks[j][0])
    p.out1, p.out_bn, p.out2 = aff(model.out_conv[0]), bn(model.out_conv[1]), aff(model.out_conv[3])
    p.fc_bn, p.fc = bn(model.out_fc[0]), aff(model.out_fc[2])
    return p


# ---------------------------------------------------------------------------------------------------------------
# the flat-gradient layout
# ---------------------------------------------------------------------------------------------------------------
_LAYOUT_OF = {}      # id(first parameter) -> (weak reference to that parameter, weak reference to the layout): mural_amd.train.Adam finds it


def layout_of_params(params, device_state=False):
    """The REGISTERED layout whose parameter list is exactly `params` (any order; empty parameters have no slot and do not count),
    or None.  A layout registered for the device loop only (``register="device_state"``: UNet_Small) is returned to an optimiser that
    carries a device step state and to nobody else: an optimiser built without one keeps torch's own step on such a model."""
    if not params or not _LAYOUT_OF:
        return None
    params = [p for p in params if p.numel()]
    for p in params:
        hit = _LAYOUT_OF.get(id(p))
        if hit is not None and hit[0]() is p:
            lay = hit[1]()
            if (lay is not None and (lay.register is True or device_state) and len(lay.plist) == len(params)
                    and {id(q) for q in lay.plist} == {id(q) for q in params}):
                return lay
    return None


def _tensors_of(model):
    return list(model.parameters()) + list(model.buffers())


class FlatGradLayout:
    """Which tensor sits in which pointer slot of `struct_type` (a flat run of pointers), found by running `fill(model, ptr)` once
    with slot tokens, and the offset of each parameter's gradient in one flat float32 buffer.

    register: True -- mural_amd.train's optimisers find the layout (layout_of_params) and take their one-launch step;
    "device_state" -- only those built with a device step state do (the device loop), the others keep torch's step.
    check_identity: `cached` rebuilds the layout when a parameter / buffer object of the model was replaced.
    twice: a BatchNorm counter that one forward bumps a second time."""

    def __init__(self, model, struct_type, fill, *, register=False, check_identity=False, twice=None):
        tensors = []

        def tok(t):
            tensors.append(t)
            return C.c_void_p(len(tensors))               # token = 1-based index into `tensors`

        self.struct_type = struct_type
        self.slots = C.sizeof(struct_type) // 8
        raw = np.frombuffer(bytes(fill(model, tok)), dtype=np.int64)
        assert raw.shape[0] == self.slots
        self.slot_tensor = [tensors[v - 1] if v else None for v in raw.tolist()]
        self.params_all = list(model.parameters())     # cached: walking the module tree costs ~0.2 ms per step
        self.plist = [p for p in self.params_all if p.numel()]
        self.model_ref = weakref.ref(model)
        self.identity = _tensors_of(model) if check_identity else None
        self.register = register
        if register and self.plist:
            for k in [k for k, (r, _) in _LAYOUT_OF.items() if r() is None]:      # (entries of models that are gone)
                del _LAYOUT_OF[k]
            _LAYOUT_OF[id(self.plist[0])] = (weakref.ref(self.plist[0]), weakref.ref(self))
        self.last_flat = None                          # the flat buffer behind the gradients of the latest backward (clip_grad_norm_)
        self.own_flat = None                           # direct-gradient mode (train_step.py): the buffer and the views into it, created once
        self.own_views = None
        self.own_base = None                           # holder counts of own_flat / own_views when they were made
        # gradient slots: offset of each parameter in one flat float32 buffer (running statistics have none)
        index = {id(p): i for i, p in enumerate(self.plist)}
        offs, o = [], 0
        for p in self.plist:
            offs.append(o)
            o += (p.numel() + 63) // 64 * 64
        self.total, self.poffs = o, offs
        self.grad_off = np.full(self.slots, -1, np.int64)
        for s, t in enumerate(self.slot_tensor):
            if t is not None and id(t) in index:
                self.grad_off[s] = offs[index[id(t)]] * 4
        self.has_grad = self.grad_off >= 0
        # num_batches_tracked: +1 per BatchNorm application (modules() lists a module registered twice, as in ResBlock, once; a
        # BatchNorm over zero features -- first_bn_layer without continuous inputs -- never runs)
        self.counters = [m.num_batches_tracked for m in model.modules()
                         if isinstance(m, torch.nn.BatchNorm1d) and m.num_batches_tracked is not None and m.weight.numel()]
        self.twice = twice

    @classmethod
    def cached(cls, model, make):
        """``model._train_layout``, made by `make(model)` when missing or (check_identity) stale."""
        lay = getattr(model, "_train_layout", None)
        if lay is not None and lay.identity is not None:
            now = _tensors_of(model)
            if len(now) != len(lay.identity) or any(a is not b for a, b in zip(now, lay.identity)):
                lay = None
        if lay is None:
            lay = model._train_layout = make(model)
        return lay

    def _struct(self, raw):
        s = self.struct_type()
        C.memmove(C.byref(s), raw.ctypes.data, self.slots * 8)
        return s

    def params_struct(self):
        for t in self.slot_tensor:
            if t is not None and (t.dtype is not torch.float32 or not t.is_contiguous()):
                raise RuntimeError("the HIP training step needs contiguous float32 parameters and buffers")
        return self._struct(np.array([0 if t is None else t.data_ptr() for t in self.slot_tensor], dtype=np.int64))

    def grads_struct(self, base):
        return self._struct(np.where(self.has_grad, self.grad_off + base, 0))

    def zero_flat(self, device):
        """A fresh gradient buffer; the zero padding between the slots makes the norm of the buffer the norm of the gradients."""
        return torch.zeros(self.total, dtype=torch.float32, device=device)

    def grad_views(self, flat):
        """One view of `flat` per parameter of ``plist``, in its order."""
        return [flat[o:o + p.numel()].view(p.shape) for p, o in zip(self.plist, self.poffs)]

    def grads_for(self, params, flat):
        """The gradients an autograd node returns for `params`: views of `flat`, zeros for empty parameters."""
        views = {id(p): v for p, v in zip(self.plist, self.grad_views(flat))}
        return tuple(views[id(p)] if p.numel() else torch.zeros_like(p) for p in params)

    def bump_counters(self):
        if self.counters:
            torch._foreach_add_(self.counters, 1)
        if self.twice is not None:
            self.twice.add_(1)


# ---------------------------------------------------------------------------------------------------------------
# shared lines of the two ModelStep nodes
# ---------------------------------------------------------------------------------------------------------------
def step_buffers(alloc, need, B, n_class, device, invalid=None):
    """(workspace of `need` bytes, (B, n_class) output), both from ``alloc.empty``: `alloc` is the calling module's ``torch``, which
    the steps' validation tests swap for one that hands out poisoned memory.  need == 0 is the library's "this shape is invalid":
    raises ValueError with `invalid`, or with the library's own message."""
    if need == 0:
        if invalid is not None:
            raise ValueError(invalid)
        _lib.check(_lib.MURAL_E_INVALID)
    return (alloc.empty(need, dtype=torch.uint8, device=device),
            alloc.empty((B, n_class), dtype=torch.float32, device=device))


def saved_workspace(ctx, name):
    """The workspace the forward left for ONE backward."""
    if ctx.ws is None:
        raise RuntimeError(f"the {name} training step keeps its saved activations for ONE backward (retain_graph=True is not supported: "
                           "run the forward again)")
    return ctx.ws


def node_grads(n_inputs, grads):
    """The return tuple of a ModelStep backward: nothing for the `n_inputs` non-parameter inputs, then the parameters' gradients."""
    return (None,) * n_inputs + tuple(grads)


# ---------------------------------------------------------------------------------------------------------------
# direct-gradient mode of the two ModelStep nodes (model/train_step.py: module docstring)
# ---------------------------------------------------------------------------------------------------------------
def _holder_counts(lay):
    """(references to the storage of the gradient buffer, Python + C++ references of every view into it)."""
    storage = torch._C._storage_Use_Count(lay.own_flat.untyped_storage()._cdata)
    return storage, [(sys.getrefcount(v), v._use_count()) for v in lay.own_views]


def _views_are_ours(lay):
    """Nobody but the layout holds last step's gradient views or anything derived from them (counts as at their creation)."""
    return _holder_counts(lay) == lay.own_base


def _direct_is_safe(params):
    """Direct-gradient mode only where nothing but ``p.grad`` observes the gradients, and every parameter takes one."""
    if torch.distributed.is_available() and torch.distributed.is_initialized() and torch.distributed.get_world_size() > 1:
        return False
    for p in params:
        if not p.requires_grad or p._backward_hooks or getattr(p, "_post_accumulate_grad_hooks", None):
            return False
    return True


def want_direct(model, params):
    """The node sets every ``.grad`` itself (one parameter anchors it in the autograd graph) unless the caller asked for the autograd
    route (``model._autograd_params`` / MURAL_TRAIN_AUTOGRAD_PARAMS) or a direct gradient could go unseen."""
    return (not getattr(model, "_autograd_params", False) and not os.environ.get("MURAL_TRAIN_AUTOGRAD_PARAMS")
            and _direct_is_safe(params))


def backward_flat(lay, dev, ctx_direct):
    """(the flat buffer this backward writes, whether its slots ARE the gradients): in direct mode with no ``.grad`` present, the
    buffer that lives with the layout -- same addresses every step -- else a fresh one (an existing ``.grad`` is accumulated into)."""
    direct = ctx_direct and all(p.grad is None for p in lay.plist)
    if direct:
        # Last step's gradients that somebody still holds (kept across zero_grad(set_to_none=True)) are not rewritten in place.
        # Three holders are looked for, each against the count recorded when the views were made: Python references to a view
        # object, C++ references to its TensorImpl, and -- what a derived tensor (`g.view(-1)`, `g[0]`, `g.detach()`) or any
        # other holder of the memory adds -- references to the buffer's storage.
        if lay.own_views is not None and not _views_are_ours(lay):
            lay.own_flat = lay.own_views = None
        if lay.own_flat is None or lay.own_flat.device != dev:
            lay.own_flat = lay.zero_flat(dev)
            lay.own_views = lay.grad_views(lay.own_flat)
            lay.own_base = _holder_counts(lay)
        flat = lay.own_flat      # every slot is rewritten by the backward call; the padding between the slots stays zero
    else:
        flat = lay.zero_flat(dev)
    lay.last_flat = flat
    return flat, direct


def hand_out(lay, flat, ctx_direct, direct, n_inputs, params):
    """The return tuple of a ModelStep backward that wrote `flat`: in direct mode the node sets / accumulates ``p.grad`` itself and
    hands autograd nothing; else the gradients of `params` as views of `flat`."""
    if ctx_direct:
        if direct:
            for p, v in zip(lay.plist, lay.own_views):
                p.grad = v
        else:
            for p, g in zip(lay.plist, lay.grad_views(flat)):
                if p.grad is None:
                    p.grad = g
                else:
                    p.grad.add_(g)
        return node_grads(n_inputs, (None,) * len(params))
    return node_grads(n_inputs, lay.grads_for(params, flat))
