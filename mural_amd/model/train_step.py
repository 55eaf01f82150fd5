"""The SNV training step as ONE autograd node over two C calls (include/mural_hip.h: mural_snv_train_forward / _backward).

``loss.backward()`` of the reference (MuRaL/training.py:424-427) walks ~120 autograd nodes; here the whole model forward is one
``torch.autograd.Function`` whose forward and backward are one library call each -- the composition of the ~100 kernels per
direction lives in C++ (csrc/snv_train.hip), so the host costs two ctypes transitions per step instead of one per layer.
Serves Network0 and the shipped tower shape (32 channels, kernel 3); towers of any other shape train on the per-layer ops of
``indel_train.py`` (``snv_tower_forward_train``) with the local branch and the head from ``train_ops.py``.

Gradients: the C backward writes every parameter gradient into ONE flat buffer.  By default the node then sets ``p.grad`` itself
-- views of a buffer that lives with the model, created once -- and hands autograd nothing: routing ~150 tensors through the engine
(one AccumulateGrad node and two view constructions per parameter) cost 1.0 ms of host time per step, as much as the whole device
backward at batch 4096.  ``p.grad`` after ``loss.backward()`` is what the reference loop (training.py:424-436: zero_grad, backward,
clip_grad_norm_, step) reads; an existing ``p.grad`` is accumulated into, like autograd does.  What this skips is autograd's own
bookkeeping per parameter: tensor hooks on parameters, ``torch.autograd.grad(loss, params)`` and DistributedDataParallel's reducer
do not see these gradients -- ``MURAL_TRAIN_AUTOGRAD_PARAMS=1`` (or ``model._autograd_params = True``) routes them through the
engine again.  The step falls back to that route BY ITSELF when a direct gradient could go unseen: a parameter carries a tensor hook
or a post-accumulate-grad hook, or a process group of more than one rank is initialised (DistributedDataParallel's reducer hangs off
the AccumulateGrad nodes this mode skips; ``north_star`` keeps training single-GPU, so nothing is lost).  ``torch.autograd.grad``
on parameters other than the anchor fails with autograd's own "not used in the graph" error.  The ``.grad`` views of one backward
are handed out again by the next one only while nobody else still holds them (reference count of the views): a caller who keeps
last step's gradients for accumulation or logging gets a fresh buffer instead of having them rewritten in place.
"""
import ctypes as C

import numpy as np
import torch

from .. import _lib
from . import step_layout
from .step_layout import layout_of_params      # noqa: F401  (mural_amd.train imports it from here)

MOMENTUM = 0.1


def _layout(model):
    # no identity check of the cached layout: walking the module tree costs ~0.2 ms of a 1.6 ms step.  _apply / load_state_dict of the
    # model clear _train_layout (model_snv._HipSnvBase)
    return step_layout.FlatGradLayout.cached(
        model, lambda m: step_layout.FlatGradLayout(m, _lib.MuralSnvParams, step_layout.fill_snv, register=True))


def supported(model):
    return model.model_no == 0 or (model.out_channels == 32 and model.kernel_size == 3)


def _make_shape(model):
    sh = getattr(model, "_train_shape", None)
    if sh is None:
        local = model.model_no != 1
        towers = model.model_no != 0
        sh = model._train_shape = _lib.MuralSnvShape(
            model.model_no, model.n_class, model.no_of_cat if local else 0, model.emb_layer.num_embeddings if local else 0,
            model.lin_layers[0].out_features if local else 0, model.lin_layers[1].out_features if local else 0,
            model.out_channels if towers else 32, model.kernel_size if towers else 3, model.seq_len if towers else 0, 1e-5)
    return sh


class ModelStep(torch.autograd.Function):
    """out = model(cat_x, distal_x) in training mode; backward returns the gradient of every parameter."""

    @staticmethod
    def forward(ctx, model, shape, cat_x, symbols, drops, seeds, seed_dev, direct, *params):
        lay = _layout(model)
        dev = params[0].device
        ctx.direct = direct
        B = (cat_x if cat_x is not None else symbols).shape[0]
        lib = _lib.lib()
        need = int(lib.mural_snv_train_workspace_bytes(C.byref(shape), B))
        ws, out = step_layout.step_buffers(torch, need, B, model.n_class, dev)
        ps = lay.params_struct()
        stream = _lib.current_stream_ptr(dev)
        _lib.check(lib.mural_snv_train_forward(C.byref(shape), C.byref(ps), None if cat_x is None else cat_x.data_ptr(), None,
                                               None if symbols is None else symbols.data_ptr(), B, drops.ctypes.data, seeds.ctypes.data,
                                               None if seed_dev is None else seed_dev.data_ptr(), MOMENTUM, out.data_ptr(), ws.data_ptr(),
                                               need, None, stream))
        lay.bump_counters()
        ctx.model, ctx.shape, ctx.ws, ctx.args, ctx.params = model, shape, ws, (cat_x, drops, seeds, seed_dev, B), params
        return out

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, dout):
        model, shape, ws = ctx.model, ctx.shape, step_layout.saved_workspace(ctx, "SNV")
        cat_x, drops, seeds, seed_dev, B = ctx.args
        lay = _layout(model)
        dev = ws.device
        flat, direct = step_layout.backward_flat(lay, dev, ctx.direct)
        ps, gs = lay.params_struct(), lay.grads_struct(flat.data_ptr())
        dout = dout.contiguous()
        _lib.check(_lib.lib().mural_snv_train_backward(C.byref(shape), C.byref(ps), C.byref(gs), None if cat_x is None else cat_x.data_ptr(),
                                                       dout.data_ptr(), B, drops.ctypes.data, seeds.ctypes.data,
                                                       None if seed_dev is None else seed_dev.data_ptr(), ws.data_ptr(), ws.numel(),
                                                       _lib.current_stream_ptr(dev)))
        ctx.ws = None
        return step_layout.hand_out(lay, flat, ctx.direct, direct, 8, ctx.params)


def run(model, cat_x, distal_x):
    """Training-mode forward of `model` on (cat_x int64 (B, cols) | None, distal_x float (B, 4, L) | uint8 (B, L) symbols | None)."""
    from . import train_ops as T
    shape = _make_shape(model)
    symbols = None
    if distal_x is not None and distal_x.dtype == torch.uint8 and distal_x.dim() == 2:
        symbols = distal_x                              # the encoder's symbols (model_snv._symbol_windows): nothing to convert or check
    elif distal_x is not None:
        symbols = T.dense_to_symbols(distal_x)          # flags non-encodings; checked behind the launches (flush_input_checks)
    ps = [model.emb_dropout_layer.p, model.droput_layers[0].p, model.droput_layers[1].p] if model.model_no != 1 else [0.0, 0.0, 0.0]
    ps += [model.distal_fc1[1].p, model.distal_fc2[1].p] if model.model_no != 0 else [0.0, 0.0]
    drops = np.asarray(ps, dtype=np.float32)
    seeds = np.zeros(5, dtype=np.uint64)
    for i, p in enumerate(ps):                          # one draw per active dropout, in the order of the reference's forward
        if p > 0.0:
            seeds[i] = int(torch.randint(0, 2 ** 62, (1,)).item())
    params = _layout(model).params_all
    # direct-gradient mode (module docstring): one parameter anchors the node in the autograd graph, the node sets every .grad itself
    direct = step_layout.want_direct(model, params)
    try:
        if direct:
            anchor = next(p for p in params if p.numel())
            out = ModelStep.apply(model, shape, cat_x, symbols, drops, seeds, T._device_seed, True, anchor)
        else:
            out = ModelStep.apply(model, shape, cat_x, symbols, drops, seeds, T._device_seed, False, *params)
        T.flush_input_checks()
    except BaseException:
        T._pending_checks.clear()                       # a failed forward must not leave its input check to the next one
        raise
    return out
