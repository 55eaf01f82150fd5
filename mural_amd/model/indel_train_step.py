"""The INDEL training step as ONE autograd node over two C calls (include/mural_hip.h: mural_indel_train_forward / _backward, or
their ``_symbols`` twins when the window comes as one symbol byte per column).

``UNet_Small.forward`` under ``model.train()`` (MuRaL/model/model_indel.py:151-176) inside the step of MuRaL/training.py:424-436: the
per-unit composition of ``indel_train.py`` walks ~40 autograd nodes and issues ~340 launches from Python; here the composition lives
in C++ (csrc/indel_train_step.hip) and the host pays two ctypes transitions per step.  ``loss.backward()``, ``clip_grad_norm_`` and
``torch.optim`` work unchanged: every gradient is a view of one flat buffer, set as ``p.grad`` by the node itself (the direct-gradient
mode of train_step.py, one copy of its rules in step_layout.py) or, where that could go unseen -- a frozen parameter, a tensor hook, a
process group of more than one rank, ``model._autograd_params`` / MURAL_TRAIN_AUTOGRAD_PARAMS -- returned to autograd one per parameter.
``clip_grad_norm_`` then takes its two launches.  The layout is registered for the device loop: ``mural_amd.train``'s optimisers take
their one-launch step on a UNet_Small when they were built with a ``device_state`` (which moves ``p.data`` into a flat buffer); built
without one they step through torch as before.
"""
import ctypes as C

import torch

from .. import _lib
from . import step_layout

MOMENTUM = 0.1


def _make_layout(model):
    # registered for optimisers on a device step state only (step_layout.layout_of_params)
    # num_batches_tracked: the strand-symmetrising layer's BatchNorm is applied twice per forward
    return step_layout.FlatGradLayout(model, _lib.MuralIndelParams, step_layout.fill_indel, register="device_state", check_identity=True,
                                      twice=model.conv[1].num_batches_tracked if model.use_reverse else None)


def _layout(model):
    # the cached layout holds the parameter / buffer OBJECTS: replacing one of them (model.conv.weight = nn.Parameter(...)) must
    # rebuild it -- compared by identity, a few dozen `is` tests per call (the step is device-bound: check_identity stays on)
    return step_layout.FlatGradLayout.cached(model, _make_layout)


def _shape(model, length):
    return _lib.MuralIndelShape(model.n_class, model.out_channels, model.kernel_size, (C.c_int32 * 6)(*model.downsize),
                                int(bool(model.use_reverse)), int(length), 1e-5)


class ModelStep(torch.autograd.Function):
    """out = model(x) in training mode; backward returns the gradient of every parameter."""

    @staticmethod
    def forward(ctx, model, x, drop_p, seed, seed_dev, direct, *params):
        lay = _layout(model)
        dev = x.device
        ctx.direct = direct
        symbols = x.dtype is torch.uint8          # (B, L) symbol bytes: the input form decides the entry, nothing else differs
        B, length = x.shape[0], x.shape[-1]
        shape = _shape(model, length)
        lib = _lib.lib()
        need = int((lib.mural_indel_train_symbols_workspace_bytes if symbols else lib.mural_indel_train_workspace_bytes)(C.byref(shape), B))
        ws, out = step_layout.step_buffers(torch, need, B, model.n_class, dev,
                                           invalid=f"input length {length} is not compatible with down_list {list(model.downsize)}")
        ps = lay.params_struct()
        fwd = lib.mural_indel_train_forward_symbols if symbols else lib.mural_indel_train_forward
        _lib.check(fwd(C.byref(shape), C.byref(ps), x.data_ptr(), B, float(drop_p), int(seed),
                       None if seed_dev is None else seed_dev.data_ptr(), MOMENTUM, out.data_ptr(), ws.data_ptr(), need,
                       _lib.current_stream_ptr(dev)))
        lay.bump_counters()
        ctx.model, ctx.shape, ctx.ws, ctx.args, ctx.params = model, shape, ws, (x, drop_p, seed, seed_dev, B, symbols), params
        return out

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, dout):
        model, shape, ws = ctx.model, ctx.shape, step_layout.saved_workspace(ctx, "INDEL")
        x, drop_p, seed, seed_dev, B, symbols = ctx.args
        lay = _layout(model)
        dev = ws.device
        flat, direct = step_layout.backward_flat(lay, dev, ctx.direct)
        ps, gs = lay.params_struct(), lay.grads_struct(flat.data_ptr())
        dout = dout.contiguous()
        bwd = _lib.lib().mural_indel_train_backward_symbols if symbols else _lib.lib().mural_indel_train_backward
        _lib.check(bwd(C.byref(shape), C.byref(ps), C.byref(gs), x.data_ptr(), dout.data_ptr(), B, float(drop_p), int(seed),
                       None if seed_dev is None else seed_dev.data_ptr(), ws.data_ptr(), ws.numel(), _lib.current_stream_ptr(dev)))
        ctx.ws = None
        return step_layout.hand_out(lay, flat, ctx.direct, direct, 6, ctx.params)


def run(model, x):
    """Training-mode forward of `model` (UNet_Small) on x float32 (B, 4, L), or on x uint8 (B, L): one MURAL_SYM_* symbol per window
    column (``SymbolWindows.sym``), which takes the symbol entries -- the dense window is never built."""
    if x.dtype is torch.uint8:
        if x.dim() != 2:
            raise ValueError(f"symbol windows must be uint8 (B, L), got {tuple(x.shape)}")
    elif x.dtype is not torch.float32 or x.dim() != 3 or x.shape[1] != 4:
        raise ValueError(f"the INDEL training step takes float32 (B, 4, L) or uint8 (B, L) symbols, got {x.dtype} {tuple(x.shape)}")
    x = x.contiguous()
    from . import train_ops as T
    p = float(model.out_fc[1].p)
    seed = int(torch.randint(0, 2 ** 62, (1,)).item()) if p > 0.0 else 0     # torch's CPU generator: torch.manual_seed applies
    params = _layout(model).params_all
    if step_layout.want_direct(model, params):      # one parameter anchors the node; it sets every .grad itself
        return ModelStep.apply(model, x, p, seed, T._device_seed, True, next(q for q in params if q.numel()))
    return ModelStep.apply(model, x, p, seed, T._device_seed, False, *params)
