"""Autograd glue for the training-mode HIP building blocks (include/mural_hip.h, ``mural_op_*``).

Each ``torch.autograd.Function`` below launches hand-written HIP kernels for its forward and backward; torch only
provides the tensors, the stream and the autograd graph (the reference relies on stock autograd over ``torch.nn`` ops,
MuRaL/training.py:424-427).  BatchNorm running statistics are updated in place by the forward kernels exactly like
``nn.BatchNorm1d`` in training mode (momentum 0.1, unbiased running variance).
"""
import ctypes as C
import os

import torch

from .. import _lib

EPS, MOMENTUM = 1e-5, 0.1
BN_SLOTS = 32          # include/mural_hip.h MURAL_BN_SLOTS


class _ZeroArena:
    """Zero-initialised float64 scratch handed out in slices: one fill kernel per chunk instead of one per accumulator.
    Slices are never reused (a fresh chunk replaces an exhausted one; views keep old chunks alive as long as needed)."""

    CHUNK = 1 << 17     # doubles (1 MiB)

    def __init__(self):
        self.buf, self.off = None, 0

    def take(self, n, device):
        if self.buf is None or self.buf.device != device or self.off + n > self.buf.numel():
            self.buf, self.off = torch.zeros(max(self.CHUNK, n), dtype=torch.float64, device=device), 0
        out = self.buf[self.off:self.off + n]
        self.off += n
        return out


_arena = _ZeroArena()


def reset_zero_arena():
    """Drop the current chunk (graph capture: the fill of the chunks used inside the graph must be part of the graph)."""
    _arena.buf, _arena.off = None, 0


def _bn_acc(Cn, device):
    """Zeroed accumulator block (BN_SLOTS, 2, C) for batch sums (see mural_op_bn_stats)."""
    return _arena.take(BN_SLOTS * 2 * Cn, device).view(BN_SLOTS, 2, Cn)


_fn_cache = {}
_Tensor = torch.Tensor


def _call(name, *args):
    fn = _fn_cache.get(name)
    if fn is None:
        fn = _fn_cache[name] = getattr(_lib.lib(), name)
    rc = fn(*[a.data_ptr() if isinstance(a, _Tensor) else a for a in args])
    if rc:
        _lib.check(rc)


def _stream(t):
    return _lib.current_stream_ptr(t.device)


def _f32(t):
    if t.dtype is torch.float32 and t.is_contiguous():
        return t                      # only its data pointer is used
    return t.detach().to(torch.float32).contiguous()


_bn_touched = []


def _bn_tick(bn):
    """nn.BatchNorm1d increments num_batches_tracked per training forward; the increments of one model forward are applied
    together (flush_bn_ticks) instead of one tiny kernel per layer."""
    _bn_touched.append(bn.num_batches_tracked)


def flush_bn_ticks():
    flush_input_checks()
    if _bn_touched:
        with torch.no_grad():
            count, first = {}, {}
            for t in _bn_touched:
                count[id(t)] = count.get(id(t), 0) + 1
                first.setdefault(id(t), t)
            once = [first[k] for k, c in count.items() if c == 1]
            if once:
                torch._foreach_add_(once, 1)
            for k, c in count.items():    # a BatchNorm applied more than once per forward (UNet_Small's strand-symmetry conv)
                if c > 1:
                    first[k].add_(c)
        _bn_touched.clear()


class _BnState:
    """Per-call batch statistics of one BatchNorm (scale/shift for the forward pre-op, mean/invstd for the backward).
    ``acc`` = accumulator block with the sums of act(x) / act(x)^2 when the producer of x already took them in its epilogue."""

    def __init__(self, x, relu, bn, L, acc=None):
        B, Cn = x.shape[0], x.shape[1]
        dev = x.device
        st = _stream(x)
        if acc is None:
            acc = _bn_acc(Cn, dev)
            _call("mural_op_bn_stats", x, B, Cn, L, int(relu), acc, st)
        self.scale, self.shift, self.mean, self.invstd = torch.empty((4, Cn), dtype=torch.float32, device=dev).unbind(0)
        _call("mural_op_bn_finalize", acc, float(B * L), Cn, _f32(bn.weight), _f32(bn.bias), EPS, MOMENTUM,
              bn.running_mean, bn.running_var, self.scale, self.shift, self.mean, self.invstd, st)
        _bn_tick(bn)


class Bn2d(torch.autograd.Function):
    """y = BN(act(x)) on (B, C) features (batch statistics over B)."""

    @staticmethod
    def forward(ctx, x, gamma, beta, bn, pre_relu):
        x = x.contiguous()
        B, Cn = x.shape
        state = _BnState(x, pre_relu, bn, 1)
        y = torch.empty_like(x)
        _call("mural_op_bn_apply", x, B, Cn, 1, int(pre_relu), state.scale, state.shift, y, _stream(x))
        ctx.save_for_backward(x, gamma, state.mean, state.invstd)
        ctx.pre_relu = pre_relu
        return y

    @staticmethod
    def backward(ctx, dy):
        x, gamma, mean, invstd = ctx.saved_tensors
        B, Cn = x.shape
        acc = _bn_acc(Cn, x.device)
        dx = torch.empty_like(x)
        dgamma = torch.empty(Cn, dtype=torch.float32, device=x.device)
        dbeta = torch.empty(Cn, dtype=torch.float32, device=x.device)
        _call("mural_op_bn_backward", dy.contiguous(), x, B, Cn, 1, int(ctx.pre_relu), mean, invstd, _f32(gamma), acc, 0, None,
              None, dx, dgamma, dbeta, _stream(x))
        return dx, dgamma, dbeta, None, None


class MaxPool(torch.autograd.Function):
    """MaxPool1d(k, s, p) (floor mode, -inf padding); k = None -> global max over L (returns (B, C))."""

    @staticmethod
    def forward(ctx, x, k, s, p):
        x = x.contiguous()
        B, Cn, L = x.shape
        glob = k is None
        if glob:
            k, s, p = L, L, 0          # one window per row: the backward is a gather (no zero fill, no atomics)
        Lout = (L + 2 * p - k) // s + 1
        y = torch.empty((B, Cn, Lout), dtype=torch.float32, device=x.device)
        arg = torch.empty((B, Cn, Lout), dtype=torch.int32, device=x.device)
        _call("mural_op_maxpool_fwd", x, B * Cn, L, k, s, p, y, arg, _stream(x))
        ctx.save_for_backward(arg)
        ctx.dims = (B, Cn, L, Lout, glob, k, s, p)
        return y.reshape(B, Cn) if glob else y

    @staticmethod
    def backward(ctx, dy):
        (arg,) = ctx.saved_tensors
        B, Cn, L, Lout, glob, k, s, p = ctx.dims
        # disjoint windows (stride >= kernel, every pool of the model): a gather writes all of dx, no zero fill / atomics
        dx = (torch.zeros if s < k else torch.empty)((B, Cn, L), device=dy.device)
        _call("mural_op_maxpool_bwd", dy.contiguous(), arg, B * Cn, L, Lout, k, s, p, dx, _stream(dy))
        return dx, None, None, None


def _first_plan(Cn, pk):
    """(tab floats, arg bytes per pooled output, backward scratch floats) of the first-layer kernels for this shape."""
    import ctypes as C
    t, a, s = C.c_int64(0), C.c_int64(0), C.c_int64(0)
    _lib.check(_lib.lib().mural_op_first_plan(Cn, pk, C.byref(t), C.byref(a), C.byref(s)))
    return t.value, a.value, s.value


class Linear(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, weight, bias):
        x = x.contiguous()
        B, I = x.shape
        O = weight.shape[0]
        y = torch.empty((B, O), dtype=torch.float32, device=x.device)
        _call("mural_op_linear_fwd", x, _f32(weight), _f32(bias), B, I, O, y, _stream(x))
        ctx.save_for_backward(x, weight)
        return y

    @staticmethod
    def backward(ctx, dy):
        x, weight = ctx.saved_tensors
        B, I = x.shape
        O = weight.shape[0]
        dx = torch.empty_like(x)
        dW = torch.empty_like(weight)
        db = torch.empty(O, dtype=torch.float32, device=x.device)
        _call("mural_op_linear_bwd", dy.contiguous(), x, _f32(weight), B, I, O, dx, dW, db, _stream(x))
        return dx, dW, db


class Embedding(torch.autograd.Function):
    """concat_i emb[cat[:, i]] with ONE shared (rows, 5) table (model_snv.py:322, :452-454)."""

    @staticmethod
    def forward(ctx, cat, table):
        cat = cat.contiguous()
        B, cols = cat.shape
        y = torch.empty((B, cols * 5), dtype=torch.float32, device=table.device)
        _call("mural_op_embedding_fwd", cat, _f32(table), B, cols, table.shape[0], y, _stream(table))
        ctx.save_for_backward(cat)
        ctx.rows = table.shape[0]
        return y

    @staticmethod
    def backward(ctx, dy):
        (cat,) = ctx.saved_tensors
        B, cols = cat.shape
        dE = torch.zeros((ctx.rows, 5), dtype=torch.float32, device=dy.device)
        _call("mural_op_embedding_bwd", cat, dy.contiguous(), B, cols, ctx.rows, dE, _stream(dy))
        return None, dE


class Dropout(torch.autograd.Function):
    """Inverted dropout with a counter-based generator; the mask is regenerated from the seed in the backward."""

    @staticmethod
    def forward(ctx, x, p, seed, seed_dev=None):
        x = x.contiguous()
        y = torch.empty_like(x)
        _call("mural_op_dropout", x, x.numel(), float(p), C.c_uint64(seed), seed_dev, y, _stream(x))
        ctx.p, ctx.seed, ctx.seed_dev = float(p), seed, seed_dev
        return y

    @staticmethod
    def backward(ctx, dy):
        dy = dy.contiguous()
        dx = torch.empty_like(dy)
        _call("mural_op_dropout", dy, dy.numel(), ctx.p, C.c_uint64(ctx.seed), ctx.seed_dev, dx, _stream(dy))
        return dx, None, None, None


_device_seed = None


def set_device_seed(t):
    """A device-resident uint64 step counter (int64 tensor of one element) added to every dropout seed, or None.  A captured
    training step (mural_amd.train.GraphedTrainStep) bakes the host-drawn seeds into the graph and advances this counter
    inside it, so every replay draws fresh masks."""
    global _device_seed
    _device_seed = t


def dropout(x, p, training=True):
    if not training or p <= 0.0:
        return x
    seed = int(torch.randint(0, 2 ** 62, (1,)).item())     # drawn from torch's CPU generator: torch.manual_seed applies
    return Dropout.apply(x, p, seed, _device_seed)


class Head(torch.autograd.Function):
    """log(clamp((softmax(local) + (softmax(mid) + softmax(large)) / 2) / 2, 1e-9)); local=None for Network1."""

    @staticmethod
    def forward(ctx, loc, mid, lar):
        B, nc = mid.shape
        out = torch.empty((B, nc), dtype=torch.float32, device=mid.device)
        loc_c = None if loc is None else loc.contiguous()
        mid, lar = mid.contiguous(), lar.contiguous()
        _call("mural_op_head_fwd", loc_c, mid, lar, B, nc, out, _stream(mid))
        ctx.save_for_backward(mid, lar, *([] if loc_c is None else [loc_c]))
        return out

    @staticmethod
    def backward(ctx, dout):
        saved = ctx.saved_tensors
        mid, lar = saved[0], saved[1]
        loc = saved[2] if len(saved) > 2 else None
        B, nc = mid.shape
        dmid, dlar = torch.empty_like(mid), torch.empty_like(lar)
        dloc = None if loc is None else torch.empty_like(loc)
        _call("mural_op_head_bwd", loc, mid, lar, dout.contiguous(), B, nc, dloc, dmid, dlar, _stream(mid))
        return dloc, dmid, dlar


_pending_checks = []
_status_host = {}
captured_status = []


def dense_to_symbols(distal_x):
    """(B, 4, L) MuRaL one-hot / IUPAC-fraction tensor -> (B, L) uint8 symbols.  Anything else raises ValueError from
    ``flush_input_checks`` (called by the model forward after its launches are enqueued: the host then waits for this early
    kernel only instead of draining the device before the forward starts)."""
    x = distal_x.to(torch.float32).contiguous()
    B, _, L = x.shape
    dev = x.device
    sym = torch.empty((B, L), dtype=torch.uint8, device=dev)
    status = torch.zeros(1, dtype=torch.int32, device=dev)
    _call("mural_op_dense_to_symbols", x, B, L, sym, status, _stream(x))
    if torch.cuda.is_current_stream_capturing():
        captured_status.append(status)          # read by the owner of the graph after a replay (GraphedTrainStep)
        return sym
    host = _status_host.get(dev)
    if host is None:
        host = _status_host[dev] = torch.zeros(1, dtype=torch.int32).pin_memory()
    host.copy_(status, non_blocking=True)
    ev = torch.cuda.Event()
    ev.record(torch.cuda.current_stream(dev))
    _pending_checks.append((ev, host))
    return sym


def flush_input_checks():
    if os.environ.get("MURAL_DEBUG_NO_INPUT_CHECK"):      # diagnostic (tools/host_vs_gpu_train.py): never wait for the device
        _pending_checks.clear()
    if _pending_checks and torch.cuda.is_current_stream_capturing():
        return                                            # a captured step: the owner of the graph checks after the replay
    while _pending_checks:
        ev, host = _pending_checks.pop()
        ev.synchronize()
        if int(host[0]) != 0:
            raise ValueError("distal_input holds a column that is not a MuRaL one-hot / IUPAC-fraction encoding")


# ---------------------------------------------------------------------------------------------------------------
# model composition (training mode)
# ---------------------------------------------------------------------------------------------------------------
def local_forward(mod, cat, out_layer, emb_p, lin_ps, training=True):
    h = Embedding.apply(cat, mod.emb_layer.weight)
    h = dropout(h, emb_p, training)
    for lin, bn, p in zip(mod.lin_layers, mod.bn_layers, lin_ps):
        h = Linear.apply(h, lin.weight, lin.bias)
        h = Bn2d.apply(h, bn.weight, bn.bias, bn, True)          # order Linear -> ReLU -> BN (model_snv.py:466-467)
        h = dropout(h, p, training)
    return Linear.apply(h, out_layer.weight, out_layer.bias)
