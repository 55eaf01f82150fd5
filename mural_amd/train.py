"""Whole-step hipGraph replay of the training step (``GraphedTrainStep``: SNV models, ``GraphedIndelTrainStep``: UNet_Small).

The eager step (MuRaL/training.py:424-436: forward, CE-sum loss, zero_grad, backward, clip_grad_norm_, optimizer.step) is
about 300 kernel launches behind ~4 ms of Python; once the kernels are fast the host is the bottleneck.  ``GraphedTrainStep``
captures one step into a HIP graph (``torch.cuda.CUDAGraph``) and replays it: the host then costs one launch per step.

Differences from a plain loop, all of them the usual graph-capture contract:
  * batch shapes are fixed at capture; inputs are copied into static tensors before every replay;
  * the optimizer must be capturable and is stepped inside the graph: ``torch.optim.Adam(..., capturable=True)`` (torch's multi-tensor
    sequence), or ``mural_amd.train.Adam`` / ``AdamW`` / ``SGD(..., device_state=DeviceStepState(...))`` -- the one-launch step with its step count, bias
    corrections and scheduled learning rate in a device block that a tick kernel advances inside the graph (csrc/train_state.hip);
  * dropout masks: the host-drawn seeds are baked into the graph, a device-resident counter advanced inside the graph is
    added to them, so every replay draws new masks (``train_ops.set_device_seed``);
  * the encoding check of ``distal_x`` (ValueError on a non-MuRaL column) is read back after the replay, one step late.

The INDEL step (MuRaL/training.py:404-450 over model_indel.py:151-176) is ~500 small launches behind 7-11 ms of Python autograd
glue, depending on the host; its replay is bound by the device alone.
"""
import torch

from .model import train_ops as T

from ._host import freeze_host_heap  # noqa: E402,F401  (re-exported: train_epoch's loop and the benches call it)


class GraphedTrainStep:
    def __init__(self, model, optimizer, criterion, cont_x, cat_x, distal_x, y, max_norm=10.0, warmup=3):
        self.cont, self.cat = (None if t is None else t.clone() for t in (cont_x, cat_x))
        self._capture(model, optimizer, criterion, self._tensor(distal_x), y, max_norm, warmup)

    @staticmethod
    def _tensor(x):
        """The static input is a tensor: the dense float (B, 4, L) windows, or the uint8 (B, L) symbols (given as such or as
        ``SymbolWindows``, the form ``EpochLoader`` yields)."""
        return getattr(x, "sym", x)

    def _capture(self, model, optimizer, criterion, distal_x, y, max_norm, warmup):
        dev = distal_x.device
        self.model, self.opt, self.crit, self.max_norm = model, optimizer, criterion, max_norm
        self.x, self.y = distal_x.clone(), y.clone()
        self.seed = torch.zeros(1, dtype=torch.int64, device=dev)
        self.loss = None
        self._status = []
        self._pending = None
        T.set_device_seed(self.seed)
        try:
            side = torch.cuda.Stream(device=dev)
            side.wait_stream(torch.cuda.current_stream(dev))
            with torch.cuda.stream(side):
                for _ in range(warmup):        # allocator warm-up, lazy kernel attributes, optimizer state
                    self._eager_step()
            torch.cuda.current_stream(dev).wait_stream(side)
            torch.cuda.synchronize(dev)
            T.reset_zero_arena()
            T.captured_status.clear()
            self.graph = torch.cuda.CUDAGraph()
            with torch.cuda.graph(self.graph):
                self._eager_step()
            self._status = list(T.captured_status)
            T.captured_status.clear()
            T.reset_zero_arena()
        finally:
            T.set_device_seed(None)

    def _eager_step(self):
        self.seed += 0x9E3779B97F4A7C15 & 0x7FFFFFFFFFFFFFFF       # new dropout masks every step (odd 63-bit increment)
        out = self._forward()
        self.loss = self.crit(out, self.y)
        # gradients of the one-call HIP step are views of a buffer that lives with the model (model/train_step.py: direct-gradient
        # mode): dropped here, set again by the backward -- same addresses every step, nothing to zero or to accumulate into
        self.opt.zero_grad(set_to_none=True)
        self.loss.backward()
        clip_grad_norm_(self.model, self.max_norm)
        state = getattr(self.opt, "device_state", None)
        if state is not None:                  # the step's tick adds this loss to the block's sum (no launch of its own)
            state.observe(self.loss, self.y.shape[0])
        self.opt.step()

    def _forward(self):
        if self.x.dtype is torch.uint8:
            from .data.genome import SymbolWindows
            return self.model((self.cont, self.cat), SymbolWindows(self.x))
        return self.model((self.cont, self.cat), self.x)

    def __call__(self, cont_x, cat_x, distal_x, y):
        """Run one training step on this batch; returns the (device) loss tensor of the step."""
        self.cont.copy_(cont_x, non_blocking=True)
        self.cat.copy_(cat_x, non_blocking=True)
        return self._replay(self._tensor(distal_x), y)

    def _replay(self, distal_x, y):
        self._check()
        self.x.copy_(distal_x, non_blocking=True)
        self.y.copy_(y, non_blocking=True)
        self.graph.replay()
        if self._status:
            host = torch.empty(len(self._status), dtype=torch.int32, pin_memory=True)
            for i, s in enumerate(self._status):
                host[i:i + 1].copy_(s, non_blocking=True)
            ev = torch.cuda.Event()
            ev.record()
            self._pending = (ev, host)
        return self.loss

    def _check(self):
        if self._pending is not None:
            ev, host = self._pending
            ev.synchronize()
            self._pending = None
            if int(host.max()) != 0:
                raise ValueError("distal_input of the previous step held a column that is not a MuRaL one-hot / IUPAC-fraction "
                                 "encoding")

    def finish(self):
        """Wait for the last replay and raise its deferred input check, if any."""
        torch.cuda.synchronize()
        self._check()


class GraphedIndelTrainStep(GraphedTrainStep):
    """The same for ``UNet_Small`` (one input tensor): ``step = GraphedIndelTrainStep(model, opt, crit, x, y); loss = step(x, y)``."""

    def __init__(self, model, optimizer, criterion, x, y, max_norm=10.0, warmup=3):
        self._capture(model, optimizer, criterion, self._tensor(x), y, max_norm, warmup)

    def _forward(self):
        if self.x.dtype is torch.uint8:
            from .data.genome import SymbolWindows
            return self.model(SymbolWindows(self.x))
        return self.model(self.x)

    def __call__(self, x, y):
        return self._replay(self._tensor(x), y)


class _CESum(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, y):
        from . import _lib
        B, nc = x.shape
        prob = torch.empty_like(x)
        loss = torch.empty((), dtype=torch.float32, device=x.device)
        with torch.cuda.device(x.device):
            _lib.check(_lib.lib().mural_op_ce_sum_fwd(x.data_ptr(), y.data_ptr(), B, nc, prob.data_ptr(), loss.data_ptr(),
                                                     _lib.current_stream_ptr(x.device)))
        ctx.save_for_backward(prob, y)
        return loss

    @staticmethod
    def backward(ctx, g):
        from . import _lib
        prob, y = ctx.saved_tensors
        B, nc = prob.shape
        g = g.to(torch.float32).contiguous()
        dx = torch.empty_like(prob)
        with torch.cuda.device(prob.device):
            _lib.check(_lib.lib().mural_op_ce_sum_bwd(prob.data_ptr(), y.data_ptr(), g.data_ptr(), B, nc, dx.data_ptr(),
                                                     _lib.current_stream_ptr(prob.device)))
        return dx, None


class CrossEntropySum(torch.nn.Module):
    """``torch.nn.CrossEntropyLoss(reduction='sum')`` (training.py:327, the criterion of the reference's loops) as one launch per
    direction: between the model's forward and backward torch's version is a chain of four to six dependent little launches (log-softmax,
    gather / reduce, their backwards) with nothing else to run beside them.  Same value up to the order of the sum (fixed here: the loss
    is reproducible), same gradient; a label outside [0, n_class) gives NaN where torch raises a device assert.  Anything but a float32
    (B, n_class) device tensor with int64 labels of at most 65536 rows goes to torch's implementation."""

    def forward(self, x, y):
        if (x.is_cuda and x.dtype == torch.float32 and x.dim() == 2 and y.dim() == 1 and y.dtype == torch.int64 and y.is_cuda
                and x.shape[0] == y.shape[0] and 0 < x.shape[0] <= 65536):
            return _CESum.apply(x.contiguous(), y.contiguous())
        return torch.nn.functional.cross_entropy(x, y, reduction="sum")


def clip_grad_norm_(model, max_norm):
    """``torch.nn.utils.clip_grad_norm_(model.parameters(), max_norm)`` (training.py:430) for a model whose gradients came out of
    the one-call HIP backward: they are views of ONE flat buffer (zero between the slots), so the total 2-norm is one reduction
    over it and the scaling one multiply -- three launches instead of a 150-tensor foreach.  Any other state (a gradient that
    was replaced or accumulated elsewhere, a model without the flat buffer) falls through to torch's implementation."""
    lay = getattr(model, "_train_layout", None)
    flat = getattr(lay, "last_flat", None) if lay is not None else None
    if flat is not None:
        base = flat.data_ptr()
        for p, off in zip(lay.plist, lay.poffs):        # every gradient still sits in its slot of the latest backward's buffer
            g = p.grad
            if g is None or g.data_ptr() != base + 4 * off:
                break
        else:
            # two launches of the library (sums of squares per workgroup in double, then coefficient + scaling by every workgroup) instead of
            # torch's single-workgroup reduction and five scalar launches: 50 -> 12 us at the tail of every step
            from . import _lib
            scratch = getattr(lay, "clip_scratch", None)
            if scratch is None or scratch.device != flat.device:
                scratch = lay.clip_scratch = torch.empty(64, dtype=torch.float64, device=flat.device)
            total = torch.empty((), dtype=torch.float32, device=flat.device)      # (a fresh tensor per call: the caller may keep it)
            _lib.check(_lib.lib().mural_op_clip_grad_norm(flat.data_ptr(), flat.numel(), float(max_norm), scratch.data_ptr(),
                                                          total.data_ptr(), _lib.current_stream_ptr(flat.device)))
            return total
    # separate gradient tensors (UNet_Small, the per-layer SNV paths): torch's own sequence of launches -- per-tensor norms by one
    # foreach call, the norm of those, one foreach multiply -- without walking the module tree and regrouping ~150 tensors every
    # step (0.3 of the 0.8 ms that call costs on the host; the parameter list is cached on the model)
    plist = getattr(model, "_clip_plist", None)
    if plist is None:
        plist = model._clip_plist = [p for p in model.parameters()]
    grads = [p.grad for p in plist if p.grad is not None]
    if not grads:
        return torch.zeros((), device=plist[0].device if plist else "cpu")
    dev, dt = grads[0].device, grads[0].dtype
    if any(g.device != dev or g.dtype != dt for g in grads):
        return torch.nn.utils.clip_grad_norm_(plist, max_norm=max_norm, error_if_nonfinite=False)
    total = torch.linalg.vector_norm(torch.stack(torch._foreach_norm(grads, 2.0)), 2.0)
    torch._foreach_mul_(grads, torch.clamp(max_norm / (total + 1e-6), max=1.0))
    return total


def _schedule(config, train_size=None):
    kind = config["lr_scheduler"]
    if kind == "StepLR":
        return (5000 * 128) // config["batch_size"], float(config["LR_gamma"]), float(config["min_lr"]), float(config["restart_lr"])
    if kind == "StepLR2":
        gamma = (config["min_lr"] / config["restart_lr"]) ** (1 / (train_size // config["batch_size"]))
        return 1, float(gamma), float(config["min_lr"]), float(config["restart_lr"])
    if kind == "ROP":           # ReduceLROnPlateau: the host writes the rate between epochs (set_lr); train_epoch applies no restart rule
        return 0, 1.0, 0.0, 0.0
    raise ValueError(f"unknown lr_scheduler {kind}")


class DeviceStepState:
    """What the reference's loop keeps on the host between steps (training.py:432-450), as one ``MuralTrainState`` block in device memory
    (include/mural_hip.h): the learning rate, Adam's step count and the two bias-correction factors of the coming update, the per-batch
    scheduler's tick count, the epoch's loss sum / rows / steps.  ``mural_op_train_state_tick`` advances it once per step -- inside a
    captured graph too, which is what lets ``GraphedTrainStep`` replay ``Adam(..., device_state=...)`` with a moving step count and a
    scheduled rate -- and nothing is read back until somebody asks (``read``: one synchronising copy).

    The BLOCK holds the learning rate of an optimiser built on it, not ``param_groups`` (they are brought up to date whenever a step
    goes through torch, and by ``train_epoch_device`` at the end of an epoch); ``set_lr`` writes it."""

    NO_SCHEDULE = (0, 1.0, 0.0, 0.0)

    def __init__(self, device, lr, betas=(0.9, 0.999)):
        self.device = torch.device(device)
        if self.device.type != "cuda":
            raise RuntimeError(f"the step state lives on a HIP device (got {self.device}); mural_amd has no CPU path")
        self.betas = (float(betas[0]), float(betas[1]))
        self.sched = self.NO_SCHEDULE          # (sched_step_size, gamma, min_lr, restart_lr) of the ticks to come
        self.buf = torch.zeros(16, dtype=torch.int64, device=self.device)      # the 128 bytes; fields by word: mural_hip.h
        self._f64 = self.buf.view(torch.float64)
        self._loss, self._rows = None, 0
        self.set_lr(lr)

    # -- host writes (stream-ordered little fills; never inside a captured region) and the one read --------------------------------
    def set_lr(self, lr):
        self._f64[0:1].fill_(float(lr))

    def set_step(self, step):
        self.buf[1:2].fill_(int(step))

    def reset_epoch(self):
        """Zero loss_sum, rows and steps_done; step, ticks and lr stay."""
        self.buf[3:6].zero_()

    def read(self):
        """The fields as a dict (ONE synchronising copy of the block)."""
        w = self.buf.cpu().numpy()
        d, f = w.view("float64"), w.view("float32")
        return dict(lr=float(d[0]), step=int(w[1]), ticks=int(w[2]), loss_sum=float(d[3]), rows=int(w[4]), steps_done=int(w[5]),
                    step_size=float(f[12]), bc2_sqrt=float(f[13]))

    # -- the schedule ----------------------------------------------------------------------------------------------------------------
    @staticmethod
    def schedule(config, train_size=None):
        """The reference's ``config`` -> (sched_step_size, gamma, min_lr, restart_lr) of the tick: what ``make_scheduler`` builds and
        ``train_epoch`` applies per batch.  'ROP' has no per-batch part: (0, 1.0) and no restart rule."""
        return _schedule(config, train_size)

    def set_schedule(self, config, train_size=None):
        self.sched = self.schedule(config, train_size)
        return self.sched

    @staticmethod
    def lr_sequence(config, lr0, n, train_size=None, ticks0=0):
        """Host mirror of the tick's scheduler: the learning rates of `n` consecutive updates that start at rate `lr0` with `ticks0`
        ticks done -- the same double operations in the same order, hence the same bits as the device's and as the host loop's."""
        k, gamma, min_lr, restart_lr = _schedule(config, train_size)
        out, lr, ticks = [], float(lr0), int(ticks0)
        for _ in range(n):
            out.append(lr)
            ticks += 1
            if k > 0 and ticks % k == 0:
                lr = lr * gamma
            if lr < min_lr:
                lr = restart_lr
        return out

    # -- the step --------------------------------------------------------------------------------------------------------------------
    def observe(self, loss, rows):
        """Remember the step's loss (a float32 device scalar) for the NEXT tick, which adds it to loss_sum and `rows` to rows."""
        if not (torch.is_tensor(loss) and loss.is_cuda and loss.dtype is torch.float32 and loss.numel() == 1 and loss.device == self.buf.device):
            raise ValueError("DeviceStepState.observe takes the loss as a float32 scalar on the state's device")
        self._loss, self._rows = loss, int(rows)

    def tick(self):
        from . import _lib
        loss, rows, self._loss, self._rows = self._loss, self._rows, None, 0
        k, gamma, min_lr, restart_lr = self.sched
        with torch.cuda.device(self.buf.device):
            _lib.check(_lib.lib().mural_op_train_state_tick(self.buf.data_ptr(), None if loss is None else loss.data_ptr(), rows, self.betas[0],
                                                            self.betas[1], int(k), float(gamma), float(min_lr), float(restart_lr),
                                                            _lib.current_stream_ptr(self.buf.device)))


class _FlatStep:
    """What ``Adam``, ``AdamW`` and ``SGD`` below share: the flat layout of the parameters and of the optimiser's state tensors, the
    checks that decide whether the one launch covers a step, and the fall-through to the torch class's own step on the same state.

    A subclass names its torch class (``_TORCH``), the state tensors that become views of flat buffers (``_BUFFERS``), whether torch keeps
    a step counter per parameter (``_COUNTS``), which settings of a parameter group the launch covers (``_covers``) and the launch
    itself (``_launch``).

    ``p.data`` becomes a view of one flat buffer at the first covered step (``_enter_flat``; only when every parameter has state or none
    has) and the state tensors are views of buffers with the same slot layout (zero padding that stays zero).  ``_flat`` is (layout,
    parameters, parameter buffer, state buffers...) while the launch applies, None otherwise; leaving the layout keeps the views -- torch
    steps on them -- and materialises the step counters.  With a ``device_state`` the block counts the updates and holds the rate; a step
    that goes through torch reads both back first and ticks the block all the same, so the two routes stay one sequence."""

    _TORCH = None
    _BUFFERS = ()
    _COUNTS = True

    def _init_flat(self, device_state):
        self._flat = None          # (layout, params, param buffer, state buffers...) while the one-launch step applies
        self._flat_t = 0           # updates done (the step counters of torch's state, materialised on demand)
        self.device_state = device_state      # with one, the BLOCK counts the updates (_flat_t: its value at the last read-back)

    # -- torch's state <-> the flat buffers -----------------------------------------------------------------------------------
    def _state_to_host(self):
        """The block's step count and learning rate -> _flat_t and param_groups (one synchronising read)."""
        r = self.device_state.read()
        self._flat_t = r["step"]
        for g in self.param_groups:
            g["lr"] = r["lr"]

    def _materialise_steps(self):
        if self._flat is None:
            return
        if self.device_state is not None:
            self._state_to_host()
        self._write_steps()

    def _write_steps(self):
        if not self._COUNTS:
            return
        g = self.param_groups[0]
        on_dev = bool(g.get("fused")) or bool(g.get("capturable"))
        for p in self._flat[1]:
            self.state[p]["step"] = (torch.full((), float(self._flat_t), dtype=torch.float32, device=p.device) if on_dev
                                     else torch.tensor(float(self._flat_t), dtype=torch.float32))

    def _leave_flat(self):
        self._materialise_steps()
        self._flat = None

    def _enter_flat(self, lay, params):
        dev = params[0].device
        if any(p.dtype is not torch.float32 or p.device != dev or not p.is_cuda for p in params):
            return False
        have = [p for p in params if len(self.state.get(p, {}))]
        t = 0
        if have:
            if len(have) != len(params) or any(not torch.is_tensor(self.state[p].get(k)) for p in params for k in self._BUFFERS):
                return False
            if self._COUNTS:
                steps = torch.stack([self.state[p]["step"].detach().to(device=dev, dtype=torch.float32).reshape(()) for p in params])
                t = float(steps[0].item())
                if t != int(t) or not bool((steps == t).all().item()):
                    return False
        pf, *bufs = (torch.zeros(lay.total, dtype=torch.float32, device=dev) for _ in range(1 + len(self._BUFFERS)))
        for p, o in zip(lay.plist, lay.poffs):
            n = p.numel()
            slot = lambda f: f[o:o + n].view(p.shape)      # noqa: E731
            slot(pf).copy_(p.data)
            st = self.state[p]
            if have:
                for k, f in zip(self._BUFFERS, bufs):
                    slot(f).copy_(st[k])
            p.data = slot(pf)
            for k, f in zip(self._BUFFERS, bufs):
                st[k] = slot(f)
        self._flat, self._flat_t = (lay, list(lay.plist), pf, *bufs), int(t)
        if self.device_state is not None:
            self.device_state.set_step(int(t))      # torch's counters are the record while the flat layout is not entered
        self._write_steps()
        return True

    def _flat_step(self):
        if len(self.param_groups) != 1:
            return False
        g = self.param_groups[0]
        if g.get("maximize") or g.get("capturable") or g.get("differentiable") or torch.is_tensor(g["lr"]) or not self._covers(g):
            return False
        if self._flat is None:
            params = [p for p in g["params"] if p.numel()]
            from .model.step_layout import layout_of_params
            lay = layout_of_params(params, device_state=self.device_state is not None)
            if lay is None or lay.last_flat is None or not self._enter_flat(lay, params):
                return False
        lay, params, pf = self._flat[:3]
        flat = lay.last_flat
        if flat is None or flat.device != pf.device or flat.numel() != pf.numel():
            return False
        gbase, pbase = flat.data_ptr(), pf.data_ptr()
        for p, off in zip(params, lay.poffs):
            gr = p.grad
            if gr is None or gr.data_ptr() != gbase + 4 * off or p.data_ptr() != pbase + 4 * off:
                return False
        st = self.device_state
        if st is not None and (st.buf.device != pf.device or not self._state_fits(g, st)):
            return False
        if st is None:
            self._flat_t += 1
        from . import _lib
        with torch.cuda.device(pf.device):
            self._launch(_lib, g, [f.data_ptr() for f in self._flat[2:]], gbase, pf.numel(), st, _lib.current_stream_ptr(pf.device))
        model = lay.model_ref()
        if model is not None and not model.training:      # (a step in eval mode: the kernel bumps no tensor version the folded copy watches)
            model.invalidate_folded()
        return True

    def _state_fits(self, g, st):
        return True

    @torch.no_grad()
    def step(self, closure=None):
        # (torch wraps the step of every optimizer class -- this one too -- with its step hooks: they fire around either route; the
        # parent's step is called without ITS wrapper so that they do not fire twice)
        if closure is None and self._flat_step():
            return None
        if self.device_state is not None:      # torch's step on the block's count and rate; the block takes the step all the same
            self._state_to_host()
            if self._flat is not None:
                self._write_steps()
                self._flat = None
            self.device_state.tick()
        else:
            self._leave_flat()
        parent = self._TORCH.step
        if getattr(parent, "hooked", False):
            parent = getattr(parent, "__wrapped__", parent)
        return parent(self, closure)

    def state_dict(self):
        self._materialise_steps()
        return super().state_dict()

    def load_state_dict(self, state_dict):
        self._flat = None            # the loaded tensors replace the views; the next step lays them out again
        return super().load_state_dict(state_dict)


class Adam(_FlatStep, torch.optim.Adam):
    """``torch.optim.Adam`` (the reference's default optimiser, training.py:346-350, stepped at :432) with a ONE-launch step for a model
    whose training step runs in the library (model/train_step.py, model/indel_train_step.py): there every gradient is a view of one flat
    buffer, so the parameters and the two moment buffers are laid out the same way -- ``p.data`` becomes a view of one flat buffer at the
    first step, ``state[p]['exp_avg']`` / ``['exp_avg_sq']`` are views as well -- and the update is one elementwise kernel
    (``mural_op_adam_flat``: torch's fused update rule, bias corrections from the host) instead of torch's multi-tensor sequence (a
    step-counter foreach + three launches over ~150 tensor quadruples, 40 us at the end of every step with nothing beside them).

    Same constructor as ``torch.optim.Adam``.  Everything the one launch does not cover goes through ``torch.optim.Adam.step`` itself,
    on the same state tensors: more than one parameter group, amsgrad / maximize / capturable / differentiable, a tensor learning rate,
    a closure, parameters that are not exactly one HIP model's (or a model without the flat gradient buffer: the per-layer paths, CPU; a
    UNet_Small unless the optimiser carries a ``device_state``), a
    gradient that is not the latest backward's view.  ``state_dict`` / ``load_state_dict`` are torch's (step counters are materialised
    first).

    ``device_state=DeviceStepState(...)``: the step count, the bias corrections and the learning rate live in that device block, and
    the step is two launches -- ``mural_op_train_state_tick`` (step += 1, the two factors from the block's rate, the observed loss added,
    the per-batch scheduler) + ``mural_op_adam_flat_state`` -- that read nothing from the host, so ``GraphedTrainStep`` can capture them.
    A step the flat kernel does not cover still goes through torch: the block's step and rate are read back first (into the step
    counters and ``param_groups``) and the block is ticked all the same, so the two routes stay one sequence."""

    _TORCH = torch.optim.Adam
    _BUFFERS = ("exp_avg", "exp_avg_sq")

    def __init__(self, params, lr=1e-3, betas=(0.9, 0.999), eps=1e-8, weight_decay=0, amsgrad=False, device_state=None, **kw):
        params = list(params)
        if "fused" not in kw and "foreach" not in kw:      # torch's fused implementation for the steps that fall through, where it applies
            flat = [q for p in params for q in (p["params"] if isinstance(p, dict) else [p])]
            kw["fused"] = bool(flat) and all(torch.is_tensor(q) and q.is_cuda and q.is_floating_point() for q in flat)
        super().__init__(params, lr=lr, betas=betas, eps=eps, weight_decay=weight_decay, amsgrad=amsgrad, **kw)
        if device_state is not None and tuple(float(b) for b in betas) != device_state.betas:
            raise ValueError(f"betas {tuple(betas)} differ from the device state's {device_state.betas}")
        self._init_flat(device_state)

    def _covers(self, g):
        return not (g.get("amsgrad") or g.get("decoupled_weight_decay"))

    def _state_fits(self, g, st):
        return (float(g["betas"][0]), float(g["betas"][1])) == st.betas

    def _launch(self, _lib, g, ptrs, gbase, n, st, stream):
        pf, mf, vf = ptrs
        b1, b2 = g["betas"]
        if st is not None:
            st.tick()
            _lib.check(_lib.lib().mural_op_adam_flat_state(pf, gbase, mf, vf, n, st.buf.data_ptr(), float(b1), float(b2), float(g["eps"]),
                                                           float(g["weight_decay"]), stream))
        else:
            _lib.check(_lib.lib().mural_op_adam_flat(pf, gbase, mf, vf, n, float(g["lr"]), float(b1), float(b2), float(g["eps"]),
                                                     float(g["weight_decay"]), self._flat_t, stream))


class AdamW(_FlatStep, torch.optim.AdamW):
    """``torch.optim.AdamW`` (the reference's 'AdamW' / 'AdamW2', training.py:351-356: ``amsgrad=True``) with the one-launch step of ``Adam``
    above: parameters, ``exp_avg``, ``exp_avg_sq`` and ``max_exp_avg_sq`` in flat buffers of one slot layout, stepped by
    ``mural_op_adamw_amsgrad_flat`` (decoupled decay, then the amsgrad update).  Same constructor as ``torch.optim.AdamW``; what the launch
    does not cover -- ``amsgrad=False`` and every case listed for ``Adam`` -- is ``torch.optim.AdamW.step`` on the same state tensors.

    ``device_state``: tick + ``mural_op_adamw_amsgrad_flat_state``, which reads the two bias-correction floats and the rate from the block.
    The rate it finds there is the one the tick's scheduler left for the NEXT update: at a tick where the scheduler moves the rate, the
    decoupled decay ``1 - lr weight_decay`` of this update is formed from the new rate, one update earlier than on the host loop (the
    Adam part of the update uses the tick's ``step_size``, formed from this update's rate)."""

    _TORCH = torch.optim.AdamW
    _BUFFERS = ("exp_avg", "exp_avg_sq", "max_exp_avg_sq")

    def __init__(self, params, lr=1e-3, betas=(0.9, 0.999), eps=1e-8, weight_decay=1e-2, amsgrad=False, device_state=None, **kw):
        super().__init__(params, lr=lr, betas=betas, eps=eps, weight_decay=weight_decay, amsgrad=amsgrad, **kw)
        if device_state is not None and tuple(float(b) for b in betas) != device_state.betas:
            raise ValueError(f"betas {tuple(betas)} differ from the device state's {device_state.betas}")
        self._init_flat(device_state)

    def _covers(self, g):
        return bool(g.get("amsgrad"))

    _state_fits = Adam._state_fits

    def _launch(self, _lib, g, ptrs, gbase, n, st, stream):
        pf, mf, vf, xf = ptrs
        b1, b2 = g["betas"]
        if st is not None:
            st.tick()
            _lib.check(_lib.lib().mural_op_adamw_amsgrad_flat_state(pf, gbase, mf, vf, xf, n, st.buf.data_ptr(), float(b1), float(b2),
                                                                    float(g["eps"]), float(g["weight_decay"]), stream))
        else:
            _lib.check(_lib.lib().mural_op_adamw_amsgrad_flat(pf, gbase, mf, vf, xf, n, float(g["lr"]), float(b1), float(b2), float(g["eps"]),
                                                              float(g["weight_decay"]), self._flat_t, stream))


class SGD(_FlatStep, torch.optim.SGD):
    """``torch.optim.SGD`` (the reference's 'SGD', training.py:357-360: momentum 0.98, nesterov) with the one-launch step of ``Adam`` above:
    parameters and ``momentum_buffer`` in flat buffers of one slot layout, stepped by ``mural_op_sgd_flat`` (a zero buffer gives torch's
    first step, so entering the layout before any state exists needs no flag).  Same constructor as ``torch.optim.SGD``; what the launch
    does not cover -- no nesterov momentum, dampening, and every case listed for ``Adam`` -- is ``torch.optim.SGD.step`` on the same state.

    ``device_state``: ``mural_op_sgd_flat_state`` reads the rate from the block, then the tick advances the block (count, loss sum,
    scheduler) -- in this order, so the update runs at the rate the previous tick left for it, as on the host loop.  The tick's betas are
    the state's; its two bias-correction floats go unused."""

    _TORCH = torch.optim.SGD
    _BUFFERS = ("momentum_buffer",)
    _COUNTS = False

    def __init__(self, params, *args, device_state=None, **kw):
        super().__init__(params, *args, **kw)
        self._init_flat(device_state)

    def _covers(self, g):
        return bool(g.get("nesterov")) and g.get("momentum", 0) > 0 and not g.get("dampening")

    def _launch(self, _lib, g, ptrs, gbase, n, st, stream):
        pf, bf = ptrs
        if st is not None:
            _lib.check(_lib.lib().mural_op_sgd_flat_state(pf, gbase, bf, n, st.buf.data_ptr(), float(g["momentum"]),
                                                          float(g["weight_decay"]), stream))
            st.tick()
        else:
            _lib.check(_lib.lib().mural_op_sgd_flat(pf, gbase, bf, n, float(g["lr"]), float(g["momentum"]), float(g["weight_decay"]), stream))


# ------------------------------------------------------------------------------------------------------------------
# the reference's epoch loop (MuRaL/training.py:346-450) around the HIP models: optimiser / scheduler choice and the
# per-batch policy (skip batches of one row, clip at 10, step the scheduler every batch, restart a learning rate that decayed
# below min_lr).  Host logic only; the model does the device work.
# ------------------------------------------------------------------------------------------------------------------
def make_optimizer(config, params, device_state=None):
    """training.py:346-360: Adam / AdamW / AdamW2 (both amsgrad) / SGD (momentum 0.98, nesterov) by ``config['optim']``."""
    params = [p for p in params if p.requires_grad]
    lr, wd = config["learning_rate"], config["weight_decay"]
    name = config["optim"]
    # the torch classes with one launch per step behind the library's training step (device_state: tick + one launch, capturable)
    if name == "Adam":
        return Adam(params, lr=lr, weight_decay=wd, device_state=device_state)
    if name in ("AdamW", "AdamW2"):
        return AdamW(params, lr=lr, weight_decay=wd, amsgrad=True, device_state=device_state)
    if name == "SGD":
        return SGD(params, lr=lr, weight_decay=wd, momentum=0.98, nesterov=True, device_state=device_state)
    raise ValueError(f"Error: unsupported optimization method {name}")


def make_scheduler(config, optimizer, train_size=None):
    """training.py:364-373: 'StepLR' (step_size (5000 * 128) // batch_size, gamma LR_gamma), 'StepLR2' (per-step decay from
    restart_lr to min_lr over one epoch), 'ROP' (ReduceLROnPlateau)."""
    kind = config["lr_scheduler"]
    if kind == "StepLR":
        return torch.optim.lr_scheduler.StepLR(optimizer, step_size=(5000 * 128) // config["batch_size"], gamma=config["LR_gamma"])
    if kind == "StepLR2":
        gamma = (config["min_lr"] / config["restart_lr"]) ** (1 / (train_size // config["batch_size"]))
        return torch.optim.lr_scheduler.StepLR(optimizer, step_size=1, gamma=gamma)
    if kind == "ROP":
        return torch.optim.lr_scheduler.ReduceLROnPlateau(optimizer, mode="min", factor=0.2, patience=1, threshold=0.0001, min_lr=1e-7)
    raise ValueError(f"unknown lr_scheduler {kind}")


def train_epoch(model, batches, criterion, optimizer, scheduler, config, device, model_type="snv", epoch=0):
    """One epoch of training.py:392-450 over an iterable of ``(y, cont_x, cat_x, distal_x)`` batches (the order
    ``generate_data_batches`` yields them).  Returns the summed loss."""
    model.train()
    freeze_host_heap()
    if epoch > 0 and config["lr_scheduler"] == "StepLR2":
        for g in optimizer.param_groups:
            g["lr"] = config["restart_lr"]
    total_loss = 0.0
    for y, cont_x, cat_x, distal_x in batches:
        if y.shape[0] == 1:                       # a single row cannot feed a batch-statistics BatchNorm (training.py:415)
            continue
        cat_x, cont_x, distal_x, y = cat_x.to(device), cont_x.to(device), distal_x.to(device), y.to(device)
        preds = model.forward((cont_x, cat_x), distal_x) if model_type == "snv" else model.forward(distal_x)
        loss = criterion(preds, y.long().squeeze())
        optimizer.zero_grad()
        loss.backward()
        clip_grad_norm_(model, 10)
        optimizer.step()
        total_loss += loss.item()
        if config["lr_scheduler"] != "ROP":
            scheduler.step()
            if optimizer.param_groups[0]["lr"] < config["min_lr"]:      # avoid very small learning rates
                for g in optimizer.param_groups:
                    g["lr"] = config["restart_lr"]
    return total_loss


def _device_epoch_refusal(model, criterion, optimizer, model_type="snv"):
    if model_type == "snv":
        from .model import train_step
        from .model.model_snv import Network0, _HipSnvBase
        core = model.model if isinstance(model, Network0) else model
        if not isinstance(core, _HipSnvBase) or not train_step.supported(core):
            return "the model does not train on the one-call step (an SNV model with 32 conv channels of kernel 3, or the local-only one)"
    else:
        import os
        from .model.model_indel import UNet_Small
        if not isinstance(model, UNet_Small) or os.environ.get("MURAL_INDEL_TRAIN_PER_UNIT"):
            return "the model does not train on the one-call step (a UNet_Small, without MURAL_INDEL_TRAIN_PER_UNIT)"
    if not isinstance(optimizer, _FlatStep) or optimizer.device_state is None:
        return "the optimizer is not mural_amd.train.Adam / AdamW / SGD(..., device_state=DeviceStepState(...))"
    if not isinstance(criterion, (CrossEntropySum, torch.nn.CrossEntropyLoss)):
        return "the criterion is not a cross-entropy loss giving one float32 device scalar"
    return None


def _device_eager_step(model, criterion, optimizer, cont_x, cat_x, distal_x, y, model_type="snv"):
    loss = criterion(model((cont_x, cat_x), distal_x) if model_type == "snv" else model(distal_x), y)
    optimizer.zero_grad()
    loss.backward()
    clip_grad_norm_(model, 10)
    optimizer.device_state.observe(loss, y.shape[0])
    optimizer.step()


def _graphed_epoch_step(model, criterion, optimizer, sched, cont_x, cat_x, distal_x, y, model_type="snv"):
    """(the model's captured step for batches of y's rows, whether it was captured just now -- its one warm-up step then WAS the step
    on this batch).  Captured again when what the graph baked in is gone: another optimiser / criterion / schedule, parameters that
    left the optimiser's flat buffer, another input form."""
    steps = model.__dict__.setdefault("_device_epoch_steps", {})
    x = GraphedTrainStep._tensor(distal_x)
    hit = steps.get(y.shape[0])
    if hit is not None:
        step, key, pbase = hit
        flat = optimizer._flat
        if (key == (id(optimizer), id(criterion), sched) and step.opt is optimizer and step.crit is criterion and flat is not None
                and flat[2].data_ptr() == pbase and step.x.shape == x.shape and step.x.dtype == x.dtype):
            return step, False
    if model_type == "snv":
        step = GraphedTrainStep(model, optimizer, criterion, cont_x, cat_x, distal_x, y, max_norm=10, warmup=1)
    else:
        step = GraphedIndelTrainStep(model, optimizer, criterion, distal_x, y, max_norm=10, warmup=1)
    if optimizer._flat is None:
        raise RuntimeError("train_epoch_device: the optimiser did not take its one-launch step on this model")
    steps[y.shape[0]] = (step, (id(optimizer), id(criterion), sched), optimizer._flat[2].data_ptr())
    return step, True


def train_epoch_device(model, batches, criterion, optimizer, config, device, epoch=0, train_size=None, model_type="snv"):
    """``train_epoch`` with the loop's state on the device (``optimizer = make_optimizer(config, params, device_state=DeviceStepState(...))``:
    this module's ``Adam``, ``AdamW`` or ``SGD``): the same policy -- batches of one row skipped, clipping at 10, the scheduler of ``config``
    ticked every batch unless 'ROP', the restart of a rate below min_lr, the rate reset to restart_lr for 'StepLR2' when epoch > 0 -- with
    the scheduler inside the tick kernel instead of a host ``scheduler`` object, and NOTHING read back before the epoch's end:

      * batches of ``config['batch_size']`` rows replay a ``GraphedTrainStep`` (``model_type="indel"``: a ``GraphedIndelTrainStep``, on dense
        windows or ``SymbolWindows``) captured once per (model, rows) and kept on the model;
      * batches of any other size (the carry batches of ``epoch_order``) run the same kernels eagerly, so the block sees one sequence;
      * at the end ONE ``state.read()``: ``param_groups[..]['lr']`` is set from it (a host ``ReduceLROnPlateau`` can act between epochs),
        the deferred input check of the last replay is raised, the block's loss sum is returned.

    Models on a one-call training step (the SNV models ``train_step.supported`` names, ``UNet_Small``) with one of this module's optimisers
    on a device state and a cross-entropy criterion; anything else raises ValueError (``train_epoch`` is the loop for it)."""
    why = _device_epoch_refusal(model, criterion, optimizer, model_type)
    if why is not None:
        raise ValueError(f"train_epoch_device: {why}; use train_epoch")
    state = optimizer.device_state
    model.train()
    freeze_host_heap()
    if epoch > 0 and config["lr_scheduler"] == "StepLR2":
        for g in optimizer.param_groups:
            g["lr"] = config["restart_lr"]
    sched = state.set_schedule(config, train_size)
    state.set_lr(optimizer.param_groups[0]["lr"])
    state.reset_epoch()
    common, graphed = int(config["batch_size"]), None
    for y, cont_x, cat_x, distal_x in batches:
        if y.shape[0] == 1:                       # a single row cannot feed a batch-statistics BatchNorm (training.py:415)
            continue
        cat_x, cont_x, distal_x, y = cat_x.to(device), cont_x.to(device), distal_x.to(device), y.to(device).long().squeeze()
        if y.shape[0] == common:
            graphed, fresh = _graphed_epoch_step(model, criterion, optimizer, sched, cont_x, cat_x, distal_x, y, model_type)
            if not fresh:
                graphed(cont_x, cat_x, distal_x, y) if model_type == "snv" else graphed(distal_x, y)
        else:
            _device_eager_step(model, criterion, optimizer, cont_x, cat_x, distal_x, y, model_type)
    r = state.read()
    optimizer._flat_t = r["step"]
    for g in optimizer.param_groups:
        g["lr"] = r["lr"]
    if graphed is not None:
        graphed.finish()
    return r["loss_sum"]
