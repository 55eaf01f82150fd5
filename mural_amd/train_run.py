"""A training run from files: the epoch loop of the reference's ``train()`` (MuRaL/training.py:387-568) around the pieces that already
run on the device -- ``train_epoch_device`` (graph-replayed steps), the eval forward, the validation analytics of
``mural_amd.evaluation`` -- with the checkpoints, the per-epoch metrics file, early stopping and ``ReduceLROnPlateau`` between epochs.

  * ``validate_epoch``     -- probabilities and loss sum of a loader or a view, written batch by batch into one table; one read-back.
  * ``validation_report``  -- training.py:478-520: FullDiri calibrator fitted on those probabilities, the ``Evaluator`` reports before
                              and after calibration (and after Poisson calibration), printed with the reference's labels.
  * ``EarlyStopping``      -- the contract of the reference's class: ``__call__(loss, model)``, ``.early_stop``, ``.counter``.
  * ``fit``                -- the loop; ``prepare_model`` -- a fresh or a pretrained model for it.

Reproducibility rule of ``fit``: with ``split_generator_seed=s`` the batches of epoch ``e`` are drawn with
``torch.Generator().manual_seed(s + e)``; with None they come from torch's global generator.
"""
import os

import numpy as np
import torch

from . import _lib
from . import train as TR
from .calibration import calibrate_device
from .evaluation import Evaluator, calibrate_prob
from .model.nn_utils import model_choice, save_model, weights_init

METRIC_KEYS = ("loss", "fdiri_loss", "after_min_loss", "score", "total_params")      # training.py:538-544, in this order


# ------------------------------------------------------------------------------------------------------------------
# host logic
# ------------------------------------------------------------------------------------------------------------------
class EarlyStopping:
    """Stop when the validation loss has not improved for `patience` calls in a row.  ``stopper(loss, model)`` once per epoch: the
    first loss, and every loss with ``-loss >= best + delta``, becomes the best one and resets ``counter``; any other loss adds one to
    ``counter`` and sets ``early_stop`` once it reaches `patience`.  (`model` is accepted and unused: nothing is saved here, the loop
    writes a checkpoint every epoch.)"""

    def __init__(self, patience=7, verbose=False, delta=0, trace_func=print):
        self.patience, self.verbose, self.delta, self.trace_func = patience, verbose, delta, trace_func
        self.counter, self.best_score, self.early_stop, self.val_loss_min = 0, None, False, float("inf")

    def __call__(self, val_loss, model=None):
        score = -val_loss
        if self.best_score is not None and score < self.best_score + self.delta:
            self.counter += 1
            self.trace_func(f"EarlyStopping counter: {self.counter} out of {self.patience}")
            if self.counter >= self.patience:
                self.early_stop = True
            return
        if self.verbose:
            self.trace_func(f"Validation loss decreased ({self.val_loss_min:.6f} --> {val_loss:.6f}).")
        self.best_score, self.val_loss_min, self.counter = score, val_loss, 0


def auto_weight_decay(weight_decay_auto, batch_size, epochs, train_size):
    """``--weight_decay_auto`` (training.py:338-344): the decay per step that shrinks a weight to `weight_decay_auto` of itself over
    the whole run, ``1 - weight_decay_auto ** (batch_size / (epochs * train_size))``.  Values outside (0, 1) raise ValueError."""
    if not 0 < weight_decay_auto < 1:
        raise ValueError("Please set a value smaller than 1 (and above 0) for --weight_decay_auto.")
    return 1 - weight_decay_auto ** (batch_size / (epochs * train_size))


def checkpoint_path(trial_dir, epoch):
    """``<trial_dir>/checkpoint_<epoch>/model`` (training.py:592-601); the directory is created."""
    d = os.path.join(os.fspath(trial_dir), f"checkpoint_{epoch}")
    os.makedirs(d, exist_ok=True)
    return os.path.join(d, "model")


def metrics_text(metrics):
    """The text of ``epoch_<N>_metrics.txt`` (training.py:538-547, :581-586): ``key: value`` lines of the five keys, in their order."""
    return "".join(f"{k}: {metrics[k]}\n" for k in METRIC_KEYS)


def write_metrics(metrics, trial_dir, epoch):
    path = os.path.join(os.fspath(trial_dir), f"checkpoint_{epoch}", f"epoch_{epoch}_metrics.txt")
    with open(path, "w") as f:
        f.write(metrics_text(metrics))
    return path


def default_emb_dims(local_radius, local_order, model_type="snv"):
    """training.py:250-254 for a sequence-only model: one (categories, min(16, int(categories ** 0.25))) pair per local column, with
    4 ** local_order k-mers and the padding id for a k-mer that holds an N (the reference counts the ids that occur in its data; a
    table sized for every id serves any data).  The reference writes the list into an INDEL model's config too (its local window has
    no middle column), and ``load_model`` reads it from every config."""
    n = 4 ** int(local_order) + 1
    return [(n, min(16, int(n ** 0.25)))] * (2 * int(local_radius) + (1 if model_type == "snv" else 0) - (int(local_order) - 1))


# ------------------------------------------------------------------------------------------------------------------
# the model of a run
# ------------------------------------------------------------------------------------------------------------------
def prepare_model(config, device, *, model_path=None, init_fc_with_pretrained=True, model_type="snv"):
    """The model ``fit`` trains: ``model_choice`` on `config` (``emb_dims`` and the sequence-only constants are filled in where the
    config lacks them) and ``weights_init``, or, with `model_path`, the transfer-learning start of training.py:289-321: the state
    dict loaded, every parameter trainable, and -- unless `init_fc_with_pretrained` -- the last layer of each head (``local_fc[-1]``,
    ``distal_fc1[-1]``, ``distal_fc2[-1]``, where the model has them) initialised afresh.  For an INDEL model that last option raises
    ValueError, where the reference exits.

    There is no frozen-body path: the reference's ``train_all=False`` branch names a ``distal_fc`` attribute that none of its
    current models has, and its command line forces ``train_all=True``."""
    config.setdefault("emb_dims", default_emb_dims(config["local_radius"], config["local_order"], model_type))
    config.setdefault("seq_only", True)
    common = {"emb_dims": config["emb_dims"], "n_cont": 0, "n_class": config["n_class"], "distal_order": 1, "in_channels": 4}
    model = model_choice(config["model_no"], config, common, model_type)
    if model_path is None:
        model.apply(weights_init)
        return model.to(device)
    if not init_fc_with_pretrained and model_type == "indel":
        raise ValueError("transfer learning for an INDEL model fine-tunes every parameter from the pretrained values: "
                         "init_fc_with_pretrained=False is not supported")
    model.load_state_dict(torch.load(model_path, map_location="cpu", weights_only=True))
    for p in model.parameters():
        p.requires_grad = True
    if not init_fc_with_pretrained:
        for name in ("local_fc", "distal_fc1", "distal_fc2"):
            head = getattr(model, name, None)
            if head is not None:
                head[-1].apply(weights_init)
    return model.to(device)


# ------------------------------------------------------------------------------------------------------------------
# the validation epoch
# ------------------------------------------------------------------------------------------------------------------
def _plain_ce_sum(criterion):
    """Is `criterion` exactly the summed cross entropy ``mural_op_ce_sum_fwd`` computes (softmax and loss in one launch)?"""
    if type(criterion) is TR.CrossEntropySum:
        return True
    return (type(criterion) is torch.nn.CrossEntropyLoss and criterion.reduction == "sum" and criterion.weight is None
            and criterion.ignore_index == -100 and criterion.label_smoothing == 0.0)


def _eval_forward(model, cont_x, cat_x, distal_x, model_type):
    from .data.genome import SymbolWindows
    if model_type != "snv":
        return model(distal_x)
    if isinstance(distal_x, SymbolWindows):
        if getattr(model, "symbols_entry_ok", lambda: False)():
            return model.forward_symbols(cat_x, distal_x.sym)
        sym = distal_x.sym.contiguous()          # a model on the per-layer eval path: the dense window the bytes stand for
        distal_x = torch.empty((sym.shape[0], 4, sym.shape[1]), dtype=torch.float32, device=sym.device)
        with torch.cuda.device(sym.device):
            _lib.check(_lib.lib().mural_op_symbols_to_dense(sym.data_ptr(), sym.shape[0], sym.shape[1], distal_x.data_ptr(),
                                                           _lib.current_stream_ptr(sym.device)))
    return model((cont_x, cat_x), distal_x)


def validate_epoch(model, loader, criterion, device, model_type="snv"):
    """(prob (N, n_class) float32 on the device, loss sum) of `loader` (an ``EpochLoader`` or a view of one) in validation order,
    ``epoch(shuffle=False)``: the model in eval mode under ``no_grad``, every batch evaluated (one of a single row too: only training
    skips those), its probabilities -- the softmax of the model output, training.py:470 -- written into the table at the batch's
    offset, its loss added to a float64 device scalar that is read back once at the end.  With the plain summed cross entropy
    (``CrossEntropySum``, ``nn.CrossEntropyLoss(reduction='sum')``) softmax and loss are one launch per batch
    (``mural_op_ce_sum_fwd``, writing into the table); any other criterion is called as it is, beside ``torch.softmax``."""
    device = torch.device(device)
    model.eval()
    TR.freeze_host_heap()
    n = len(loader)
    prob, off = None, 0
    loss = torch.zeros((), dtype=torch.float64, device=device)
    fused = _plain_ce_sum(criterion)
    lib = _lib.lib() if fused else None
    with torch.no_grad():
        for y, cont_x, cat_x, distal_x in loader.epoch(shuffle=False):
            b = y.shape[0]
            out = _eval_forward(model, cont_x.to(device), cat_x.to(device), distal_x.to(device), model_type)
            target = y.to(device).long().squeeze(1)
            if prob is None:
                prob = torch.empty((n, out.shape[1]), dtype=torch.float32, device=device)
            if off + b > n:
                raise RuntimeError(f"validate_epoch: the loader yields more rows than its length {n}")
            rows = prob[off:off + b]
            if fused and out.dtype is torch.float32 and out.is_cuda:
                out = out.contiguous()
                part = torch.empty((), dtype=torch.float32, device=device)
                with torch.cuda.device(device):
                    _lib.check(lib.mural_op_ce_sum_fwd(out.data_ptr(), target.data_ptr(), b, out.shape[1], rows.data_ptr(), part.data_ptr(),
                                                       _lib.current_stream_ptr(device)))
                loss.add_(part)
            else:
                loss.add_(criterion(out, target).double())
                torch.softmax(out, dim=1, out=rows)
            off += b
    if off != n:
        raise RuntimeError(f"validate_epoch: the loader yielded {off} rows, its length is {n}")
    check = getattr(getattr(model, "model", model), "check_encoding", None)     # Network0 wraps its body in .model
    if check is not None:
        check(wait=True)
    if prob is None:
        prob = torch.empty((0, getattr(model, "n_class", 0)), dtype=torch.float32, device=device)
    return prob, float(loss.item())


def validation_report(view_rows, prob, valid_size, n_class, model_type, poisson_calib=False, printer=print, valid_loss_sum=None,
                      train_loss=None):
    """The per-epoch report of training.py:478-520 from device tensors.  `view_rows`: ``loader.rows(local_order=1)`` of the validation
    rows (chromosome, start, label, ORDER-1 local codes -- the columns the k-mer reports read), `prob` the table of
    ``validate_epoch``.  In the reference's order: the FullDiri calibrator fitted on `prob` (NLL / ECE / CwECE / Brier before and
    after), k-mer correlations (3/5/7, INDEL 2/4/6) before and after calibration, the loss lines, regional scores over the first two
    k, regional correlations in 100 kb and 500 kb windows -- each also for Poisson-calibrated probabilities when `poisson_calib` is
    set or the model is INDEL.  Reductions run on the device (``mural_amd.evaluation``); only their small tables reach the host.

    Returns ``dict(loss, fdiri_loss, score, calibrator, ...)``: ``loss`` = `valid_loss_sum` / `valid_size` (None without the sum),
    ``calibrator`` the fitted (n_class, n_class + 1) weights, and per variant (``before``, ``fdiri``, ``poisson``) the ``kmer``,
    ``corr_list``, ``score`` and ``regional_corr`` values."""
    codes, label = view_rows.local, view_rows.label
    weights, fdiri_nll, prob_cal = calibrate_prob(prob, label, printer=printer, calibr_name="FullDiri")
    variants = [("before", "no_calibra", prob), ("fdiri", "FullDiri", prob_cal)]
    if poisson_calib or model_type == "indel":
        variants.append(("poisson", "Poisson", calibrate_device(prob, poisson=True, input_is_prob=True)))
    evs = [(tag, Evaluator(codes, label, p, n_class, calibra=name, printer=printer, model_type=model_type)) for tag, name, p in variants]
    kmer_list = [2, 4, 6] if model_type == "indel" else [3, 5, 7]
    out = {tag: {} for tag, _ in evs}
    for tag, ev in evs:
        out[tag]["kmer"] = ev.evaluate_kmer(kmer_list)
    loss = None if valid_loss_sum is None else valid_loss_sum / valid_size
    if train_loss is not None:
        printer("Training Loss: ", train_loss)
    if loss is not None:
        printer("Validation Loss: ", loss)
    printer("Validation Loss (after fdiri_cal): ", fdiri_nll)
    for tag, ev in evs:
        out[tag]["corr_list"], out[tag]["score"], out[tag]["n_regions"] = ev.evaluate_regional_score(valid_size, kmer_list[:2])
    for tag, ev in evs:
        out[tag]["regional_corr"] = ev.evaluate_regional_corr(view_rows.chrom_id, view_rows.start)
    out.update(loss=loss, fdiri_loss=fdiri_nll, score=out["before"]["score"], calibrator=weights)
    return out


def write_valid_preds(path, view_rows, prob, chrom_names, strand=None):
    """``--save_valid_preds`` (evaluation.py:529-543): chrom, start, end, strand, mut_type and the probabilities of the validation
    rows, sorted by (chrom, start), tab-separated with ``%.4g`` probabilities, gzip."""
    import gzip
    names = np.asarray(chrom_names, dtype=object)[view_rows.chrom_id.cpu().numpy()]
    start, label, p = view_rows.start.cpu().numpy(), view_rows.label.cpu().numpy(), prob.cpu().numpy()
    sign = np.full(len(start), "+", dtype=object) if strand is None else np.where(strand.cpu().numpy() != 0, "-", "+")
    order = sorted(range(len(start)), key=lambda i: (names[i], start[i]))
    with gzip.open(path, "wt") as f:
        f.write("\t".join(["chrom", "start", "end", "strand", "mut_type"] + [f"prob{k}" for k in range(p.shape[1])]) + "\n")
        for i in order:
            f.write("\t".join([names[i], str(start[i]), str(start[i] + 1), sign[i], str(label[i])] + ["%.4g" % v for v in p[i]]) + "\n")


# ------------------------------------------------------------------------------------------------------------------
# the run
# ------------------------------------------------------------------------------------------------------------------
def fit(model, config, train, valid, *, epochs, trial_dir, grace_period, device, model_type="snv", device_loop=True,
        split_generator_seed=None, save_valid_preds=False, poisson_calib=False, printer=print, criterion=None, optimizer=None, timings=None):
    """The epoch loop of training.py:387-568.  `train` / `valid`: ``EpochLoader``s or views of one (``EpochLoader.split``), `config` the
    reference's dict (``optim``, ``learning_rate``, ``weight_decay``, ``lr_scheduler``, ``LR_gamma``, ``min_lr``, ``restart_lr``,
    ``batch_size`` and the model's keys; it is pickled beside every checkpoint).  Per epoch, in order:

      1. ``train_epoch_device`` over ``train.epoch(shuffle=True)`` with ``train_size=len(train)``.  With ``device_loop=False``, or
         where the model / optimiser / criterion is not one the device loop takes, ``train_epoch`` with ``make_scheduler`` runs
         instead; the fallback is announced once through `printer`.
      2. ``validate_epoch`` over `valid`, 3. ``validation_report``,
      4. ``save_model`` into ``<trial_dir>/checkpoint_<epoch>/model`` (+ ``.fdiri_cal.pkl``, ``.config.pkl``),
      5. ``checkpoint_<epoch>/epoch_<epoch>_metrics.txt`` (loss, fdiri_loss, after_min_loss, score, total_params),
      6. the minimum-loss book-keeping, 7. ``EarlyStopping(grace_period)`` -- the run ends after the epoch that trips it --,
      8. for 'ROP', ``scheduler.step(validation loss)``: the rate it leaves in ``param_groups`` is the one ``train_epoch_device``
         writes into the device block at the start of the next epoch.

    The batches of epoch ``e`` are drawn with ``torch.Generator().manual_seed(split_generator_seed + e)``: a run with a seed is
    reproducible; with None torch's global generator is used.  `criterion` defaults to ``CrossEntropySum()``, `optimizer` to
    ``make_optimizer(config, ...)`` (on a ``DeviceStepState`` for the device loop).

    `timings`: a dict that receives, per epoch, the seconds of ``train``, ``validate``, ``report`` and ``save`` (lists; the device is
    synchronised at each boundary, which a run without the dict never is).

    Returns (history, best_epoch): one dict per epoch run -- the five metrics, ``epoch``, ``train_loss`` (per row), ``lr`` (the rate
    after the epoch's training), ``report`` (``validation_report``'s dict), ``checkpoint`` -- and the reference's
    ``best_epoch = last epoch - early_stopping.counter``."""
    device = torch.device(device)
    criterion = TR.CrossEntropySum() if criterion is None else criterion
    if optimizer is None:
        state = TR.DeviceStepState(device, config["learning_rate"]) if device_loop else None
        optimizer = TR.make_optimizer(config, model.parameters(), device_state=state)
    on_device = bool(device_loop)
    if on_device:
        why = TR._device_epoch_refusal(model, criterion, optimizer, model_type)
        if why is not None:
            printer(f"NOTE: the device training loop does not apply ({why}); using the host loop (train_epoch)")
            on_device = False
            if getattr(optimizer, "device_state", None) is not None:
                optimizer = TR.make_optimizer(config, model.parameters())
    else:
        printer("NOTE: device_loop=False; using the host loop (train_epoch)")
    train_size, valid_size = len(train), len(valid)
    printer("train_size, valid_size:", train_size, valid_size)
    scheduler = None
    if not on_device or config["lr_scheduler"] == "ROP":
        scheduler = TR.make_scheduler(config, optimizer, train_size)
    total_params = sum(p.numel() for p in model.parameters() if p.requires_grad)
    n_class = config["n_class"]
    rows = valid.rows(local_order=1)
    stopper = EarlyStopping(patience=grace_period, verbose=True, trace_func=printer)
    history = []

    def lap(name, t0):
        if timings is None:
            return None
        import time
        torch.cuda.synchronize(device)
        now = time.perf_counter()
        if name is not None:
            timings.setdefault(name, []).append(now - t0)
        return now

    min_loss = min_loss_epoch = after_min_loss = 0
    epoch = -1
    for epoch in range(epochs):
        gen = None if split_generator_seed is None else torch.Generator().manual_seed(int(split_generator_seed) + epoch)
        batches = train.epoch(shuffle=True, generator=gen)
        t0 = lap(None, 0)
        if on_device:
            total = TR.train_epoch_device(model, batches, criterion, optimizer, config, device, epoch=epoch, train_size=train_size,
                                          model_type=model_type)
        else:
            total = TR.train_epoch(model, batches, criterion, optimizer, scheduler, config, device, model_type=model_type, epoch=epoch)
        lr = optimizer.param_groups[0]["lr"]
        printer("optimizer learning rate:", lr)
        t0 = lap("train", t0)
        prob, valid_total = validate_epoch(model, valid, criterion, device, model_type)
        t0 = lap("validate", t0)
        report = validation_report(rows, prob, valid_size, n_class, model_type, poisson_calib=poisson_calib, printer=printer,
                                   valid_loss_sum=valid_total, train_loss=total / train_size)
        t0 = lap("report", t0)
        save_path = checkpoint_path(trial_dir, epoch)
        if save_valid_preds:
            write_valid_preds(save_path + ".valid_preds.tsv.gz", rows, prob, valid.chrom_names, getattr(rows, "strand", None))
        save_model(model, report["calibrator"], config, save_path)
        current = valid_total / valid_size
        if epoch == 0 or current < min_loss:
            min_loss, min_loss_epoch, after_min_loss = current, epoch, 0
        else:
            after_min_loss = epoch - min_loss_epoch
        stopper(current, model)
        metrics = dict(loss=current, fdiri_loss=report["fdiri_loss"], after_min_loss=after_min_loss, score=report["score"],
                       total_params=total_params)
        write_metrics(metrics, trial_dir, epoch)
        lap("save", t0)
        history.append(dict(metrics, epoch=epoch, train_loss=total / train_size, lr=lr, report=report, checkpoint=save_path))
        if stopper.early_stop:
            printer("Early stopping")
            break
        if config["lr_scheduler"] == "ROP":
            scheduler.step(current)
    best_epoch = epoch - stopper.counter
    printer(f"Best Epoch: {best_epoch}")
    return history, best_epoch
