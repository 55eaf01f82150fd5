"""A training run from files (mural_amd.train_run, EpochLoader.split / rows) on a fixture small enough for seconds per test: two
chromosomes of about 30 kb (one with a run of N), 600 BED rows, segments of 8 kb (16 (segment, strand) groups, 3 of them to
validation), local radius 5 of order 2, batches of 64 out of groups of 2 segments: training epochs with carried tails and a short
last batch, a validation epoch with a short tail batch, and a second batch size chosen so that validation ends on a batch of ONE row.

distal_radius is 110, not smaller: the SNV models refuse windows of 200 columns and less (their middle tower reads the central 201),
as the reference's do.

Bars.  Probabilities and eval outputs of the same kernels on the same batches: ``torch.equal``.  The validation loss against
``model_predict_m``: the float32 summation rule of tests/_parity.py for a sum of that many rows.  Training losses of two runs of the
same steps, and the device loop against the host loop: 1e-3 relative, the bar tests/test_gpu_train_state.py and
tests/test_gpu_train_device_all.py hold between two such loops (the training step accumulates with floating-point atomics; it is not
bit-reproducible run to run, see tests/test_gpu_epoch_loader.py).  Learning rates: ``==``."""
import copy
import os

import numpy as np
import pytest
import torch

from tests._parity import U24
from tests.test_gpu_indel_train_symbols import DOWN

pytestmark = pytest.mark.gpu

R_LOCAL, ORDER, R_DISTAL, BATCH, SEGMENT, SAMPLED = 5, 2, 110, 64, 8000, 2
RATIO, SPLIT_SEED, RUN_SEED = 0.2, 15, 11
SNV_CFG = dict(model_no=2, n_class=4, local_radius=R_LOCAL, local_order=ORDER, local_hidden1_size=32, local_hidden2_size=16,
               distal_radius=R_DISTAL, emb_dropout=0.0, local_dropout=0.0, distal_fc_dropout=0.0, CNN_kernel_size=3, CNN_out_channels=32,
               optim="Adam", learning_rate=1e-3, weight_decay=1e-6, lr_scheduler="StepLR", LR_gamma=0.5, batch_size=BATCH, min_lr=1e-6,
               restart_lr=1e-4, segment_center=SEGMENT, sampled_segments=SAMPLED)
INDEL_CFG = dict(model_no=0, n_class=4, local_radius=R_LOCAL, local_order=ORDER, distal_radius=R_DISTAL, CNN_kernel_size=7,
                 CNN_out_channels=8, down_list=DOWN, use_reverse=True, optim="Adam", learning_rate=1e-3, weight_decay=1e-6,
                 lr_scheduler="StepLR", LR_gamma=0.9, batch_size=BATCH, min_lr=1e-7, restart_lr=1e-4, segment_center=SEGMENT,
                 sampled_segments=SAMPLED)


def write_files(tmp):
    """(fasta, bed, {(chrom, start): (label, strand)}): A sites on '+', T sites on '-', labels 0..3, 300 rows per chromosome."""
    rng = np.random.default_rng(977)
    fa, bed = tmp / "g.fa", tmp / "s.bed"
    table, text, lines = {}, [], []
    for name, length in (("chr1", 30011), ("chr2", 29873)):
        seq = rng.choice(np.frombuffer(b"ACGT", np.uint8), size=length)
        if name == "chr2":
            seq[12000:12090] = ord("N")
        text.append(f">{name}\n" + "\n".join(seq[i:i + 70].tobytes().decode() for i in range(0, length, 70)) + "\n")
        at = np.nonzero((seq == ord("A")) | (seq == ord("T")))[0]
        near_n = at[(at > 11990) & (at < 12100)][:6] if name == "chr2" else at[:0]       # local and distal windows over the N run
        pos = np.unique(np.r_[at[:2], at[-2:], near_n, rng.choice(at, size=300, replace=False)])[:300]
        for p in pos:
            strand, lab = "+" if seq[p] == ord("A") else "-", int(rng.integers(0, 4))
            table[name, int(p)] = (lab, strand)
            lines.append(f"{name}\t{p}\t{p + 1}\t.\t{lab}\t{strand}\n")
    fa.write_text("".join(text))
    bed.write_text("".join(lines))
    return fa, bed, table


@pytest.fixture(scope="module")
def files(tmp_path_factory):
    return write_files(tmp_path_factory.mktemp("train_run"))


def make_loader(files, batch=BATCH, **kw):
    from mural_amd.data import EpochLoader
    return EpochLoader(files[0], files[1], batch, R_LOCAL, ORDER, R_DISTAL, segment_center=SEGMENT, sampled_segments=SAMPLED, **kw)


@pytest.fixture(scope="module")
def views(files):
    loader = make_loader(files)
    train, valid = loader.split(RATIO, SPLIT_SEED)
    return loader, train, valid


def fresh_model(cfg=SNV_CFG, model_type="snv", seed=0):
    from mural_amd.train_run import prepare_model
    torch.manual_seed(seed)
    cfg = copy.deepcopy(cfg)
    return prepare_model(cfg, "cuda", model_type=model_type), cfg


class Log(list):
    def __call__(self, *args):
        self.append(" ".join(str(a) for a in args))

    def has(self, text):
        return any(text in line for line in self)


class OneBatch:
    """The first batch of a view's epoch, as an epoch of its own: every epoch of a run over it is one step."""

    def __init__(self, view):
        self.view = view

    def __len__(self):
        return BATCH

    def epoch(self, shuffle=True, generator=None):
        for batch in self.view.epoch(shuffle=shuffle, generator=generator):
            assert batch[0].shape[0] == BATCH
            yield batch
            return


# ------------------------------------------------------------------------------------------------------------------ 1. split and rows
def test_split_views_and_rows_equal_the_batches_and_the_bed(files, views):
    from mural_amd.data.batching import split_segments
    loader, train, valid = views
    n_groups = len(loader.group_sizes)
    assert len(loader) == 600 and n_groups >= 12
    tr, va = split_segments(n_groups, RATIO, SPLIT_SEED)
    assert 2 <= len(va) <= 3 and train._groups == tr and valid._groups == va
    assert len(train) + len(valid) == 600 and len(valid) == int(loader.group_sizes[va].sum())
    # both views read the parent's tables: nothing is uploaded twice
    assert train._table is loader and valid._table is loader and valid.genomes is loader.genomes and valid.row_pos is loader.row_pos
    t_sizes = [b[0].shape[0] for b in train.epoch(shuffle=True, generator=torch.Generator().manual_seed(1))]
    v_batches = list(valid.epoch(shuffle=False))
    v_sizes = [b[0].shape[0] for b in v_batches]
    print(f"[train_run] groups {loader.group_sizes.tolist()}, validation {va}; training batches {t_sizes}, validation batches {v_sizes}")
    assert len(t_sizes) == train.n_batches and sum(t_sizes) == len(train) and t_sizes[-1] != BATCH and set(t_sizes[:-1]) == {BATCH}
    assert len(v_sizes) == valid.n_batches and sum(v_sizes) == len(valid) and 1 < v_sizes[-1] < BATCH
    with pytest.raises(ValueError):
        loader.split(0.01, SPLIT_SEED)
    with pytest.raises(ValueError):
        loader.split(1.0, SPLIT_SEED)
    for view, batches in ((valid, v_batches), (loader, list(loader.epoch(shuffle=False)))):
        rows = view.rows()
        cat = torch.cat([b[2] for b in batches])
        assert rows.local.dtype == torch.int64 and rows.local.shape == cat.shape and torch.equal(rows.local, cat)
        assert rows.chrom_id.dtype == torch.int32 and rows.start.dtype == torch.int64 and rows.label.dtype == torch.int64
        assert torch.equal(rows.label, torch.cat([b[0] for b in batches]).long().squeeze(1))
        names = [view.chrom_names[c] for c in rows.chrom_id.tolist()]
        got = [(lab, "-" if s else "+") for lab, s in zip(rows.label.tolist(), rows.strand.tolist())]
        assert got == [files[2][key] for key in zip(names, rows.start.tolist())]
        assert len(set(zip(names, rows.start.tolist()))) == len(view)
    # the order-1 codes the report reads: PackedGenome.encode_kmer of the same sites
    rows = valid.rows(local_order=1)
    assert rows.local.shape == (len(valid), 2 * R_LOCAL + 1) and int(rows.local.max()) <= 4
    for slot, name in enumerate(valid.chrom_names):
        sel = (rows.chrom_id == slot).nonzero().reshape(-1)
        assert torch.equal(rows.local[sel], loader.genomes[name].encode_kmer(rows.start[sel], rows.strand[sel], R_LOCAL, 1))
    assert int((loader.rows(local_order=1).local == 4).sum()) > 0      # sites beside the N run: the padding code is in play
    # rows in an order of the caller's
    some = torch.tensor([5, 0, 599, 17])
    assert torch.equal(loader.rows(some).start, loader.row_pos[some.cuda()])


def _one_row_batch_size(n_valid):
    return next(b for b in range(BATCH - 1, 8, -1) if n_valid % b == 1)


def test_a_second_validation_bed_shares_the_uploaded_genome(files, views, tmp_path):
    loader = views[0]
    bed2 = tmp_path / "v.bed"
    bed2.write_text("".join(open(files[1]).readlines()[100:160]))
    other = make_loader((files[0], bed2), genomes=loader.genomes)
    assert len(other) == 60 and all(other.genomes[k] is loader.genomes[k] for k in other.genomes)
    only = make_loader((tmp_path / "no_such.fa", bed2), genomes=loader.genomes)      # the FASTA is not opened at all
    a, b = list(other.epoch(shuffle=False)), list(only.epoch(shuffle=False))
    assert len(a) == len(b) == 1 and torch.equal(a[0][2], b[0][2]) and torch.equal(a[0][3].sym, b[0][3].sym)
    own = make_loader((files[0], bed2))
    assert torch.equal(list(own.epoch(shuffle=False))[0][3].sym, a[0][3].sym)


# ------------------------------------------------------------------------------------------------------------------ 2. validate_epoch
def _ce_rows(out, target):
    """softmax and summed loss of one batch by the launch validate_epoch uses"""
    from mural_amd import _lib
    out = out.contiguous()
    prob, loss = torch.empty_like(out), torch.empty((), dtype=torch.float32, device=out.device)
    _lib.check(_lib.lib().mural_op_ce_sum_fwd(out.data_ptr(), target.data_ptr(), out.shape[0], out.shape[1], prob.data_ptr(), loss.data_ptr(),
                                              _lib.current_stream_ptr(out.device)))
    return prob, loss


def test_validate_epoch_equals_model_predict_m(files, views):
    from mural_amd.model.nn_utils import model_predict_m
    from mural_amd.train import CrossEntropySum
    from mural_amd.train_run import validate_epoch
    _, _, valid = views
    model, _ = fresh_model()
    crit = torch.nn.CrossEntropyLoss(reduction="sum")
    dense_valid = make_loader(files, dense=True).split(RATIO, SPLIT_SEED)[1]
    batches = list(dense_valid.epoch(shuffle=False))
    n = len(valid)
    assert sum(b[0].shape[0] for b in batches) == n
    model.train()                                                 # validate_epoch puts the model in eval mode itself
    prob_d, loss_d = validate_epoch(model, dense_valid, crit, "cuda")
    assert not model.training and prob_d.shape == (n, 4) and prob_d.dtype == torch.float32 and prob_d.is_cuda
    pred, want_loss = model_predict_m(model, batches, crit, "cuda", 4, fuse_rows=1)      # one forward per batch: the same batches
    want, off = [], 0
    for b in batches:
        k = b[0].shape[0]
        want.append(_ce_rows(pred[off:off + k], b[0].long().squeeze(1))[0])
        off += k
    want = torch.cat(want)
    ref = torch.softmax(pred, dim=1)
    print(f"[train_run] validate_epoch: rows {n}, loss {loss_d!r} vs model_predict_m {want_loss!r}; "
          f"prob max |kernel - torch.softmax| {float((want - ref).abs().max()):.3e}, bit-equal rows {int((prob_d == want).all(1).sum())}/{n}")
    assert torch.equal(prob_d, want)
    # the launch's softmax against torch's: both are a few float32 roundings from the exact value (exp, a sum of 4, a reciprocal, a
    # product: at most 8 ulp each), probabilities are at most 1
    assert float((prob_d - ref).abs().max()) <= 16 * U24
    bound = 2.0 * (n + 2.0) * U24 * abs(want_loss)                 # tests/_parity.py, _sum_check: n non-negative terms, S = their sum
    assert abs(loss_d - want_loss) <= bound, (loss_d, want_loss, bound)
    # the loader's own form (symbol windows): the same rows through forward_symbols, and either spelling of the criterion
    prob_s, loss_s = validate_epoch(model, valid, CrossEntropySum(), "cuda")
    print(f"[train_run] symbols vs dense: max |diff| {float((prob_s - prob_d).abs().max()):.3e}, loss {loss_s!r} vs {loss_d!r}")
    assert torch.equal(prob_s, prob_d) and loss_s == loss_d
    # a criterion the launch does not stand for is called as it is, beside torch.softmax
    weighted = torch.nn.CrossEntropyLoss(reduction="sum", weight=torch.tensor([1.0, 2.0, 0.5, 1.0], device="cuda"))
    prob_w, loss_w = validate_epoch(model, valid, weighted, "cuda")
    want_w = float(weighted(pred, valid.rows().label))
    assert torch.equal(prob_w, ref) and abs(loss_w - want_w) <= 2.0 * (n + 2.0) * U24 * 2.0 * abs(want_w)


def test_validation_evaluates_a_final_batch_of_one_row(files, views):
    from mural_amd.train_run import validate_epoch
    _, _, valid = views
    b = _one_row_batch_size(len(valid))
    small = make_loader(files, batch=b).split(RATIO, SPLIT_SEED)[1]
    sizes = [x[0].shape[0] for x in small.epoch(shuffle=False)]
    assert sizes[-1] == 1 and len(small) == len(valid)
    model, _ = fresh_model()
    crit = torch.nn.CrossEntropyLoss(reduction="sum")
    prob, loss = validate_epoch(model, small, crit, "cuda")
    prob64, loss64 = validate_epoch(model, valid, crit, "cuda")
    print(f"[train_run] batches of {b}: sizes {sizes}; max |prob - prob(batch 64)| {float((prob - prob64).abs().max()):.3e}")
    assert prob.shape == prob64.shape and bool(torch.isfinite(prob).all())
    assert torch.equal(prob, prob64)                               # eval outputs do not depend on the batch a row is computed in
    assert abs(loss - loss64) <= 2.0 * (len(valid) + 2.0) * U24 * abs(loss64)


# ------------------------------------------------------------------------------------------------------------------ 3./4. fit
@pytest.fixture(scope="module")
def device_run(views, tmp_path_factory):
    """fit for 2 epochs on the device loop, computed once: (model, config, initial state, history, best epoch, trial dir, log)."""
    from mural_amd.train_run import fit
    _, train, valid = views
    model, cfg = fresh_model()
    init = copy.deepcopy(model.state_dict())
    trial = tmp_path_factory.mktemp("trial_device")
    log = Log()
    history, best = fit(model, cfg, train, valid, epochs=2, trial_dir=trial, grace_period=5, device="cuda", split_generator_seed=RUN_SEED,
                        printer=log)
    return model, cfg, init, history, best, trial, log


def test_fit_writes_checkpoints_that_load_and_match(views, device_run):
    from mural_amd.calibration import dirichlet_calibrate, load_dirichlet_weights
    from mural_amd.model.nn_utils import load_model
    from mural_amd.train import CrossEntropySum, DeviceStepState, make_optimizer, train_epoch_device
    from mural_amd.train_run import metrics_text, validate_epoch
    _, train, valid = views
    model, cfg, init, history, best, trial, log = device_run
    assert len(history) == 2 and [h["epoch"] for h in history] == [0, 1] and not log.has("host loop")
    assert best == 1 - (0 if history[1]["loss"] <= history[0]["loss"] else 1)
    crit = CrossEntropySum()
    for h in history:
        e = h["epoch"]
        d = os.path.join(str(trial), f"checkpoint_{e}")
        assert sorted(os.listdir(d)) == [f"epoch_{e}_metrics.txt", "model", "model.config.pkl", "model.fdiri_cal.pkl"]
        assert h["checkpoint"] == os.path.join(d, "model")
        assert open(os.path.join(d, f"epoch_{e}_metrics.txt")).read() == metrics_text(h)
        assert h["total_params"] == sum(p.numel() for p in model.parameters()) and np.isfinite(h["loss"]) and np.isfinite(h["fdiri_loss"])
        loaded, lcfg = load_model(h["checkpoint"])
        assert lcfg == cfg
        prob, total = validate_epoch(loaded, valid, crit, "cuda")
        assert total / len(valid) == h["loss"]                     # eval forwards are bitwise repeatable: the checkpoint's own loss
        w = load_dirichlet_weights(h["checkpoint"] + ".fdiri_cal.pkl")
        assert w.shape == (4, 5) and np.array_equal(w, h["report"]["calibrator"])
        cal = dirichlet_calibrate(prob.cpu().numpy(), w)
        assert cal.shape == (len(valid), 4) and np.allclose(cal.sum(1), 1.0)
    # the last checkpoint is the model in memory, bit for bit
    mine, _ = validate_epoch(model, valid, crit, "cuda")
    assert torch.equal(prob, mine)
    assert history[0]["after_min_loss"] == 0 and set(history[0]["report"]["before"]["kmer"]) == {3, 5, 7}
    assert log.has("3mer correlation - all: ") and log.has("7mer correlation(after fdiri_cal)") and log.has("regional score: ")
    assert log.has("regional corr (validation, after fdiri_cal): 500000bp") and log.has("Validation Loss: ") and log.has("Best Epoch: ")
    assert not log.has("Poisson")
    # the training losses: a hand-written loop of train_epoch_device over the same view with the same seeds
    torch.manual_seed(0)
    twin, _ = fresh_model()
    twin.load_state_dict(init)
    opt = make_optimizer(cfg, twin.parameters(), device_state=DeviceStepState("cuda", cfg["learning_rate"]))
    for h in history:
        gen = torch.Generator().manual_seed(RUN_SEED + h["epoch"])
        total = train_epoch_device(twin, train.epoch(shuffle=True, generator=gen), crit, opt, cfg, "cuda", epoch=h["epoch"], train_size=len(train))
        print(f"[train_run] epoch {h['epoch']}: training loss per row fit {h['train_loss']!r}, hand loop {total / len(train)!r}")
        assert abs(total / len(train) - h["train_loss"]) <= 1e-3 * abs(h["train_loss"])
    assert list(twin._device_epoch_steps) == [BATCH] == list(model._device_epoch_steps)


def test_host_loop_gives_the_device_loops_validation_losses(views, device_run, tmp_path):
    from mural_amd.train_run import fit
    _, train, valid = views
    _, cfg, init, history, _, _, _ = device_run
    model, cfg2 = fresh_model()
    model.load_state_dict(init)
    assert cfg2 == cfg
    log = Log()
    host, _ = fit(model, cfg2, train, valid, epochs=2, trial_dir=tmp_path, grace_period=5, device="cuda", device_loop=False,
                  split_generator_seed=RUN_SEED, printer=log)
    assert sum("host loop" in line for line in log) == 1           # announced, once
    assert not hasattr(model, "_device_epoch_steps")
    for a, b in zip(host, history):
        print(f"[train_run] epoch {a['epoch']}: validation loss host loop {a['loss']!r}, device loop {b['loss']!r}; training {a['train_loss']!r} / {b['train_loss']!r}")
        assert abs(a["loss"] - b["loss"]) <= 1e-3 * abs(b["loss"])
        assert abs(a["train_loss"] - b["train_loss"]) <= 1e-3 * abs(b["train_loss"])
        assert a["lr"] == b["lr"]
    assert os.path.exists(os.path.join(str(tmp_path), "checkpoint_1", "model.fdiri_cal.pkl"))


# ------------------------------------------------------------------------------------------------------------------ 5./6. between epochs
def _stub(per_row_loss_of_epoch, batches_per_validation):
    """The loop's criterion in training; under no_grad (validation) the loss of the epoch's entry, per row."""
    from mural_amd.train import CrossEntropySum

    class Stub(CrossEntropySum):
        calls = 0

        def forward(self, x, y):
            if torch.is_grad_enabled():
                return super().forward(x, y)
            epoch = self.calls // batches_per_validation
            self.calls += 1
            return x.new_full((), per_row_loss_of_epoch(epoch) * x.shape[0])

    return Stub()


def test_reduce_on_plateau_rate_reaches_the_next_epochs_first_update(views, tmp_path):
    """A constant validation loss: ReduceLROnPlateau (patience 1, factor 0.2) cuts the rate after the third epoch.  Every epoch here
    is ONE step, so what the block shows after epoch 3 is what it shows after that epoch's first update."""
    from mural_amd.train import DeviceStepState, make_optimizer
    from mural_amd.train_run import fit
    _, train, valid = views
    model, cfg = fresh_model()
    cfg["lr_scheduler"] = "ROP"
    opt = make_optimizer(cfg, model.parameters(), device_state=DeviceStepState("cuda", cfg["learning_rate"]))
    log = Log()
    history, best = fit(model, cfg, OneBatch(train), valid, epochs=4, trial_dir=tmp_path, grace_period=2, device="cuda",
                        split_generator_seed=RUN_SEED, printer=log, criterion=_stub(lambda e: 2.0, valid.n_batches), optimizer=opt)
    assert not log.has("host loop") and len(history) == 4 and best == 3
    assert [h["loss"] for h in history] == [2.0] * 4 and [h["after_min_loss"] for h in history] == [0, 1, 2, 3]
    reduced = 1e-3 * 0.2
    assert [h["lr"] for h in history] == [1e-3, 1e-3, 1e-3, reduced]
    r = opt.device_state.read()
    print(f"[train_run] ROP: block after epoch 3's only step {r}")
    assert r["lr"] == reduced == opt.param_groups[0]["lr"] and r["step"] == 4 and r["steps_done"] == 1 and r["rows"] == BATCH
    want = np.float32(reduced / (1.0 - 0.9 ** 4))                  # the step size the tick formed for update 4: from the reduced rate
    assert abs(np.float32(r["step_size"]) - want) <= np.spacing(want)
    assert abs(np.float32(r["step_size"]) - np.float32(1e-3 / (1.0 - 0.9 ** 4))) > 1e3 * np.spacing(want)


def test_early_stopping_ends_the_run_and_names_the_best_epoch(views, tmp_path):
    from mural_amd.train_run import fit
    _, train, valid = views
    model, cfg = fresh_model()
    losses = [3.0, 2.0, 2.5, 2.25, 1.0, 0.5]                       # best at epoch 1; epochs 2 and 3 trip patience 2
    log = Log()
    history, best = fit(model, cfg, OneBatch(train), valid, epochs=6, trial_dir=tmp_path, grace_period=2, device="cuda",
                        split_generator_seed=RUN_SEED, printer=log, criterion=_stub(lambda e: losses[e], valid.n_batches))
    assert [h["loss"] for h in history] == losses[:4] and best == 1
    assert [h["after_min_loss"] for h in history] == [0, 0, 1, 2]
    assert log.has("Early stopping") and log.has("EarlyStopping counter: 2 out of 2") and log[-1] == "Best Epoch: 1"
    assert sorted(os.listdir(tmp_path)) == [f"checkpoint_{e}" for e in range(4)]
    assert open(os.path.join(str(tmp_path), "checkpoint_3", "epoch_3_metrics.txt")).read().startswith("loss: 2.25\n")


# ------------------------------------------------------------------------------------------------------------------ 7. INDEL
def test_indel_run_on_symbol_windows(files, tmp_path):
    from mural_amd.model.nn_utils import load_model
    from mural_amd.train_run import fit
    loader = make_loader(files, model_type="indel", symbols=True)
    train, valid = loader.split(RATIO, SPLIT_SEED)
    model, cfg = fresh_model(INDEL_CFG, "indel")
    log = Log()
    history, best = fit(model, cfg, train, valid, epochs=1, trial_dir=tmp_path, grace_period=5, device="cuda", model_type="indel",
                        split_generator_seed=RUN_SEED, printer=log)
    assert len(history) == 1 and best == 0 and not log.has("host loop")
    assert list(model._device_epoch_steps) == [BATCH] and model._device_epoch_steps[BATCH][0].x.dtype is torch.uint8
    rep = history[0]["report"]
    assert set(rep["before"]["kmer"]) == set(rep["fdiri"]["kmer"]) == set(rep["poisson"]["kmer"]) == {2, 4, 6}
    assert log.has("2mer correlation - all: ") and log.has("6mer correlation(after Poisson_cal)")
    assert log.has("regional score(after Poisson_cal)") and log.has("regional corr (validation, after Poisson_cal): 100000bp")
    assert np.isfinite(history[0]["loss"]) and np.isfinite(history[0]["train_loss"]) and history[0]["loss"] > 0
    loaded, _ = load_model(history[0]["checkpoint"], model_type="indel")
    assert type(loaded).__name__ == "UNet_Small"


# ------------------------------------------------------------------------------------------------------------------ 8. transfer
def test_transfer_reinitialises_exactly_the_last_head_layers(tmp_path):
    from mural_amd.model.nn_utils import save_model
    from mural_amd.train_run import prepare_model
    model, cfg = fresh_model(seed=3)
    with torch.no_grad():
        for p in model.parameters():                               # a "pretrained" state in which no tensor holds its initial value
            p.add_(0.01 * torch.randn_like(p))
    path = str(tmp_path / "model")
    save_model(model, None, cfg, path)
    state = {k: v.detach().cpu().clone() for k, v in model.state_dict().items()}
    heads = {"local_fc.0.weight", "local_fc.0.bias", "distal_fc1.2.weight", "distal_fc1.2.bias", "distal_fc2.2.weight", "distal_fc2.2.bias"}
    assert heads <= set(state)
    torch.manual_seed(8)
    kept = prepare_model(copy.deepcopy(cfg), "cuda", model_path=path)
    assert all(p.requires_grad for p in kept.parameters())
    assert all(torch.equal(v.cpu(), state[k]) for k, v in kept.state_dict().items())
    torch.manual_seed(8)
    fresh = prepare_model(copy.deepcopy(cfg), "cuda", model_path=path, init_fc_with_pretrained=False)
    changed = {k for k, v in fresh.state_dict().items() if not torch.equal(v.cpu(), state[k])}
    assert changed == heads
    assert all(p.requires_grad for p in fresh.parameters()) and next(fresh.parameters()).is_cuda
    assert not fresh.state_dict()["distal_fc1.2.bias"].any() and not fresh.state_dict()["local_fc.0.bias"].any()
    with pytest.raises(ValueError, match="INDEL"):
        prepare_model(copy.deepcopy(INDEL_CFG), "cuda", model_path=path, init_fc_with_pretrained=False, model_type="indel")
