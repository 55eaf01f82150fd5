"""``mural_amd.data.EpochLoader`` (one ``mural_train_batch_encode`` launch per batch) against ``train_batches_from_files`` on a fixture
that takes every branch of the kernel: both strands, windows that reach beyond both ends of a record, an N run, IUPAC codes, groups of
segments that cross a chromosome boundary, carried tails, the SNV and the INDEL window widths."""
import numpy as np
import pytest
import torch

from tests import _loader_data as D

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def files(tmp_path_factory):
    return D.write_fixture(tmp_path_factory.mktemp("epoch_loader"))


@pytest.fixture(scope="module")
def old_batches(files):
    """The old route's batches, computed once per (model_type, shuffle) and left unchanged."""
    cache = {}

    def get(model_type, shuffle):
        if (model_type, shuffle) not in cache:
            cache[model_type, shuffle] = D.old_route(*files, model_type, shuffle, seed=5)
        return cache[model_type, shuffle]
    return get


def _rows_of_epoch(loader, shuffle, seed):
    from mural_amd.data.batching import epoch_order
    g = torch.Generator().manual_seed(seed) if shuffle else None
    return epoch_order(loader.group_sizes, D.SAMPLED, D.BATCH, shuffle=shuffle, generator=g)[0]


def _encode_symbols_of_rows(loader, rows, model_type):
    """``PackedGenome.encode_symbols`` of the rows, chromosome by chromosome (the existing single-genome encoder)."""
    rows = rows.cuda()
    chrom, pos, strand = loader.row_chrom[rows], loader.row_pos[rows], loader.row_strand[rows]
    out = torch.full((rows.shape[0], loader.width), 255, dtype=torch.uint8, device="cuda")
    for slot, name in enumerate(loader.chrom_names):
        sel = (chrom == slot).nonzero().reshape(-1)
        out[sel] = loader.genomes[name].encode_symbols(pos[sel], strand[sel], D.R_DISTAL, model_type).sym
    return out


@pytest.mark.parametrize("shuffle", [False, True])
@pytest.mark.parametrize("model_type", ["snv", "indel"])
def test_batches_equal_the_old_route(files, old_batches, model_type, shuffle):
    old = old_batches(model_type, shuffle)
    loader = D.make_loader(*files, model_type=model_type)
    assert len(loader) == sum(b[0].shape[0] for b in old) == 64 and loader.n_batches == len(old)
    # the INDEL training path takes the dense tensor only: its loader is dense whatever `dense` says
    new = D.new_route(loader, shuffle, seed=5)
    D.assert_batches_equal(new, old, dense=model_type == "indel")
    assert [b[0].shape[0] for b in new] == [7] * 9 + [1]      # a final batch of one row, carried tails in front of it
    if model_type == "snv":
        rows = _rows_of_epoch(loader, shuffle, seed=5)
        want = _encode_symbols_of_rows(loader, rows, model_type)
        assert torch.equal(torch.cat([b[3].sym for b in new]), want)
        codes = set(want.unique().tolist())
        assert {0, 1, 2, 3, 4, 5, 6} <= codes and codes & {11, 14} and max(codes) <= 14      # N, R, Y and B (or its complement V) were in play
        dense = D.new_route(D.make_loader(*files, model_type=model_type, dense=True), shuffle, seed=5)
        D.assert_batches_equal(dense, old, dense=True)


def test_epochs_repeat_and_reshuffle(files):
    loader = D.make_loader(*files)
    first = D.new_route(loader, True, seed=11)
    kept = [tuple(t.clone() if torch.is_tensor(t) else t.sym.clone() for t in b) for b in first]
    again = D.new_route(loader, True, seed=11)
    other = D.new_route(loader, True, seed=12)
    key = lambda bs: [tuple(r) for b in bs for r in torch.cat([b[2].cpu(), b[3].sym.cpu().long(), b[0].cpu().long()], 1).tolist()]  # noqa: E731
    assert key(first) == key(again) and key(first) != key(other) and sorted(key(first)) == sorted(key(other))
    # a caller that holds earlier batches is not overwritten by later ones (every batch owns its tensors)
    for b, k in zip(first, kept):
        assert torch.equal(b[0], k[0]) and torch.equal(b[2], k[2]) and torch.equal(b[3].sym, k[3])


def test_direct_entry_refuses_rows_outside_the_tables(files):
    """An order entry of -1 or n_rows, or a row whose chromosome number is outside the genome array, is an argument error: the status
    word gets MURAL_E_INVALID, those batch rows come out as N windows with label 0, every other row is what a clean call gives."""
    from mural_amd import _lib
    loader = D.make_loader(*files)
    n = len(loader)
    clean = torch.arange(n, dtype=torch.int64, device="cuda")
    y0, cat0, sym0 = loader.encode(clean, 0, n)
    assert int(loader._status.item()) == 0
    bad_at = [0, 5, 33, n - 1]
    order = clean.clone()
    order[bad_at] = torch.tensor([-1, n, 2 ** 40, -(2 ** 62)], device="cuda")
    y, cat, sym = loader.encode(order, 0, n)
    assert int(loader._status.item()) == _lib.MURAL_E_INVALID
    loader._status.zero_()
    good = torch.ones(n, dtype=torch.bool, device="cuda")
    good[bad_at] = False
    assert torch.equal(y[good], y0[good]) and torch.equal(cat[good], cat0[good]) and torch.equal(sym[good], sym0[good])
    assert (sym[~good] == 4).all() and (y[~good] == 0).all() and (cat[~good] == 4 ** D.ORDER).all()
    # a chromosome number outside the genome array: every chrB row (chromosome 1 of 2) when the call is told there is one genome
    n_genomes, loader.n_genomes = loader.n_genomes, 1
    y, cat, sym = loader.encode(clean, 0, n)
    loader.n_genomes = n_genomes
    assert int(loader._status.item()) == _lib.MURAL_E_INVALID
    loader._status.zero_()
    on_a = loader.row_chrom == 0
    assert 0 < int(on_a.sum()) < n
    assert torch.equal(sym[on_a], sym0[on_a]) and torch.equal(cat[on_a], cat0[on_a]) and torch.equal(y[on_a], y0[on_a])
    assert (sym[~on_a] == 4).all() and (y[~on_a] == 0).all() and (cat[~on_a] == 4 ** D.ORDER).all()
    # a batch that reaches outside the order fails on the host
    for first, rows in ((n - 3, 4), (-1, 2), (n + 1, 0)):
        with pytest.raises(ValueError):
            loader.encode(clean, first, rows)
    # a part of the order, at an odd first row: the rows of the clean call
    y, cat, sym = loader.encode(clean, 13, 9)
    assert torch.equal(sym, sym0[13:22]) and torch.equal(cat, cat0[13:22]) and torch.equal(y, y0[13:22])


def test_missing_chromosome_and_bad_labels(files, tmp_path):
    fa, bed = files
    extra = tmp_path / "x.bed"
    extra.write_text(open(bed).read() + "chrZ\t5\t6\t.\t1\t+\n")
    with pytest.raises(KeyError, match="chrZ"):
        D.make_loader(fa, extra)
    frac = tmp_path / "f.bed"
    frac.write_text("chrA\t500\t501\t.\t0.5\t+\n")
    with pytest.raises(ValueError):
        D.make_loader(fa, frac)
    empty = tmp_path / "e.bed"
    empty.write_text("")
    loader = D.make_loader(fa, empty)
    assert len(loader) == 0 and loader.n_batches == 0 and list(loader.epoch()) == []


# Summed loss of one unshuffled train_epoch at this shape on an MI355X, the OLD route's batches, 8 runs from equal weights (the training
# step accumulates with floating-point atomics: it is not bit-reproducible run to run, so exact equality cannot be asked of any feed):
#   96.35772800 96.35772705 96.35772705 96.35773277 96.35772705 96.35772705 96.35773659 96.35772419
# sample standard deviation 3.97e-06; the loader's batches, 8 runs: 96.35772991 96.35773945 96.35773468 96.35772324 96.35772800 96.35773659 96.35772800 96.35772705 (sigma 5.5e-06).
# Two runs on bit-identical inputs differ by noise of standard deviation sqrt(2) * sigma; the bound is 5 of those.  A feed that differs in
# a single row moves the loss by orders of magnitude more (one row's loss is about 1.4).
OLD_ROUTE_SIGMA = 3.97e-06
LOSS_BOUND = 5 * 2 ** 0.5 * OLD_ROUTE_SIGMA


def train_loss(batches):
    """Summed loss of one ``train_epoch`` of a small Network2 (32 channels, kernel 3, every dropout 0) from fixed initial weights."""
    from mural_amd import train as TR
    from mural_amd.model import model_choice, weights_init
    ncol = 2 * D.R_LOCAL + 1 - (D.ORDER - 1)
    config = dict(local_radius=D.R_LOCAL, local_order=D.ORDER, local_hidden1_size=32, local_hidden2_size=16, distal_radius=D.R_DISTAL,
                  emb_dropout=0.0, local_dropout=0.0, CNN_kernel_size=3, CNN_out_channels=32, distal_fc_dropout=0.0, n_class=4, model_no=2,
                  emb_dims=[(4 ** D.ORDER + 1, 2)] * ncol, optim="Adam", learning_rate=2e-3, weight_decay=1e-6, lr_scheduler="StepLR",
                  LR_gamma=0.9, batch_size=D.BATCH, min_lr=1e-6, restart_lr=1e-4)
    common = dict(emb_dims=config["emb_dims"], n_cont=0, n_class=4, distal_order=1, in_channels=4)
    torch.manual_seed(0)
    m = model_choice(2, config, common, "snv")
    m.apply(weights_init)
    m = m.cuda()
    torch.manual_seed(1)
    opt = TR.make_optimizer(config, m.parameters())
    return TR.train_epoch(m, batches, torch.nn.CrossEntropyLoss(reduction="sum"), opt, TR.make_scheduler(config, opt), config, "cuda")


def test_train_epoch_consumes_the_batches(files, old_batches):
    """One ``train_epoch`` over the loader's batches and one over the old route's, unshuffled, from equal weights: the same summed loss.
    The inputs are bit-identical once the old route's dense tensor has gone through dense_to_symbols, but the old route's own loss is
    not bit-reproducible run to run at this shape; the bound is its measured spread (LOSS_BOUND above, with the figures)."""
    old = train_loss(old_batches("snv", False))
    new = train_loss(D.new_route(D.make_loader(*files), False, seed=0))
    print(f"train_epoch summed loss: old route {old!r}, loader {new!r}, difference {abs(new - old)!r}, bound {LOSS_BOUND!r}")
    assert np.isfinite(new) and new > 0
    assert abs(new - old) <= LOSS_BOUND
