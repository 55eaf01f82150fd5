"""Training batches gathered and encoded on the device, one launch per batch (``mural_train_batch_encode``, csrc/train_batch.hip).

``train_batches_from_files`` encodes every bed_reader segment as a dense one-hot tensor, concatenates `sampled_segments` of them and
shuffles the group with an index-select over those dense rows.  ``EpochLoader`` keeps the row table (chromosome, start, strand, label)
and the packed chromosomes on the device, takes an epoch's order as pure index logic (``batching.epoch_order``: the same rows, the same
draws from the generator) and encodes each batch from its row numbers: k-mer ids, one symbol byte per window column, labels.  The files
are read once for any number of epochs.

``EpochLoader.split`` cuts the segments into a training and a validation view (``EpochView``) over the same device tables, and ``rows``
hands out what a validation report reads beside the probabilities: chromosome, start, label and local codes of the rows in validation
order.
"""
from collections import namedtuple

import numpy as np
import torch

from .. import _lib
from .batching import epoch_order, split_segments
from .genome import SymbolWindows
from .ingest import bed_order, read_bed, read_fasta


ViewRows = namedtuple("ViewRows", "chrom_id start label local strand")
ViewRows.__doc__ = """``rows()`` of a loader or a view, device tensors in the order asked for: ``chrom_id`` int32 (indexes ``chrom_names``), ``start``
int64, ``label`` int64, ``local`` int64 (N, columns) local codes, ``strand`` uint8 (0 '+', 1 '-')."""


class _Batches:
    """What ``EpochLoader`` and ``EpochView`` share: an epoch over ``_groups`` (None: every segment) of the row table of ``_table``."""

    def __len__(self):
        return self.n_rows

    def _order(self, shuffle, generator=None):
        t = self._table
        return epoch_order(t.group_sizes, t.sampled_segments, t.batch_size, shuffle=shuffle, generator=generator, groups=self._groups)

    @property
    def n_batches(self):
        """Batches per epoch (the same for every shuffle: the carry rule depends on the group sizes alone)."""
        return int(self._order(False)[1].shape[0]) - 1

    def epoch(self, shuffle=True, generator=None):
        """The batches of one epoch (a generator): the rows and the generator draws of ``train_batches_from_files`` with the same
        `shuffle` / `generator`.  The order is uploaded once; nothing is read back until the epoch's last batch has been yielded."""
        t = self._table
        order, bounds = self._order(shuffle, generator)
        order_dev = order.to(t.device)
        bounds = bounds.tolist()
        for lo, hi in zip(bounds[:-1], bounds[1:]):
            y, cat, distal = t.encode(order_dev, lo, hi - lo)
            cont = torch.zeros((hi - lo, 1), dtype=torch.float64, device=t.device)
            yield y, cont, cat, (distal if t.dense else SymbolWindows(distal))
        t._raise_status(bounds[-1])

    def rows(self, order=None, local_order=None):
        """``ViewRows`` of the rows in validation order -- the order ``epoch(shuffle=False)`` yields them in -- or in `order` (int64 row
        numbers of the table): what a validation report reads beside the probabilities.  ``local`` holds the values of the batches'
        ``cat_x`` for the same rows; ``local_order=1`` gives the order-1 codes instead (us_r .. us_1, [mid,] ds_1 .. ds_r, values
        0 .. 4: the columns ``mural_amd.evaluation`` reads its k-mers from).  Encoded in launches of at most 65536 rows over windows
        of the local radius; nothing but the status word is read back."""
        t = self._table
        if order is None:
            order = self._order(False)[0]
        order = torch.as_tensor(order, dtype=torch.int64).to(t.device).contiguous()
        n = int(order.shape[0])
        k = t.local_order if local_order is None else int(local_order)
        cols = 2 * t.local_radius + (0 if t.indel else 1) - (k - 1)
        local = torch.empty((n, cols), dtype=torch.int64, device=t.device)
        small = 2 * t.local_radius + (0 if t.indel else 1)       # the symbol window the launch must write: as narrow as the local one
        with torch.cuda.device(t.device):
            for lo in range(0, n, 65536):
                m = min(65536, n - lo)
                y = torch.empty(m, dtype=torch.float32, device=t.device)
                sym = torch.empty((m, small), dtype=torch.uint8, device=t.device)
                _lib.check(_lib.lib().mural_train_batch_encode(
                    t._genome_structs.data_ptr(), t.n_genomes, t.row_chrom.data_ptr(), t.row_pos.data_ptr(), t.row_strand.data_ptr(),
                    t.row_label.data_ptr(), t.n_rows, order.data_ptr(), n, lo, m, t.local_radius, k, t.local_radius, int(t.indel),
                    local[lo:lo + m].data_ptr(), sym.data_ptr(), None, y.data_ptr(), t._status.data_ptr(), _lib.current_stream_ptr(t.device)))
        t._raise_status(n)
        return ViewRows(t.row_chrom[order], t.row_pos[order], t.row_label[order].to(torch.int64), local, t.row_strand[order])


class EpochView(_Batches):
    """The segments `groups` of an ``EpochLoader`` (``EpochLoader.split``): the same batches interface -- ``len``, ``n_batches``,
    ``group_sizes``, ``epoch``, ``rows`` -- over the parent's device tables; row numbers index the parent's table."""

    def __init__(self, table, groups):
        self._table, self._groups = table, [int(g) for g in groups]
        self.group_sizes = table.group_sizes[self._groups]
        self.n_rows = int(self.group_sizes.sum())

    def __getattr__(self, name):          # batch_size, device, chrom_names, cols, width, dense, ...: the parent's
        if name.startswith("_"):
            raise AttributeError(name)
        return getattr(self._table, name)


class EpochLoader(_Batches):
    """Batches ``(y (B, 1) float32, cont_x (B, 1) float64 zeros, cat_x (B, cols) int64, distal_x)`` of a FASTA + BED pair in the order
    and with the values of ``train_batches_from_files``, for ``train_epoch``.

    ``distal_x`` is ``SymbolWindows`` over the uint8 (B, W) symbol tensor for SNV models -- the form their training forward takes in
    place of the dense tensor, bit-identical to converting it.  With ``dense=True``, and by default for ``model_type="indel"``, it is
    the float32 (B, 4, W) one-hot tensor of the batch's rows, written by the same launch.  ``symbols=True`` asks for ``SymbolWindows``
    from an INDEL loader too (``UNet_Small`` trains from them through model/indel_train_step.py: 1 byte per column instead of 16).
    Every batch owns freshly allocated tensors: a caller may keep any number of them.

    ``genomes``: a dict {chromosome name: ``PackedGenome`` on `device`} of chromosomes that are already uploaded (another loader's
    ``.genomes``: a separate validation BED on the training FASTA); only chromosomes the BED names and the dict lacks are read from the
    FASTA."""

    _groups = None           # (an EpochView names its segments here; the loader itself runs over all of them)

    def __init__(self, fasta_path, bed_path, batch_size, local_radius, local_order=3, distal_radius=None, segment_center=300000,
                 sampled_segments=10, model_type="snv", device="cuda", dense=False, symbols=False, genomes=None):
        if model_type not in ("snv", "indel"):
            raise ValueError(f"model_type {model_type} not supported!")
        if distal_radius is None:
            raise ValueError("EpochLoader: distal_radius is required")
        if int(batch_size) < 1 or int(sampled_segments) < 1:
            raise ValueError("batch_size and sampled_segments must be >= 1")
        self.batch_size, self.sampled_segments = int(batch_size), int(sampled_segments)
        self.local_radius, self.local_order, self.distal_radius = int(local_radius), int(local_order), int(distal_radius)
        self.indel = model_type == "indel"
        if dense and symbols:
            raise ValueError("EpochLoader: dense=True and symbols=True exclude each other")
        self.dense = bool(dense) or (self.indel and not symbols)
        self.device = torch.device(device)
        odd = 0 if self.indel else 1
        self.cols, self.width = 2 * self.local_radius + odd - (self.local_order - 1), 2 * self.distal_radius + odd
        sites = read_bed(bed_path)
        order, group = bed_order(sites, segment_center)
        used_ids = np.unique(sites.chrom_id)
        used = {sites.chrom_names[c] for c in used_ids}
        if genomes is None:
            self.genomes = read_fasta(fasta_path, self.device, names=used)
        else:
            self.genomes = {k: g for k, g in genomes.items() if k in used}
            here = torch.empty(0, device=self.device).device      # ("cuda" resolved to the current device's index)
            if any(g.packed2.device != here for g in self.genomes.values()):
                raise ValueError(f"EpochLoader: the genomes handed over do not live on {self.device}")
            if used - set(self.genomes):
                self.genomes.update(read_fasta(fasta_path, self.device, names=used - set(self.genomes)))
        missing = used - set(self.genomes)
        if missing:
            raise KeyError(sorted(missing)[0])
        label = sites.score[order]
        if len(label) and not (np.isfinite(label).all() and (label >= 0).all() and (label <= 255).all() and (label == np.floor(label)).all()):
            raise ValueError("EpochLoader: the BED scores (class labels) must be integers in 0 .. 255")
        # rows in bed_reader order; the chromosomes in use numbered 0 .. in the order of the BED's name table
        slot = np.full(max(len(sites.chrom_names), 1), -1, np.int32)
        slot[used_ids] = np.arange(len(used_ids), dtype=np.int32)
        self.n_rows = len(order)
        up = lambda a, dt: torch.from_numpy(np.ascontiguousarray(a, dt)).to(self.device)      # noqa: E731
        self.row_chrom, self.row_pos = up(slot[sites.chrom_id[order]], np.int32), up(sites.start[order], np.int64)
        self.row_strand, self.row_label = up(sites.strand[order], np.uint8), up(label, np.uint8)
        structs = (_lib.MuralGenome * max(len(used_ids), 1))()
        for i, c in enumerate(used_ids):
            structs[i] = self.genomes[sites.chrom_names[c]].as_struct()
        self.n_genomes = len(used_ids)
        self.chrom_names = [sites.chrom_names[c] for c in used_ids]      # row_chrom indexes this list
        self._genome_structs = torch.frombuffer(bytearray(bytes(structs)), dtype=torch.uint8).to(self.device)
        edges = np.r_[0, np.nonzero(group[1:] != group[:-1])[0] + 1, len(group)] if len(group) else np.zeros(1, np.int64)
        self.group_sizes = np.diff(edges).astype(np.int64)
        self._status = torch.zeros(1, dtype=torch.int32, device=self.device)

    @property
    def _table(self):
        return self

    def encode(self, order, first, n):
        """(y, cat_x, distal tensor) of the rows ``order[first : first + n]`` (`order`: int64 device tensor of row numbers): one launch."""
        dev = self.device
        y = torch.empty((n, 1), dtype=torch.float32, device=dev)
        cat = torch.empty((n, self.cols), dtype=torch.int64, device=dev)
        if self.dense:
            distal = torch.empty((n, 4, self.width), dtype=torch.float32, device=dev)
            sym_ptr, dense_ptr = None, distal.data_ptr()
        else:
            distal = torch.empty((n, self.width), dtype=torch.uint8, device=dev)
            sym_ptr, dense_ptr = distal.data_ptr(), None
        with torch.cuda.device(dev):
            _lib.check(_lib.lib().mural_train_batch_encode(
                self._genome_structs.data_ptr(), self.n_genomes, self.row_chrom.data_ptr(), self.row_pos.data_ptr(),
                self.row_strand.data_ptr(), self.row_label.data_ptr(), self.n_rows, order.data_ptr(), order.shape[0], int(first), int(n),
                self.local_radius, self.local_order, self.distal_radius, int(self.indel), cat.data_ptr(), sym_ptr, dense_ptr,
                y.data_ptr(), self._status.data_ptr(), _lib.current_stream_ptr(dev)))
        return y, cat, distal

    def _raise_status(self, rows):
        if rows and int(self._status.item()) != 0:      # (cannot happen with an order of epoch_order: a corrupted row table)
            self._status.zero_()
            raise RuntimeError("EpochLoader: a batch named a row or a chromosome outside the tables")

    def split(self, valid_ratio, split_seed):
        """(training view, validation view): the segments (the groups of ``group_sizes``) divided by ``batching.split_segments`` --
        ``int(n_segments * valid_ratio)`` of them to validation, assigned by ``random_split`` under ``manual_seed(split_seed)``, the
        validation segments ascending, the training segments in the split's order.  Both views read this loader's tables; a ratio that
        leaves either side without a segment raises ValueError."""
        train, valid = split_segments(len(self.group_sizes), valid_ratio, split_seed)
        return EpochView(self, train), EpochView(self, valid)
