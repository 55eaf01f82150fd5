"""Host-side row ordering and batching with the reference's contracts (pure index logic, no tensors moved).

  * ``segment_order``          -- row order produced by bed_reader (MuRaL/data/preprocessing.py:39-106): sites are cut
                                  into `central_bp`-wide segments along each chromosome and every segment yields its '+'
                                  rows, then its '-' rows.  Predictions come out in this order
                                  (run_predict.py:234) before the final sort by (chrom, start).
  * ``generate_data_batches``  -- two-level batching of MuRaL/data/preprocessing.py:1148-1226: `batch_segment` segments
                                  are concatenated, cut into `batch_size` batches, a short tail batch is PREPENDED to the
                                  next group, and the final short batch is emitted.  Works on any sequence of 4-tuples
                                  of tensors shaped like the reference's DataLoader output (leading dim 1).
  * ``epoch_order``            -- the rows ``generate_data_batches`` yields, as row numbers: the order of a whole epoch and its
                                  batch boundaries from the group sizes alone (what a device-side loader gathers by).
  * ``split_segments``         -- the training / validation split by segment of MuRaL/training.py:220-227; ``segment_rows`` lists
                                  the rows of a set of segments.  ``epoch_order(groups=)`` runs an epoch over such a set.
"""
import numpy as np
import torch


def segment_order(chrom, start, strand, central_bp):
    """Return (order, group): `order` permutes the input rows (sorted by chrom/start, as a BED file is) into
    bed_reader order; `group` numbers the (segment, strand) groups the reference yields."""
    chrom = np.asarray(chrom)
    start = np.asarray(start, dtype=np.int64)
    strand = np.asarray(strand).astype(bool)
    order, group = [], []
    g = 0
    pos_rows, neg_rows = [], []

    def flush():
        nonlocal g, pos_rows, neg_rows
        if pos_rows:
            order.extend(pos_rows)
            group.extend([g] * len(pos_rows))
            g += 1
            pos_rows = []
        if neg_rows:
            order.extend(neg_rows)
            group.extend([g] * len(neg_rows))
            g += 1
            neg_rows = []

    cur_chrom, end0 = None, 0
    for i in range(len(start)):
        if cur_chrom is None:
            cur_chrom = chrom[i]
            end0 = int(start[i]) + central_bp          # the first segment starts at the first site (:62-64)
        if chrom[i] != cur_chrom:
            flush()
            cur_chrom = chrom[i]
            end0 = 1 + central_bp                      # later chromosomes start their grid at 1 (:77-78)
        if start[i] > end0:
            flush()
            while start[i] > end0:
                end0 += central_bp
        (neg_rows if strand[i] else pos_rows).append(i)
    flush()
    return np.asarray(order, dtype=np.int64), np.asarray(group, dtype=np.int64)


def _concat_segments(segs):
    y = torch.cat([s[0].squeeze(0) for s in segs])
    cat = torch.cat([s[2].squeeze(0) for s in segs])
    dist = torch.cat([s[3].squeeze(0) for s in segs])
    return y, cat, dist


def generate_data_batches(segment_loader, batch_segment, batch_size, shuffle=True, generator=None):
    """Yield (y, cont_x, cat_x, distal_x) batches; cont_x is float64 zeros (n, 1) like the reference (:1209)."""
    carry = None
    group = []

    def batches_of(y, cat, dist, last):
        nonlocal carry
        n = y.shape[0]
        idx = torch.randperm(n, generator=generator) if shuffle else torch.arange(n)
        for o in range(0, n, batch_size):
            sel = idx[o:o + batch_size]
            if sel.shape[0] < batch_size and not last:
                carry = (y[sel], cat[sel], dist[sel])
                return
            yield y[sel], torch.zeros((sel.shape[0], 1), dtype=torch.float64), cat[sel], dist[sel]

    it = iter(segment_loader)
    pending = next(it, None)
    while pending is not None:
        group.append(pending)
        pending = next(it, None)
        if len(group) >= batch_segment or pending is None:
            y, cat, dist = _concat_segments(group)
            group = []
            if carry is not None:                       # the short tail of the previous group goes FIRST (:1219-1225)
                y, cat, dist = torch.cat([carry[0], y]), torch.cat([carry[1], cat]), torch.cat([carry[2], dist])
                carry = None
            yield from batches_of(y, cat, dist, last=pending is None)


def split_segments(n_segments, valid_ratio, split_seed):
    """(training segments, validation segments) of a run without a validation file (MuRaL/training.py:220-227):
    ``n_valid = int(n_segments * valid_ratio)`` segments go to validation, assigned by ``torch.utils.data.random_split`` over the segment
    numbers with ``torch.Generator().manual_seed(split_seed)``; the validation segments are sorted ascending, the training segments stay in
    the order the split gave them.  A ratio that leaves either side empty raises ValueError."""
    n_segments = int(n_segments)
    n_valid = int(n_segments * valid_ratio)
    if n_valid < 1 or n_valid >= n_segments:
        raise ValueError(f"valid_ratio {valid_ratio} of {n_segments} segments leaves {n_valid} for validation and {n_segments - n_valid} "
                         "for training: both sides need at least one segment")
    train, valid = torch.utils.data.random_split(range(n_segments), [n_segments - n_valid, n_valid],
                                                 torch.Generator().manual_seed(int(split_seed)))
    return [int(i) for i in train.indices], sorted(int(i) for i in valid.indices)


def segment_rows(group_sizes, groups):
    """Row numbers (int64 numpy, rows of the whole table) of the segments `groups`, segment after segment in the order given."""
    starts = np.concatenate([[0], np.cumsum([int(v) for v in group_sizes], dtype=np.int64)]).astype(np.int64)
    parts = [np.arange(starts[g], starts[g + 1], dtype=np.int64) for g in groups]
    return np.concatenate(parts) if parts else np.zeros(0, np.int64)


def epoch_order(group_sizes, batch_segment, batch_size, shuffle=True, generator=None, groups=None):
    """(order, batch_bounds) of one epoch of ``generate_data_batches`` over segments of `group_sizes` rows each (the (segment, strand)
    groups of ``bed_order``, in order), with row i = the i-th row in bed_reader order: `order` (int64, a permutation of 0..n-1) lists
    the rows as the batches yield them, batch k is ``order[batch_bounds[k]:batch_bounds[k + 1]]`` (int64, len = batches + 1).  Same
    draws from `generator` as ``generate_data_batches``: one ``torch.randperm`` over the rows of each group of `batch_segment` segments,
    a carried tail included, in group order.

    `groups` (a sequence of indices into `group_sizes`, each at most once) runs the epoch over those segments alone, in the order given --
    what ``EpochLoader.split`` hands its two views: `order` then lists the rows of those segments, still numbered as rows of the WHOLE
    table, and the groups of `batch_segment` are taken along `groups`.  None is every segment in table order."""
    sizes = [int(v) for v in group_sizes]
    if any(v < 0 for v in sizes) or int(batch_segment) < 1 or int(batch_size) < 1:
        raise ValueError("epoch_order: group sizes must be >= 0, batch_segment and batch_size >= 1")
    starts = np.concatenate([[0], np.cumsum(sizes, dtype=np.int64)]).astype(np.int64)
    if groups is not None:
        groups = [int(g) for g in groups]
        if any(g < 0 or g >= len(sizes) for g in groups) or len(set(groups)) != len(groups):
            raise ValueError("epoch_order: groups must be distinct indices into group_sizes")
    n_groups = len(sizes) if groups is None else len(groups)
    order, bounds, emitted = [], [0], 0
    carry = None
    for g0 in range(0, n_groups, batch_segment):
        g1 = min(g0 + batch_segment, n_groups)
        if groups is None:
            rows = torch.arange(int(starts[g0]), int(starts[g1]), dtype=torch.int64)
        else:
            rows = torch.cat([torch.arange(int(starts[g]), int(starts[g + 1]), dtype=torch.int64) for g in groups[g0:g1]])
        if carry is not None:                           # the short tail of the previous group goes FIRST
            rows = torch.cat([carry, rows])
            carry = None
        n = rows.shape[0]
        idx = torch.randperm(n, generator=generator) if shuffle else torch.arange(n)
        rows = rows[idx]
        last = g1 == n_groups
        full = n if last else n - n % batch_size
        if full < n:
            carry = rows[full:]
        for o in range(0, full, batch_size):
            emitted += min(batch_size, full - o)
            bounds.append(emitted)
        order.append(rows[:full])
    order = torch.cat(order) if order else torch.zeros(0, dtype=torch.int64)
    return order, torch.tensor(bounds, dtype=torch.int64)
