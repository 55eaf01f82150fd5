"""Genome summaries reduced in flight from the shards of a file-level prediction: the numpy "host twins" that specify the device
reductions (csrc/summary*.hip, csrc/simulate*.hip) and ``SummarySink``, the shard consumer that runs one reducer per summary kind --
window tables and totals, k-mer tables, motif tables, calibration metrics with the calibrator fit, and the integer tables per name or
transcript (annotations, consequences, transcript structure, INDEL structure and their simulated nulls), whose reducers share one
lifecycle, ``_TableReducer``."""
import ctypes as C
import os
import zlib

import numpy as np
import torch
import torch.distributed as dist

from . import _lib
from .calibration import calibrate_device, dirichlet_calibrate, save_dirichlet_calibrator
from .evaluation import _FIT_MAX_CLASSES, CALIBRATORS, newton_calibrator
from .sinks import _np, _refuse_second_calibration, host_calibrate, shard_bounds, shard_name, strand_u8
from .tables import (annotation_meta, annotation_output_names, check_alt_order, consequence_output_name,
                     consequence_simulation_output_name, consequence_table_from_sums, write_consequence_simulation_outputs,
                     read_transcripts, read_transcript_structure, structure_output_name, write_consequence_outputs,
                     write_structure_outputs, structure_cells_from_sums, structure_simulation_output_name,
                     write_structure_simulation_outputs, simulation_bed_name, simulation_bed_text, simulation_output_name,
                     write_simulation_outputs, check_kmer_length, check_motif_length, kmer_name, kmer_output_names,
                     motif_output_names, mu_scaling_factor, print_scaling_factor, read_annotations, read_regions, regional_output_names,
                     strand_mode, write_annotation_outputs, write_kmer_outputs, write_motif_outputs, write_regional_outputs,
                     check_breakpoint_offset, check_indel_kind, check_indel_lengths, indel_structure_output_name, structure_links,
                     write_indel_structure_outputs, indel_structure_cells_from_sums, indel_structure_simulation_output_name,
                     write_indel_structure_simulation_outputs)


def _refuse_fit_on_calibrated(calibrated):
    """``SummarySink(fit_calibrator=...)`` fits the raw softmax (MuRaL/training.py:478): refused where the sink or the forward
    calibrates."""
    if calibrated:
        raise ValueError("these probabilities are calibrated already (HipShardForward applied its dirichlet_weights / poisson / "
                         "scale_factor chain on the device, or the sink was given poisson= / dirichlet_weights=; poisson defaults to on "
                         "for model_type='indel'): fit_calibrator= fits a calibrator on the raw softmax: drop poisson= / "
                         "dirichlet_weights= / scale_factor=, or build the forward with poisson=False")


# ------------------------------------------------------------------------------------------------------------------
# genome summaries in flight: what calc_scaling_factor and evaluate --window_size read from the written table, reduced from the
# shards while they are on the device (csrc/summary.hip), so that a summary-only pass needs no table at all
# ------------------------------------------------------------------------------------------------------------------
_SUMMARY_STATUS = ((2, "a mut_type outside 0 .. n_class - 1"), (1, "a negative start"),
                   (4, "rows of a chromosome that do not ascend in start"), (8, "a probability that is NaN, negative or above 1"))
_LABEL_KIND = {torch.float32: 0, torch.int32: 1, torch.int64: 2}      # `label_kind` of the device entry points, by the label column's dtype


def summary_rows_host(prob, start, end, label, n_class, windows, regions=None):
    """The numpy twin of ``mural_summary_rows`` for the rows of one chromosome (any order): ({W: (bin0, table [bins][1 + 2 n_class])},
    prob_sum, n_sites, status).  float64, ``np.add.at`` in row order; `regions`: (sorted starts, sorted ends) of the chromosome's
    benchmark regions or None; status bits as on the device (a negative start 1, a label outside 0 .. n_class - 1 2)."""
    k = int(n_class)
    prob = np.asarray(prob)[:, :k].astype(np.float64)
    start, end, label = np.asarray(start, np.int64), np.asarray(end, np.int64), np.asarray(label)
    lab = np.where(np.isfinite(label.astype(np.float64)), label, -1).astype(np.int64)
    bad_label = (lab < 0) | (lab >= k) | (lab != label)
    bad_start = start < 0
    status = (1 if bad_start.any() else 0) | (2 if bad_label.any() else 0)
    ok = ~(bad_label | bad_start)
    prob, start, end, lab = prob[ok], start[ok], end[ok], lab[ok]
    tables = {}
    for W in windows:
        if len(start) == 0:
            tables[W] = (0, np.zeros((0, 1 + 2 * k)))
            continue
        b = start // W
        bin0 = int(b.min())
        t = np.zeros((int(b.max()) - bin0 + 1, 1 + 2 * k))
        np.add.at(t[:, 0], b - bin0, 1.0)
        np.add.at(t, (b - bin0, 1 + lab), 1.0)
        for c in range(k):
            np.add.at(t[:, 1 + k + c], b - bin0, prob[:, c])
        tables[W] = (bin0, t)
    if regions is None:
        w = np.ones(len(start), np.int64)
    else:
        w = np.searchsorted(regions[0], end, "left") - np.searchsorted(regions[1], start, "right")
    total = 0.0
    for v in (w * prob[:, 1:].sum(axis=1))[w > 0].tolist():
        total += v
    return tables, total, int(w[w > 0].sum()), status


# ---- k-mer rate tables (csrc/summary_kmer.hip): exact integer sums of the probabilities quantised to 2^-71 -------------------------------
_KMER_HI_BITS, _KMER_LO_BITS = 31, 40
_KMER_LO_MASK = np.uint64((1 << _KMER_LO_BITS) - 1)
_KMER_ORD_SHIFT = 40               # a chromosome's ordinal sits above any 2 * start + 1 (chromosomes shorter than 2^39 bases)
_KMER_FOLD_ROWS = 1 << 21          # rows between two folds of the lo limbs (the bound of csrc/summary_kmer.hip)
_KMER_NEVER = np.uint64(2 ** 64 - 1)


def _host_genome(genome):
    """(packed2 uint32[], nmask uint32[], length) of a sequence (str / bytes), a ``PackedGenome`` or such a triple."""
    if isinstance(genome, (str, bytes)):
        from .data.genome import pack_sequence
        return pack_sequence(genome)[:3]
    if hasattr(genome, "packed2"):
        return genome.packed2.cpu().numpy().view(np.uint32), genome.nmask.cpu().numpy().view(np.uint32), int(genome.length)
    packed, nmask, length = genome[:3]
    return np.asarray(packed).view(np.uint32), np.asarray(nmask).view(np.uint32), int(length)


def _window_keys_host(host, s0, s1, k):
    """(fwd, rev) int64 of the Python slices chrom[s0:s1] (csrc/kmer_key.h: kmer_window_decode): -1 where a slice is not k bases of
    A/C/G/T.  `host`: ``_host_genome``'s triple."""
    packed, nmask, L = host
    lo = np.where(s0 < 0, np.maximum(L + s0, 0), np.minimum(s0, L))
    hi = np.where(s1 < 0, np.maximum(L + s1, 0), np.minimum(s1, L))
    ok = hi - lo == k
    fwd, rev = np.zeros(len(s0), np.int64), np.zeros(len(s0), np.int64)
    base = np.where(ok, lo, 0)
    for j in range(k):
        q = np.minimum(base + j, max(L - 1, 0))
        if L == 0:
            break
        ok &= ((nmask[q >> 5] >> (q & 31).astype(np.uint32)) & 1) == 0
        code = ((packed[q >> 4] >> (2 * (q & 15)).astype(np.uint32)) & 3).astype(np.int64)
        fwd = fwd * 4 + code
        rev += (3 - code) << (2 * j)
    return np.where(ok, fwd, -1), np.where(ok, rev, -1)


def kmer_keys_host(genome, start, end, strand, k, indel=False, mode=0):
    """The numpy twin of ``mural_table_kmer_keys`` (csrc/kmer_key.h): (key_a, key_b) int64, -1 where the Python slice
    chrom[start - k/2 (+1 indel) : end + k/2] is not k bases of A/C/G/T; key_a follows the strand mode (0 the rows' strand, 1 '+', 2 '-'),
    in mode 3 key_a is the forward key and key_b its reverse complement (otherwise key_b is all -1)."""
    start, end = np.asarray(start, np.int64), np.asarray(end, np.int64)
    fwd, rev = _window_keys_host(_host_genome(genome), start - k // 2 + (1 if indel else 0), end + k // 2, k)
    none = np.full(len(start), -1, np.int64)
    if mode == 3:
        return fwd, rev
    minus = np.ones(len(start), bool) if mode == 2 else (np.asarray(strand) != 0 if mode == 0 else np.zeros(len(start), bool))
    return np.where(minus, rev, fwd), none


def kmer_quantise(prob):
    """(hi, lo, bad) of float probabilities: q = rne(p * 2^71) as hi = floor(p * 2^31), lo = rint((p * 2^31 - hi) * 2^40) (uint64; every
    step exact in float64, float32 widened first); bad: NaN, negative or above 1 (hi = lo = 0 there)."""
    p = np.asarray(prob).astype(np.float64)
    with np.errstate(invalid="ignore"):
        bad = ~((p >= 0.0) & (p <= 1.0))
    p = np.where(bad, 0.0, p)
    s = p * float(1 << _KMER_HI_BITS)
    h = np.floor(s)
    return h.astype(np.uint64), np.rint((s - h) * float(1 << _KMER_LO_BITS)).astype(np.uint64), bad


def _kmer_fold(table):
    """Carry the lo limbs' overflow into hi: table [groups][3][n_class] uint64, in place."""
    carry = table[:, 2] >> np.uint64(_KMER_LO_BITS)
    table[:, 1] += carry
    table[:, 2] &= _KMER_LO_MASK
    return table


def _kmer_row_checks(prob, start, label, nc):
    """(hi, lo, integer labels, rows that count, status bits) of the rows of a k-mer or motif summary."""
    label = np.asarray(label)
    hi, lo, bad_p = kmer_quantise(np.asarray(prob)[:, :nc])
    lab = np.where(np.isfinite(label.astype(np.float64)), label, -1).astype(np.int64)
    bad_label = (lab < 0) | (lab >= nc) | (lab != label)
    bad_start, bad_prob = start < 0, bad_p.any(axis=1)
    status = (1 if bad_start.any() else 0) | (2 if bad_label.any() else 0) | (8 if bad_prob.any() else 0)
    return hi, lo, lab, ~(bad_label | bad_start | bad_prob), status


def summary_kmer_host(genome, prob, start, end, strand, label, n_class, kmers, indel=False, mode=0, order_base=0, into=None):
    """The numpy twin of ``mural_summary_kmer_rows`` -- and its specification -- for rows (any order) of one chromosome:
    ({k: (table uint64 [4^k][3][n_class] of label counts | sums of hi | sums of lo, first uint64 [4^k])}, status).  `genome`: the
    chromosome as a sequence, a ``PackedGenome`` or (packed2, nmask, length); `into`: tables of earlier parts to add to (in place).  Status
    bits as on the device (1 a negative start, 2 a label outside 0 .. n_class - 1, 8 a probability that is NaN, negative or above 1);
    such rows are skipped in every table."""
    nc = int(n_class)
    start, end = np.asarray(start, np.int64), np.asarray(end, np.int64)
    hi, lo, lab, ok, status = _kmer_row_checks(prob, start, label, nc)
    strand = np.zeros(len(start), np.uint8) if strand is None else strand_u8(strand)
    hi, lo, start, end, lab, strand = hi[ok], lo[ok], start[ok], end[ok], lab[ok], np.asarray(strand)[ok]
    if len(start) and int(start.max()) >= 1 << (_KMER_ORD_SHIFT - 1):
        raise ValueError("k-mer summary: a start at or above 2^39")
    host = _host_genome(genome)
    out = {} if into is None else into
    cls = np.arange(nc)
    for k in kmers:
        table, first = out.get(k) or (np.zeros((4 ** k, 3, nc), np.uint64), np.full(4 ** k, _KMER_NEVER, np.uint64))
        for r0 in range(0, len(start), _KMER_FOLD_ROWS):
            r = slice(r0, r0 + _KMER_FOLD_ROWS)
            for sub, key in enumerate(kmer_keys_host(host, start[r], end[r], strand[r], k, indel, mode)):
                live = key >= 0
                kk = key[live]
                np.add.at(table[:, 0], (kk, lab[r][live]), np.uint64(1))
                np.add.at(table[:, 1], (kk[:, None], cls[None, :]), hi[r][live])
                np.add.at(table[:, 2], (kk[:, None], cls[None, :]), lo[r][live])
                np.minimum.at(first, kk, (np.uint64(order_base) + (2 * start[r][live] + sub).astype(np.uint64)))
            _kmer_fold(table)
        out[k] = (table, first)
    return out, status


def kmer_table_from_sums(table, first, k, n_class):
    """(k-mer names, table [groups][1 + 2 n_class] of rows / per-class counts / per-class probability sums) -- ``tables.kmer_table``'s
    pair -- from the integer sums: the keys with a row, by first appearance; a probability sum is (hi * 2^40 + lo) / 2^71, formed from
    Python integers (true division rounds correctly)."""
    nc = int(n_class)
    live = np.nonzero(table[:, 0].sum(axis=1) > 0)[0]
    order = live[np.argsort(first[live], kind="stable")]
    out = np.zeros((len(order), 1 + 2 * nc))
    out[:, 1:1 + nc] = table[order, 0]
    out[:, 0] = table[order, 0].sum(axis=1)
    den = 1 << (_KMER_HI_BITS + _KMER_LO_BITS)
    hi, lo = table[order, 1].tolist(), table[order, 2].tolist()
    for j in range(len(order)):
        out[j, 1 + nc:] = [((h << _KMER_LO_BITS) + l) / den for h, l in zip(hi[j], lo[j])]
    return [kmer_name(int(g), k) for g in order], out


def _kmer_collapse(tables, firsts, shift=_KMER_ORD_SHIFT):
    """({k: table}, {chromosome: {k: first}}) -> (names ascending, {k: (table, first)}): a k-mer's first appearance over the chromosomes
    in ascending name order -- the order of the written table -- with the chromosome's ordinal above the word."""
    names = sorted(firsts)
    out = {}
    for k, table in tables.items():
        first = np.full(table.shape[0], _KMER_NEVER, np.uint64)
        for ordinal, nm in enumerate(names):
            f = firsts[nm][k]
            np.minimum(first, np.where(f != _KMER_NEVER, f | np.uint64(ordinal << shift), _KMER_NEVER), out=first)
        out[k] = (table, first)
    return names, out


def _kmer_merge(states, shift=_KMER_ORD_SHIFT):
    """[(chromosome names ascending, {k: (table, first)})] of the ranks (or of a rank's devices and its host rows) -> one such pair:
    tables added, first-appearance words min-merged after the ordinals are reconciled by name (every list ascends, so renumbering it to
    the merged list keeps the order it was collapsed under)."""
    tables = {}
    names = sorted({nm for their_names, _ in states for nm in their_names})
    low = np.uint64((1 << shift) - 1)
    for their_names, their in states:
        remap = np.array([names.index(nm) for nm in their_names] + [0], np.uint64)
        for k, (table, first) in their.items():
            seen = first != _KMER_NEVER
            moved = first.copy()
            moved[seen] = (remap[(first[seen] >> np.uint64(shift)).astype(np.int64)] << np.uint64(shift)) | (first[seen] & low)
            if k not in tables:
                tables[k] = (table.copy(), moved)
            else:
                tables[k][0][...] += table
                np.minimum(tables[k][1], moved, out=tables[k][1])
                _kmer_fold(tables[k][0])
    return names, tables


# ---- motif rate tables (csrc/summary_kmer.hip: mural_summary_motif_rows): the k-mer cells under the key rule of `evaluate --motif_only` ----
_MOTIF_POS_SHIFT = 5               # first-appearance word: (order_base + pos) << 5 | window i << 1 | orientation
_MOTIF_ORD_SHIFT = 44              # a chromosome's ordinal sits above any such word of a start below 2^39
_MOTIF_FOLD_ROWS = 1 << 18         # rows between two folds: a row adds up to m <= 15 times to one cell


def summary_motif_host(genome, prob, start, end, label, n_class, motifs, indel=False, order_base=0, into=None, order_by_row=False):
    """The numpy twin of ``mural_summary_motif_rows`` -- and its specification -- for rows (any order) of one chromosome:
    ({m: (table uint64 [4^m][3][n_class] of label counts | sums of hi | sums of lo, first uint64 [4^m])}, status).  A row adds to every
    window of m bases that holds its site, on the reference strand: the Python slices chrom[start - i : end + m-1 - i], i = 0 .. m-1, of
    an SNV row, chrom[start - i + 1 : end + m - i], i = 1 .. m-1, of an INDEL row, those that are m bases of A/C/G/T.  A motif and its
    reverse complement share the cell of the smaller key; first = min of (order_base + pos) << 5 | i << 1 | o over the windows, pos the
    row's start (its index among the rows given with `order_by_row`), o = 1 where the window's own key is the larger of the two.
    `genome`, `into` and the status bits as ``summary_kmer_host``."""
    nc = int(n_class)
    start, end = np.asarray(start, np.int64), np.asarray(end, np.int64)
    hi, lo, lab, ok, status = _kmer_row_checks(prob, start, label, nc)
    pos = np.arange(len(start), dtype=np.int64) if order_by_row else start
    hi, lo, start, end, lab, pos = hi[ok], lo[ok], start[ok], end[ok], lab[ok], pos[ok]
    if len(start) and int(pos.max()) + int(order_base) >= 1 << 58:
        raise ValueError("motif summary: a row order at or above 2^58")
    host = _host_genome(genome)
    out = {} if into is None else into
    cls = np.arange(nc)
    for m in motifs:
        m = check_motif_length(m, device=True)
        table, first = out.get(m) or (np.zeros((4 ** m, 3, nc), np.uint64), np.full(4 ** m, _KMER_NEVER, np.uint64))
        for r0 in range(0, len(start), _MOTIF_FOLD_ROWS):
            r = slice(r0, r0 + _MOTIF_FOLD_ROWS)
            word = (np.uint64(order_base) + pos[r].astype(np.uint64)) << np.uint64(_MOTIF_POS_SHIFT)
            for w in range(m - (1 if indel else 0)):           # the reference's i = w + indel
                fwd, rev = _window_keys_host(host, start[r] - w, end[r] + (m - 1 - w), m)
                live = fwd >= 0
                kk = np.minimum(fwd, rev)[live]
                np.add.at(table[:, 0], (kk, lab[r][live]), np.uint64(1))
                np.add.at(table[:, 1], (kk[:, None], cls[None, :]), hi[r][live])
                np.add.at(table[:, 2], (kk[:, None], cls[None, :]), lo[r][live])
                np.minimum.at(first, kk, word[live] | np.uint64((w + (1 if indel else 0)) << 1) | (fwd > rev)[live].astype(np.uint64))
            _kmer_fold(table)
        out[m] = (table, first)
    return out, status


def motif_table_from_sums(table, first, m, n_class):
    """(motif names, table [entries][1 + 2 n_class] of windows / per-class counts / per-class probability sums) -- ``tables.motif_table``'s
    pair -- from the merged integer tables: the keys with a window, by first appearance; an entry is named after the orientation of its
    first window (the lowest bit of its word: 1 the reverse complement of the smaller key).  Sums as ``kmer_table_from_sums``."""
    names, out = kmer_table_from_sums(table, first, m, n_class)
    live = np.nonzero(table[:, 0].sum(axis=1) > 0)[0]
    order = live[np.argsort(first[live], kind="stable")]
    flip = (first[order] & np.uint64(1)).astype(bool)
    top = 4 ** m - 1
    return [kmer_name(top - _revdigits(int(g), m) if f else int(g), m) for g, f in zip(order, flip)], out


def _revdigits(key, m):
    """The base-4 digits of a key in reverse order (4^m - 1 - that is the key of the reverse complement)."""
    out = 0
    for _ in range(m):
        out, key = out * 4 + (key & 3), key >> 2
    return out


# ---- annotation tables (csrc/summary_annot.hip: mural_summary_annot_rows): the k-mer cells per named interval set ----------------------
_ANNOT_SLICE_ROWS = 1 << 20        # rows of one prefix-sum slice here (any size below 2^23 keeps the unfolded lo prefixes below 2^63)
_ANNOT_FOLD_PIECES = 1 << 20       # pieces between two folds of the table: lo < 2^40 + 2^20 * 2^40


def summary_annot_host(prob, start, label, n_class, pieces, n_groups, into=None):
    """The numpy twin of ``mural_summary_annot_rows`` -- and its specification -- for rows (any order) of one chromosome:
    (table uint64 [n_groups][3][n_class] of label counts | sums of hi | sums of lo, status).  `pieces`: the chromosome's (b0, b1, group)
    of ``tables.read_annotations`` (or None); a row adds to the cells of piece p's group when b0[p] <= start < b1[p] -- the pieces of one
    group are disjoint, so once per group that covers it.  The rows are sorted by start, a piece's rows are the range between the lower
    bounds of its two ends, its sums the difference of two prefix sums: integer sums of the limbs of ``kmer_quantise``, so the table is a
    function of the SET of rows alone, bit for bit; on return lo < 2^40.  `into`: the table of earlier parts (and chromosomes) to add
    to, in place.  Status bits as ``summary_kmer_host`` (1, 2, 8); such rows are skipped."""
    nc, ng = int(n_class), int(n_groups)
    start = np.asarray(start, np.int64)
    hi, lo, lab, ok, status = _kmer_row_checks(prob, start, label, nc)
    table = np.zeros((ng, 3, nc), np.uint64) if into is None else into
    if pieces is None or len(pieces[0]) == 0:
        return table, status
    b0, b1, grp = (np.asarray(x) for x in pieces)
    order = np.argsort(start[ok], kind="stable")
    hi, lo, start, lab = hi[ok][order], lo[ok][order], start[ok][order], lab[ok][order]
    for r0 in range(0, len(start), _ANNOT_SLICE_ROWS):
        r = slice(r0, r0 + _ANNOT_SLICE_ROWS)
        st = start[r]
        prefix = np.zeros((len(st) + 1, 3, nc), np.uint64)
        np.cumsum(lab[r][:, None] == np.arange(nc)[None, :], axis=0, dtype=np.uint64, out=prefix[1:, 0])
        np.cumsum(hi[r], axis=0, dtype=np.uint64, out=prefix[1:, 1])
        np.cumsum(lo[r], axis=0, dtype=np.uint64, out=prefix[1:, 2])
        i0 = np.searchsorted(st, b0, "left")
        i1 = np.maximum(np.searchsorted(st, b1, "left"), i0)
        live = np.nonzero(i1 > i0)[0]
        for q0 in range(0, len(live), _ANNOT_FOLD_PIECES):
            q = live[q0:q0 + _ANNOT_FOLD_PIECES]
            np.add.at(table, grp[q], _kmer_fold(prefix[i1[q]] - prefix[i0[q]]))
            _kmer_fold(table)
    return table, status


def annot_table_from_sums(table, n_class):
    """table float64 [n_groups][1 + 2 n_class] of rows / per-class counts / per-class probability sums from the integer sums of
    ``summary_annot_host`` / ``mural_summary_annot_rows``: a probability sum is (hi * 2^40 + lo) / 2^71, formed from Python integers."""
    nc = int(n_class)
    out = np.zeros((table.shape[0], 1 + 2 * nc))
    out[:, 1:1 + nc] = table[:, 0]
    out[:, 0] = table[:, 0].sum(axis=1)
    den = 1 << (_KMER_HI_BITS + _KMER_LO_BITS)
    hi, lo = table[:, 1].ravel().tolist(), table[:, 2].ravel().tolist()      # (one flat pass: there may be 10^5 names)
    out[:, 1 + nc:] = np.array([((h << _KMER_LO_BITS) + l) / den for h, l in zip(hi, lo)], np.float64).reshape(table.shape[0], nc)
    return out


# ---- consequence tables (csrc/summary_conseq.hip: mural_summary_conseq_rows): the k-mer cells per transcript and consequence ---------------
_CONSEQ_PAIRS = 1 << 20            # (row, segment) pairs of one vectorised pass here
_CONSEQ_STOP = ord("*")


def _conseq_row_checks(prob, start, label):
    """(hi, lo [n][3] of classes 1 .. 3, integer labels, rows that count, status bits): class 0's probability is not read."""
    label = np.asarray(label)
    hi, lo, bad_p = kmer_quantise(np.asarray(prob)[:, 1:4])
    lab = np.where(np.isfinite(label.astype(np.float64)), label, -1).astype(np.int64)
    bad_label = (lab < 0) | (lab >= 4) | (lab != label)
    bad_start, bad_prob = start < 0, bad_p.any(axis=1)
    status = (1 if bad_start.any() else 0) | (2 if bad_label.any() else 0) | (8 if bad_prob.any() else 0)
    return hi, lo, lab, ~(bad_label | bad_start | bad_prob), status


def _item_row_pairs(start, b0, b1):
    """(item, row) index arrays of every pair with b0[item] <= start[row] < b1[item], `start` ascending: passes of at most
    ``_CONSEQ_PAIRS`` pairs, item by item."""
    i0 = np.searchsorted(start, b0, "left")
    i1 = np.maximum(np.searchsorted(start, b1, "left"), i0)
    n_in = i1 - i0
    ends = np.cumsum(n_in)
    total = int(ends[-1]) if len(ends) else 0
    for p0 in range(0, total, _CONSEQ_PAIRS):
        pair = np.arange(p0, min(p0 + _CONSEQ_PAIRS, total), dtype=np.int64)
        s = np.searchsorted(ends, pair, "right")                       # the pair's item
        yield s, i0[s] + (pair - (ends[s] - n_in[s]))                  # and its row


def _conseq_pairs(genome, start, rs, segments, aa, alt_of, with_offset=False):
    """The one bin rule of the consequence tables on the host, shared by ``summary_conseq_host`` and ``simulate_conseq_host``: for rows
    sorted by start (`rs`: their strands as int64 0 / 1) and a chromosome's `segments`, yields (i, tx, bins) per pass of at most
    ``_CONSEQ_PAIRS`` (segment, row) pairs with seg_b0 <= start[i] < seg_b1 -- the row index, the segment's transcript and bins int64
    [pairs][3], the bin 0 .. 4 of classes 1 .. 3 by the rule ``summary_conseq_host`` states.  `with_offset`: (i, tx, bins, x), x the CDS
    offset of each pair's row (``summary_txstruct_host`` asks whether it lies in codon 0)."""
    b0, b1, cds0 = (np.asarray(segments[key], np.int64) for key in ("seg_b0", "seg_b1", "seg_cds0"))
    seg_tx, prev, nxt = (np.asarray(segments[key], np.int64) for key in ("seg_tx", "seg_prev", "seg_next"))
    tx_minus, tx_len = np.asarray(segments["tx_strand"]) != 0, np.asarray(segments["tx_cds_len"], np.int64)
    packed, nmask, L = _host_genome(genome)
    for s, i in _item_row_pairs(start, b0, b1):
        q, tx = start[i], seg_tx[s]
        minus = tx_minus[tx]
        x = cds0[s] + np.where(minus, b1[s] - 1 - q, q - b0[s])
        cs = x - x % 3
        found = cs + 2 < tx_len[tx]
        codon = np.zeros(len(s), np.int64)
        for j in range(3):
            o, cur = cs + j, s.copy()
            for _ in range(2):
                c0, ln = cds0[cur], b1[cur] - b0[cur]
                hop = np.where(o < c0, prev[cur], np.where(o >= c0 + ln, nxt[cur], cur))
                found &= hop >= 0
                cur = np.where(hop >= 0, hop, cur)
            c0 = cds0[cur]
            found &= (o >= c0) & (o < c0 + b1[cur] - b0[cur]) & (seg_tx[cur] == tx)
            pos = np.where(minus, b1[cur] - 1 - (o - c0), b0[cur] + (o - c0))
            found &= (pos >= 0) & (pos < L)
            at = np.where(found, pos, 0)
            if L:
                found &= ((nmask[at >> 5] >> (at & 31).astype(np.uint32)) & 1) == 0
                code = ((packed[at >> 4] >> (2 * (at & 15)).astype(np.uint32)) & 3).astype(np.int64)
            else:
                code = np.zeros(len(s), np.int64)
            codon = codon * 4 + np.where(minus, 3 - code, code)
        codon = np.where(found, codon, 0)
        sh = 2 * (2 - (x - cs))
        own_tx = (codon >> sh) & 3
        flip = minus != (rs[i] != 0)
        r = np.where(flip, 3 - own_tx, own_tx)
        bins = np.empty((len(s), 3), np.int64)
        for c in range(3):
            alt = alt_of[r, c]
            alt_tx = np.where(flip, 3 - alt, alt)
            a_ref, a_alt = aa[codon], aa[(codon & ~(3 << sh)) | (alt_tx << sh)]
            b = np.where(a_ref == a_alt, 0, np.where(a_alt == _CONSEQ_STOP, 2, np.where(a_ref == _CONSEQ_STOP, 3, 1)))
            bins[:, c] = np.where(found, b, 4)
        yield (i, tx, bins, x) if with_offset else (i, tx, bins)


def summary_conseq_host(genome, prob, start, strand, label, segments, n_transcripts, aa=None, alt_order=None, into=None, n_class=4):
    """The numpy twin of ``mural_summary_conseq_rows`` -- and its specification -- for SNV rows (any order) of one chromosome:
    (table uint64 [n_transcripts][5][3], rows uint64 [n_transcripts][2], status).  `segments`: the chromosome's dict of
    ``tables.read_transcripts`` (or None); `aa`: uint8 [64] (``tables.check_codon_table``; None: the standard code); `alt_order`:
    ``tables.check_alt_order``'s argument; `strand`: 1 / '-' where the row is on the reverse strand, None for all '+'.

    For row i at q = start[i] and every segment with seg_b0 <= q < seg_b1: g = the reference base at q, r = the row's own base
    (comp(g) where strand[i]); class c = 1 .. 3 is the substitution r > alt_order[r][c - 1] on the row's strand, complemented onto the
    reference strand where strand[i]; x = seg_cds0 + (q - seg_b0) on a '+' transcript, seg_cds0 + (seg_b1 - 1 - q) on a '-' one; the
    codon is offsets 3 floor(x / 3) .. + 2, mapped to genomic positions over seg_prev / seg_next (at most two hops each), complemented
    for a '-' transcript and read 5' -> 3'.  All three classes go to bin 4 (unresolved) when 3 floor(x / 3) + 2 >= tx_cds_len, a codon
    base is masked (N or IUPAC) or a codon position falls outside the record; otherwise class c goes to bin 0 (synonymous: aa_ref ==
    aa_alt, stop -> stop included), 2 (stop gained: aa_alt == '*'), 3 (stop lost: aa_ref == '*') or 1 (missense).  Cell [t][b] += {label
    == c, hi(p_c), lo(p_c)} (the limbs of ``kmer_quantise``) per (row, c) routed to bin b of transcript t; rows[t] += {1, label == 0}
    per row inside t's CDS.  A row counts once per transcript that covers it; integer sums, so both tables are a function of the SET of
    rows, bit for bit; on return lo < 2^40.  `into`: (table, rows) of earlier parts and chromosomes to add to, in place.  Status bits: 1
    a negative start, 2 a label outside 0 .. 3, 8 a probability of a class >= 1 that is NaN, negative or above 1; such rows are
    skipped."""
    from .tables import check_alt_order, check_codon_table
    if int(n_class) != 4:
        raise ValueError("the consequence table takes SNV rows of 4 classes (INDEL tables are out of scope)")
    n_tx = int(n_transcripts)
    aa = check_codon_table(aa).astype(np.int64)
    alt_of = check_alt_order(alt_order).astype(np.int64)
    start = np.asarray(start, np.int64)
    hi, lo, lab, ok, status = _conseq_row_checks(prob, start, label)
    table, rows = (np.zeros((n_tx, 5, 3), np.uint64), np.zeros((n_tx, 2), np.uint64)) if into is None else into
    if segments is None or len(segments["seg_b0"]) == 0 or not ok.any():
        return table, rows, status
    rs = np.zeros(len(start), np.int64) if strand is None else strand_u8(strand).astype(np.int64)
    order = np.argsort(start[ok], kind="stable")
    hi, lo, start, lab, rs = hi[ok][order], lo[ok][order], start[ok][order], lab[ok][order], rs[ok][order]
    flat_table, flat_rows = table.reshape(-1), rows.reshape(-1)
    for i, tx, bins in _conseq_pairs(genome, start, rs, segments, aa, alt_of):
        cell = tx * 15
        for c in range(3):
            b = bins[:, c]
            np.add.at(flat_table, cell + 3 * b, (lab[i] == c + 1).astype(np.uint64))
            np.add.at(flat_table, cell + 3 * b + 1, hi[i, c])
            np.add.at(flat_table, cell + 3 * b + 2, lo[i, c])
        np.add.at(flat_rows, 2 * tx, np.uint64(1))
        np.add.at(flat_rows, 2 * tx + 1, (lab[i] == 0).astype(np.uint64))
        _conseq_fold(table)
    return table, rows, status


def _conseq_fold(table):
    """Carry the lo limbs' overflow into hi: table [transcripts][5][3] uint64, in place."""
    table[:, :, 1] += table[:, :, 2] >> np.uint64(_KMER_LO_BITS)
    table[:, :, 2] &= _KMER_LO_MASK
    return table


def _upload_once(cache, name, arrays, dev):
    """The device copies of `arrays` (an iterable, read only the first time) in cache[name]: uploaded once, from pinned memory and
    non-blocking -- behind the work already enqueued; a pageable copy would wait for the forward --, the pinned tuple kept alive as the
    last element."""
    on_dev = cache.get(name)
    if on_dev is None:
        pinned = tuple(torch.from_numpy(np.ascontiguousarray(x)).pin_memory() for x in arrays)
        on_dev = cache[name] = tuple(x.to(dev, non_blocking=True) for x in pinned) + (pinned,)
    return on_dev


def _grow_ws(acc, need, dev):
    """(pointer, bytes) of acc["ws"], grown to `need` bytes or more (the launches of one stream run in order: one workspace serves
    every entry that uses `acc`)."""
    if acc["ws"] is None or acc["ws"].numel() * 8 < need:
        acc["ws"] = torch.empty(need // 8 + 1, dtype=torch.int64, device=dev)
    return acc["ws"].data_ptr(), acc["ws"].numel() * 8


def _fill_rows(s, n_class, prob, prob_f64, prob_stride, start, n, strand=None, label=None, label_kind=None):
    """The row fields every ``*_rows`` argument struct has, from device pointers; `strand` and `label` where the entry reads them."""
    s.prob, s.prob_f64, s.prob_stride = prob, int(prob_f64), int(prob_stride)
    s.start, s.n, s.n_class = start, int(n), int(n_class)
    if strand is not None:
        s.strand = strand
    if label is not None:
        s.label, s.label_kind = label, int(label_kind)


_SEG_KEYS = ("seg_b0", "seg_b1", "seg_cds0", "seg_tx", "seg_prev", "seg_next")
_FEAT_KEYS = ("feat_b0", "feat_b1", "feat_tx", "feat_kind", "feat_seg", "feat_prev", "feat_next")


def _fill_transcripts(s, n_transcripts, tx, seg_dev, n_seg_keys, feat_dev=None, codons=None):
    """The transcript fields of a per-transcript argument struct: the strands and CDS lengths `tx`, the first `n_seg_keys` segment
    arrays of `seg_dev` (None or empty: the chromosome has no CDS; 6 for the SNV structs, 4 for the INDEL structs, which have no
    seg_prev / seg_next), the item arrays `feat_dev` (with their links where uploaded) and `codons` = (aa, alt_order, genome_struct)
    for the entries that read codons."""
    s.n_transcripts = int(n_transcripts)
    s.tx_strand, s.tx_cds_len = tx[0].data_ptr(), tx[1].data_ptr()
    if seg_dev is not None and seg_dev[0].shape[0]:
        for key, x in zip(_SEG_KEYS[:n_seg_keys], seg_dev):
            setattr(s, key, x.data_ptr())
        s.n_segments = int(seg_dev[0].shape[0])
    if feat_dev is not None:
        for key, x in zip(_FEAT_KEYS, feat_dev[:-1]):
            setattr(s, key, x.data_ptr())
        s.n_features = int(feat_dev[0].shape[0])
    if codons is not None:
        aa, alt_order, genome_struct = codons
        s.genome = C.pointer(genome_struct)
        C.memmove(s.aa, np.ascontiguousarray(aa, np.uint8).ctypes.data, 64)
        C.memmove(s.alt_order, np.ascontiguousarray(alt_order, np.uint8).ctypes.data, 12)


def _fill_indel(s, kind, breakpoint_offset, class_len, chrom_length):
    s.kind, s.breakpoint_offset, s.chrom_length = int(kind), int(breakpoint_offset), -1 if chrom_length is None else int(chrom_length)
    for c, (lo, hi) in enumerate(np.asarray(class_len).tolist()[:16]):
        s.class_len[c][0], s.class_len[c][1] = lo, hi


def _conseq_segments_device(acc, name, segments, dev):
    """The device arrays of chromosome `name`'s segments in acc["segments"], and the transcripts' strands and CDS lengths in acc["tx"]
    (`segments` may be a chromosome's dict of features: it has the same two): uploaded the first time, from pinned memory."""
    _upload_once(acc, "tx", (segments[key] for key in ("tx_strand", "tx_cds_len")), dev)
    if "seg_b0" not in segments:
        return None
    return _upload_once(acc["segments"], name, (segments[key] for key in _SEG_KEYS), dev)


def conseq_rows_device(acc, name, segments, n_transcripts, aa, alt_order, genome_struct, dev, *, prob, prob_f64, prob_stride, start,
                       strand, label, label_kind, n):
    """One ``mural_summary_conseq_rows`` call on device pointers into the accumulators of `acc` (dict: table int64 [n_transcripts * 15], rows int64 [n_transcripts * 2], status int32 [1],
    segments {chromosome: device arrays}, ws): the chromosome's segment arrays are uploaded the first time it arrives, the workspace
    grows as needed."""
    lib = _lib.lib()
    on_dev = _conseq_segments_device(acc, name, segments, dev)
    s = _lib.MuralSummaryConseqRows()
    _fill_rows(s, 4, prob, prob_f64, prob_stride, start, n, strand, label, label_kind)
    _fill_transcripts(s, n_transcripts, acc["tx"], on_dev, 6, codons=(aa, alt_order, genome_struct))
    s.table, s.rows, s.status = acc["table"].data_ptr(), acc["rows"].data_ptr(), acc["status"].data_ptr()
    ws = _grow_ws(acc, int(lib.mural_summary_conseq_workspace_bytes(int(on_dev[0].shape[0]))), dev)
    _lib.check(lib.mural_summary_conseq_rows(C.byref(s), *ws, _lib.current_stream_ptr(dev)))


# ---- structure tables (csrc/summary_txstruct.hip: mural_summary_txstruct_rows): the same cells per transcript and place in its structure ---
TX_BINS = 9


def _txstruct_pairs(genome, start, rs, segments, features, aa, alt_of):
    """The one item walk and bin rule of the structure tables on the host, shared by ``summary_txstruct_host`` and
    ``simulate_txstruct_host``: for rows sorted by start (`rs`: their strands as int64 0 / 1), a chromosome's `features` and its
    `segments` (or None), yields (i, tx, bins) per pass of at most ``_CONSEQ_PAIRS`` (item, row) pairs with feat_b0 <= start[i] <
    feat_b1 -- the row index, the item's transcript and bins int64 [pairs][3], the bin 0 .. 8 of classes 1 .. 3 by the rule
    ``summary_txstruct_host`` states.  The CDS parts are the segments: they go through ``_conseq_pairs``."""
    kind = np.asarray(features["feat_kind"], np.int64)
    other = np.nonzero(kind != 5)[0]
    a, b = np.asarray(features["feat_b0"], np.int64)[other], np.asarray(features["feat_b1"], np.int64)[other]
    f_tx, kind = np.asarray(features["feat_tx"], np.int64)[other], kind[other]
    tx_minus = np.asarray(features["tx_strand"]) != 0
    for f, i in _item_row_pairs(start, a, b):
        q, tx = start[i], f_tx[f]
        sites = (kind[f] >= 3) & (b[f] - a[f] >= 4)
        low, high = sites & (q < a[f] + 2), sites & (q >= b[f] - 2)
        donor = np.where(tx_minus[tx], high, low)
        site_bin = np.where(kind[f] == 3, np.where(donor, 3, 4), 5)
        bins = np.where(kind[f] < 3, kind[f], np.where(low | high, site_bin, 6))
        yield i, tx, np.repeat(bins[:, None], 3, axis=1)
    if segments is not None and len(segments["seg_b0"]):
        for i, tx, bins, x in _conseq_pairs(genome, start, rs, segments, aa, alt_of, with_offset=True):
            yield i, tx, np.where((x < 3)[:, None] & (bins >= 1) & (bins <= 3), 7, 8)


def summary_txstruct_host(genome, prob, start, strand, label, segments, features, n_transcripts, aa=None, alt_order=None, into=None,
                          n_class=4):
    """The numpy twin of ``mural_summary_txstruct_rows`` -- and its specification -- for SNV rows (any order) of one chromosome: (table
    uint64 [n_transcripts][9][3], rows uint64 [n_transcripts][2], status).  `segments`, `features`: the chromosome's dicts of
    ``tables.read_transcript_structure`` (or None); the other arguments, the row checks and the status bits are
    ``summary_conseq_host``'s.  The bins (``tables.STRUCTURE_BINS``): 0 utr5, 1 utr3, 2 noncoding_exon, 3 splice_donor, 4
    splice_acceptor, 5 splice_utr, 6 intron, 7 start_lost, 8 cds.

    For row i at q = start[i] and every item [a, b) = [feat_b0, feat_b1) with a <= q < b, by the item's kind:
      0, 1, 2 (5'UTR part, 3'UTR part, exon of a transcript without CDS): all three classes go to bin 0, 1 or 2;
      3, 4 (coding intron, other gap): with b - a < 4 there are no splice sites and all classes go to bin 6; otherwise the 5' two bases
        in transcript orientation are the donor ([a, a + 2) on '+', [b - 2, b) on '-') and the other end's two the acceptor: a donor or
        acceptor row goes to bin 3 or 4 in a coding intron and to bin 5 in any other gap, every other row to bin 6;
      5 (CDS part): x and the codon are ``summary_conseq_host``'s (``_conseq_pairs``); class c goes to bin 7 iff x < 3, the codon
        resolves and aa_alt != aa_ref, and to bin 8 otherwise -- an unresolved first codon and cds_length < 3 included.  BED12 carries no
        frame and the rule does not demand ATG: `start lost` is "changes the amino acid of CDS codon 0".
    Cell [t][b] += {label == c, hi(p_c), lo(p_c)} per class c that lands in bin b of transcript t; rows[t] += {1, label == 0} per row
    inside t's span -- a transcript's items tile its span, so a row counts once per transcript that covers it.  Integer sums: both
    tables are a function of the SET of rows, bit for bit; on return lo < 2^40; class 0's probability is never read.  For every t the
    cells [t][7] + [t][8] add up to the five cells of ``summary_conseq_host``'s table[t], the observed word by word and the
    probability as the integer hi 2^40 + lo.  `into`: (table, rows) of earlier parts and chromosomes to add to, in place."""
    from .tables import check_alt_order, check_codon_table
    if int(n_class) != 4:
        raise ValueError("the structure table takes SNV rows of 4 classes (INDEL tables are out of scope)")
    n_tx = int(n_transcripts)
    aa = check_codon_table(aa).astype(np.int64)
    alt_of = check_alt_order(alt_order).astype(np.int64)
    start = np.asarray(start, np.int64)
    hi, lo, lab, ok, status = _conseq_row_checks(prob, start, label)
    table, rows = (np.zeros((n_tx, TX_BINS, 3), np.uint64), np.zeros((n_tx, 2), np.uint64)) if into is None else into
    if features is None or len(features["feat_b0"]) == 0 or not ok.any():
        return table, rows, status
    rs = np.zeros(len(start), np.int64) if strand is None else strand_u8(strand).astype(np.int64)
    order = np.argsort(start[ok], kind="stable")
    hi, lo, start, lab, rs = hi[ok][order], lo[ok][order], start[ok][order], lab[ok][order], rs[ok][order]
    flat_table, flat_rows = table.reshape(-1), rows.reshape(-1)

    def add(i, tx, bins):      # bins int64 [pairs][3]
        cell = tx * (3 * TX_BINS)
        for c in range(3):
            b = bins[:, c]
            np.add.at(flat_table, cell + 3 * b, (lab[i] == c + 1).astype(np.uint64))
            np.add.at(flat_table, cell + 3 * b + 1, hi[i, c])
            np.add.at(flat_table, cell + 3 * b + 2, lo[i, c])
        np.add.at(flat_rows, 2 * tx, np.uint64(1))
        np.add.at(flat_rows, 2 * tx + 1, (lab[i] == 0).astype(np.uint64))
        _conseq_fold(table)

    for i, tx, bins in _txstruct_pairs(genome, start, rs, segments, features, aa, alt_of):
        add(i, tx, bins)
    return table, rows, status


def txstruct_rows_device(acc, conseq_acc, name, segments, features, n_transcripts, aa, alt_order, genome_struct, dev, *, prob, prob_f64,
                         prob_stride, start, strand, label, label_kind, n):
    """One ``mural_summary_txstruct_rows`` call on device pointers into the accumulators of `acc`
    (dict: table int64 [n_transcripts * 27], rows int64 [n_transcripts * 2], status int32 [1], features {chromosome: device arrays},
    ws): the chromosome's item arrays are uploaded the first time it arrives, the workspace grows as needed.  The segment arrays are
    those of `conseq_acc` (dict with "segments": {}), ``conseq_rows_device``'s accumulators, which uploaded them for chromosome `name`
    just before -- or they are uploaded into it now; `segments` None: the chromosome has no CDS."""
    lib = _lib.lib()
    on_dev = _upload_once(acc["features"], name, (features[key] for key in _FEAT_KEYS[:5]), dev)
    seg_dev = _conseq_segments_device(conseq_acc, name, features if segments is None else segments, dev)
    s = _lib.MuralSummaryTxstructRows()
    _fill_rows(s, 4, prob, prob_f64, prob_stride, start, n, strand, label, label_kind)
    _fill_transcripts(s, n_transcripts, conseq_acc["tx"], seg_dev, 6, on_dev, codons=(aa, alt_order, genome_struct))
    s.table, s.rows, s.status = acc["table"].data_ptr(), acc["rows"].data_ptr(), acc["status"].data_ptr()
    ws = _grow_ws(acc, int(lib.mural_summary_txstruct_workspace_bytes(int(on_dev[0].shape[0]))), dev)
    _lib.check(lib.mural_summary_txstruct_rows(C.byref(s), *ws, _lib.current_stream_ptr(dev)))


# ---- INDEL structure tables (csrc/summary_txindel.hip: mural_summary_txindel_rows): what an INDEL event does to the transcript -----------
TXINDEL_BINS = 10
_TXINDEL_MAX_WALK = 64             # the longest deletion: a walk moves on by a base or more every step


def _txindel_frame_bin(lo, hi, n):
    """The frame bin of a class of lengths lo .. hi with `n` CDS bases affected (an array): 9 for a mixed class, 7 for a range without a
    multiple of 3, and for a framed class 7 where n % 3 != 0, else 8."""
    if lo == hi:
        return np.where(n % 3 != 0, 7, 8)
    return np.full(np.shape(n), 9 if hi // 3 > (lo - 1) // 3 else 7, np.int64)


def _txindel_pairs(start, segments, features, links, n_tx, kind, off, cl, chrom_length):
    """The one item walk and bin rule of the INDEL structure tables on the host, shared by ``summary_txindel_host`` and
    ``simulate_txindel_host``: for rows sorted by start, a chromosome's `features`, its `segments` (or None) and `links` (None: built
    here), the checked `kind` 0 / 1 / 2, breakpoint offset `off` and class lengths `cl` int [n_class][2], yields (i, tx, counted, bins)
    per pass of at most ``_CONSEQ_PAIRS`` (home item, row) pairs -- the row indices, the home item's transcript, whether the transcript
    counts the row (an insertion on the span's last boundary does not) and bins int64 [pairs][n_class - 1], the bin 0 .. 9 of classes
    1 .. n_class - 1 by the rule ``summary_txindel_host`` states.  Home items that a walk may not stand on are skipped."""
    k = len(cl)
    b0, b1 = np.asarray(features["feat_b0"], np.int64), np.asarray(features["feat_b1"], np.int64)
    f_tx, f_kind, f_seg = (np.asarray(features[key], np.int64) for key in ("feat_tx", "feat_kind", "feat_seg"))
    prev, nxt = (np.asarray(x, np.int64) for x in (structure_links(features) if links is None else links))
    tx_minus, tx_len = np.asarray(features["tx_strand"]) != 0, np.asarray(features["tx_cds_len"], np.int64)
    n_feat = len(b0)
    # the items a walk may stand on, and the CDS offset of a CDS part's first base in transcript orientation
    item_ok = (b1 > b0) & (f_kind <= 5) & (f_tx >= 0) & (f_tx < n_tx)
    cds0, is_cds = np.zeros(n_feat, np.int64), f_kind == 5
    if is_cds.any():
        n_seg = 0 if segments is None else len(segments["seg_b0"])
        good = is_cds & (f_seg >= 0) & (f_seg < n_seg)
        if n_seg:
            s = np.where(good, f_seg, 0)
            good &= ((np.asarray(segments["seg_b0"], np.int64)[s] == b0) & (np.asarray(segments["seg_b1"], np.int64)[s] == b1)
                     & (np.asarray(segments["seg_tx"], np.int64)[s] == f_tx))
            cds0 = np.where(good, np.asarray(segments["seg_cds0"], np.int64)[s], 0)
        item_ok &= ~is_cds | good
    home = np.nonzero(item_ok)[0]
    shift = off - (0 if kind == 1 else 1)

    def neighbour(cur, tx, step):
        """(index, usable) of the item behind `cur` (step: the link array) for transcript tx."""
        at = step[cur]
        inside = (at >= 0) & (at < n_feat)
        at = np.where(inside, at, 0)
        return at, inside & item_ok[at] & (f_tx[at] == tx)

    def cds_rule(x, cds_len):
        return np.where(x == 0, 0, np.where(x == cds_len, 1, np.where(x <= 2, 6, -1)))

    for s, i in _item_row_pairs(start + shift, b0[home], b1[home]):
        f = home[s]
        j, tx, a, b, kd = start[i] + off, f_tx[f], b0[f], b1[f], f_kind[f]
        minus, cds_len = tx_minus[tx], tx_len[tx]
        if kind == 0:
            at, usable = neighbour(f, tx, nxt)
            usable &= b0[at] == b
            same, kb = j < b, f_kind[at]
            gap_a, gap_b = (kd == 3) | (kd == 4), (kb == 3) | (kb == 4)
            split = (b - a >= 4) & ((j == a + 1) | (j == b - 1))
            site_same = np.where(kd < 3, kd, np.where(gap_a, np.where(split, np.where(kd == 3, 3, 4), 5),
                                                      cds_rule(cds0[f] + np.where(minus, b - j, j - a), cds_len)))
            site_diff = np.where(kd == 5, cds_rule(cds0[f] + np.where(minus, 0, b - a), cds_len),
                                 np.where(kb == 5, cds_rule(cds0[at] + np.where(minus, b1[at] - b0[at], 0), cds_len),
                                          np.where(gap_a & gap_b, 5, np.where(gap_a, kb, kd))))
            site, counted = np.where(same, site_same, site_diff), same | usable
        else:
            counted = np.ones(len(i), bool)
        bins_all = np.empty((len(i), k - 1), np.int64)
        for c in range(1, k):
            c_lo, c_hi = int(cl[c, 0]), int(cl[c, 1])
            if kind == 0:
                bins = np.where(site < 0, _txindel_frame_bin(c_lo, c_hi, np.full(len(i), c_lo, np.int64)), site)
            else:
                fwd = kind == 1
                d0, d1 = (j, j + c_lo) if fwd else (np.maximum(j - c_lo, 0), j)
                if fwd and chrom_length is not None and int(chrom_length) >= 0:
                    d1 = np.maximum(np.minimum(d1, int(chrom_length)), j + 1)
                n_cds, touch = np.zeros(len(i), np.int64), np.zeros(len(i), np.int64)
                cur, on = f.copy(), np.ones(len(i), bool)
                for _ in range(_TXINDEL_MAX_WALK + 1):
                    u, v = np.maximum(b0[cur], d0), np.minimum(b1[cur], d1)
                    meets, ck, c0 = on & (u < v), f_kind[cur], cds0[cur]
                    n_cds += np.where(meets & (ck == 5), v - u, 0)
                    first = np.where(minus, v > np.maximum(b0[cur], b1[cur] - (3 - c0)), u < np.minimum(b1[cur], b0[cur] + (3 - c0)))
                    sites = (b1[cur] - b0[cur] >= 4) & ((u < b0[cur] + 2) | (v > b1[cur] - 2))
                    for bit, where in ((1, (ck == 5) & (c0 < 3) & first), (2, (ck == 3) & sites), (4, (ck == 4) & sites), (8, ck == 2),
                                       (16, ck == 0), (32, ck == 1)):
                        touch |= np.where(meets & where, bit, 0)
                    on &= (b1[cur] < d1) if fwd else (b0[cur] > d0)
                    if not on.any():
                        break
                    at, usable = neighbour(cur, tx, nxt if fwd else prev)
                    on &= usable & ((b0[at] == b1[cur]) if fwd else (b1[at] == b0[cur]))
                    cur = np.where(on, at, cur)
                bins = np.where(touch & 1, 6, np.where(touch & 2, 3, np.where(n_cds > 0, _txindel_frame_bin(c_lo, c_hi, n_cds),
                                np.where(touch & 4, 4, np.where(touch & 8, 2, np.where(touch & 16, 0, np.where(touch & 32, 1, 5)))))))
            bins_all[:, c - 1] = bins
        yield i, tx, counted, bins_all


def summary_txindel_host(prob, start, label, n_class, segments, features, n_transcripts, kind, breakpoint_offset=1, class_len=None,
                         chrom_length=None, links=None, into=None):
    """The numpy twin of ``mural_summary_txindel_rows`` -- and its specification -- for INDEL rows (any order) of one chromosome: (table
    uint64 [n_transcripts][10][3], rows uint64 [n_transcripts][2], status).  `segments`, `features`: the chromosome's dicts of
    ``tables.read_transcript_structure`` (or None); `links`: ``tables.structure_links(features)`` (None: built here); `kind`: 0 / 1 / 2 or
    'insertion' / 'deletion_start' / 'deletion_end', of all rows; `class_len`: ``tables.check_indel_lengths``' argument, the inclusive
    lengths lo .. hi of every class c >= 1; `chrom_length`: the chromosome's, or None.  2 <= n_class <= 16.  Class 0's probability, the
    rows' strand and the genome are never read.  The bins (``tables.INDEL_STRUCTURE_BINS``): 0 utr5, 1 utr3, 2 noncoding_exon, 3 splice,
    4 splice_utr, 5 intron, 6 start_lost, 7 frameshift, 8 inframe, 9 cds_mixed.

    The event's boundary is j = start + breakpoint_offset, between bases j - 1 and j; its home base h is j - 1 for an insertion and a
    deletion end, j for a deletion start.  A row counts for every transcript whose span holds h (an insertion: and j), once, through the
    item [a, b) that holds h.  x(j) is the number of CDS bases 5' of boundary j in transcript orientation.  The FRAME BIN of class c
    with n CDS bases affected: 9 where the range lo .. hi holds a multiple of 3 and another length (mixed), 7 for any other range of two
    lengths, and for lo == hi (framed) 7 where n % 3 != 0, else 8.  The CDS RULE at boundary j: x == 0 bin 0, x == cds_length bin 1, x <=
    2 bin 6 for every class, otherwise the frame bin with n = lo.
      Insertion, A the item of base j - 1, B that of base j.  A == B: kinds 0, 1, 2 give bins 0, 1, 2; in a gap of 4 bases or more, j ==
        a + 1 or j == b - 1 splits a splice dinucleotide: bin 3 for kind 3, bin 4 for kind 4; any other gap position is bin 5; a CDS part
        follows the CDS rule.  A != B: a gap yields to an exon part; a CDS part decides by the CDS rule (A first); two other exon parts
        have one kind.
      Deletion: D = [j, j + L) (deletion start) or [j - L, j) (deletion end), L = lo, clipped to the span and to [0, chrom_length) (the
        home base stays).  Over the items that meet D, reached from the home item over the links: n_cds = the CDS bases in D, touch_start
        = a CDS base of offset < 3 is in D, touch_splice = one of the first two or last two bases of a kind-3 gap of 4 bases or more is in
        D, touch_splice_utr = the same for kind 4.  The first that holds: touch_start bin 6, touch_splice bin 3, n_cds > 0 the frame bin
        with n = n_cds, touch_splice_utr bin 4, a kind-2 base bin 2, a kind-0 base bin 0, a kind-1 base bin 1, otherwise bin 5.
    A link that is out of range or names another transcript, and an item that is empty, of an unknown kind, a CDS part without its
    segment or that does not abut the item before it, end the walk; such a home item is skipped, and so is an insertion whose B is one.
    Cell [t][b] += {label == c, hi(p_c), lo(p_c)} per (row, c >= 1) routed to bin b of transcript t; rows[t] += {1, label == 0} per row
    counted.  Integer sums: both tables are a function of the SET of rows, bit for bit; on return lo < 2^40.  `into`: (table, rows) of
    earlier parts and chromosomes to add to, in place.  Status bits: 1 a negative start, 2 a label outside 0 .. n_class - 1, 8 a
    probability of a class >= 1 that is NaN, negative or above 1; such rows are skipped."""
    k = int(n_class)
    if not 2 <= k <= 16:
        raise ValueError(f"the INDEL structure table takes rows of 2 .. 16 classes (got {k})")
    kind, off, cl = check_indel_kind(kind), check_breakpoint_offset(breakpoint_offset), check_indel_lengths(class_len, k)
    n_tx = int(n_transcripts)
    start, label = np.asarray(start, np.int64), np.asarray(label)
    hi, lo, bad_p = kmer_quantise(np.asarray(prob)[:, 1:k])
    lab = np.where(np.isfinite(label.astype(np.float64)), label, -1).astype(np.int64)
    bad_label = (lab < 0) | (lab >= k) | (lab != label)
    bad_start, bad_prob = start < 0, bad_p.any(axis=1)
    status = (1 if bad_start.any() else 0) | (2 if bad_label.any() else 0) | (8 if bad_prob.any() else 0)
    ok = ~(bad_label | bad_start | bad_prob)
    table, rows = (np.zeros((n_tx, TXINDEL_BINS, 3), np.uint64), np.zeros((n_tx, 2), np.uint64)) if into is None else into
    if features is None or len(features["feat_b0"]) == 0 or not ok.any():
        return table, rows, status
    order = np.argsort(start[ok], kind="stable")
    hi, lo, start, lab = hi[ok][order], lo[ok][order], start[ok][order], lab[ok][order]
    flat_table, flat_rows = table.reshape(-1), rows.reshape(-1)
    for i, tx, counted, bins in _txindel_pairs(start, segments, features, links, n_tx, kind, off, cl, chrom_length):
        ic = i[counted]
        for c in range(1, k):
            cell = (tx * (3 * TXINDEL_BINS) + 3 * bins[:, c - 1])[counted]
            np.add.at(flat_table, cell, (lab[ic] == c).astype(np.uint64))
            np.add.at(flat_table, cell + 1, hi[ic, c - 1])
            np.add.at(flat_table, cell + 2, lo[ic, c - 1])
            # (per class: a pass holds up to 2^20 pairs, and 15 classes of them unfolded would bring a cell's lo limb to 2^64)
            _conseq_fold(table)
        np.add.at(flat_rows, 2 * tx[counted], np.uint64(1))
        np.add.at(flat_rows, 2 * tx[counted] + 1, (lab[ic] == 0).astype(np.uint64))
    return table, rows, status


def txindel_rows_device(acc, name, segments, features, links, n_transcripts, kind, breakpoint_offset, class_len, chrom_length, dev, *,
                        prob, prob_f64, prob_stride, start, label, label_kind, n, n_class):
    """One ``mural_summary_txindel_rows`` call on device pointers into the accumulators of `acc` (dict: table int64 [n_transcripts * 30], rows int64 [n_transcripts * 2], status int32 [1], features
    {chromosome: device arrays}, segments {the same}, ws): the chromosome's item, link and segment arrays are uploaded the first time
    it arrives, the workspace grows as needed.  `segments` None: the chromosome has no CDS.  `class_len`: int32 [n_class][2]
    (``tables.check_indel_lengths``); `chrom_length` None: not known."""
    lib = _lib.lib()
    arrays = [features[key] for key in _FEAT_KEYS[:5]] + [np.asarray(x, np.int32) for x in links]
    on_dev = _upload_once(acc["features"], name, arrays, dev)
    seg_dev = _conseq_segments_device(acc, name, features if segments is None else segments, dev)
    s = _lib.MuralSummaryTxindelRows()
    _fill_rows(s, n_class, prob, prob_f64, prob_stride, start, n, label=label, label_kind=label_kind)
    _fill_indel(s, kind, breakpoint_offset, class_len, chrom_length)
    _fill_transcripts(s, n_transcripts, acc["tx"], seg_dev, 4, on_dev)
    s.table, s.rows, s.status = acc["table"].data_ptr(), acc["rows"].data_ptr(), acc["status"].data_ptr()
    ws = _grow_ws(acc, int(lib.mural_summary_txindel_workspace_bytes(int(on_dev[0].shape[0]))), dev)
    _lib.check(lib.mural_summary_txindel_rows(C.byref(s), *ws, _lib.current_stream_ptr(dev)))


# ---- mutation sets drawn from the rates (csrc/simulate.hip: mural_simulate_annot_rows, mural_simulate_rows) -----------------------------
SIMULATE_MAX_REPLICATES = 1 << 20
_PHILOX_M0, _PHILOX_M1 = 0xD2511F53, 0xCD9E8D57
_PHILOX_W0, _PHILOX_W1 = 0x9E3779B9, 0xBB67AE85
_U32 = np.uint64(0xFFFFFFFF)


def simulate_chrom_key(name):
    """The third counter word of a chromosome's draws: crc32 of its name as UTF-8, formed on the host so that every rank has the same."""
    return zlib.crc32(str(name).encode("utf-8")) & 0xFFFFFFFF


def philox4x32_10(counter, key):
    """Philox4x32-10 on arrays: counter uint [..., 4], key uint [..., 2] (broadcast against each other) -> uint32 [..., 4]."""
    c = [np.asarray(counter, np.uint64)[..., j] & _U32 for j in range(4)]
    k = [np.asarray(key, np.uint64)[..., j] & _U32 for j in range(2)]
    for rnd in range(10):
        if rnd:
            k = [(k[0] + np.uint64(_PHILOX_W0)) & _U32, (k[1] + np.uint64(_PHILOX_W1)) & _U32]
        p0, p1 = c[0] * np.uint64(_PHILOX_M0), c[2] * np.uint64(_PHILOX_M1)
        c = [(p1 >> np.uint64(32)) ^ c[1] ^ k[0], p1 & _U32, (p0 >> np.uint64(32)) ^ c[3] ^ k[1], p0 & _U32]
    return np.stack(np.broadcast_arrays(*c), axis=-1).astype(np.uint32)


def simulate_cum_host(prob, start, n_class):
    """(cum uint64 [n][n_class - 1], bad rows, status) of the class rule: q_c = floor(double(p_c) * 2^32) for c >= 1 (the product is
    exact; a p_c of 1 or more gives 2^32 or more and is taken as 2^32, which the clamp below would make of it anyway),
    cum_c = min(q_1 + .. + q_c, 2^32).  Bad rows -- a NaN, negative or infinite p_c (status 8), a negative start (status 1) -- have
    cum = 0: they draw class 0 in every replicate."""
    nc = int(n_class)
    p = np.asarray(prob)[:, 1:nc].astype(np.float64)
    start = np.asarray(start, np.int64)
    bad_p = ~(np.isfinite(p) & ~np.signbit(np.where(p == 0, 0.0, p))).all(axis=1)
    bad_s = start < 0
    one = float(1 << 32)
    with np.errstate(invalid="ignore", over="ignore"):
        q = np.floor(np.minimum(np.where(bad_p[:, None], 0.0, p) * one, one)).astype(np.uint64)
    cum = np.minimum(np.cumsum(q, axis=1, dtype=np.uint64), np.uint64(1 << 32))
    cum[bad_p | bad_s] = 0
    return cum, bad_p | bad_s, (8 if bad_p.any() else 0) | (1 if bad_s.any() else 0)


def simulate_rows_host(prob, start, strand, n_class, chrom_key, seed, reps, with_status=False):
    """The numpy twin of the draw of csrc/simulate.hip -- and its specification: labels uint8 [n][len(reps)], the class of every row in
    every replicate of `reps`.  Generator: Philox4x32-10 with key (seed & 0xffffffff, seed >> 32) and counter (start & 0xffffffff,
    start >> 32, chrom_key, (replicate >> 2) | (strand << 31)), `strand` 1 for '-' (None: all '+'); replicate r reads output word r & 3
    as u.  The label is the smallest c >= 1 with u < cum_c (``simulate_cum_host``), 0 where there is none; class 0's probability is
    never read.  A draw depends on (seed, chromosome, start, strand, replicate) alone -- never on the row's index in a call, so any
    split of the rows into parts draws the same --, and two rows with the same chromosome, start and strand draw the same value."""
    reps = np.asarray(reps, np.int64).reshape(-1)
    if len(reps) and (reps.min() < 0 or reps.max() >= SIMULATE_MAX_REPLICATES):
        raise ValueError(f"replicates are 0 .. {SIMULATE_MAX_REPLICATES - 1}")
    seed = int(seed)
    if not 0 <= seed < 1 << 64:
        raise ValueError("the seed is an unsigned 64-bit integer")
    start = np.asarray(start, np.int64)
    n = len(start)
    cum, _, status = simulate_cum_host(prob, start, n_class)
    minus = np.zeros(n, np.uint64) if strand is None else (np.asarray(strand) != 0).astype(np.uint64)
    s = start.view(np.uint64)
    labels = np.zeros((n, len(reps)), np.uint8)
    key = np.array([seed & 0xFFFFFFFF, seed >> 32], np.uint64)
    for block in np.unique(reps >> 2):
        ctr = np.stack([s & _U32, s >> np.uint64(32), np.full(n, int(chrom_key) & 0xFFFFFFFF, np.uint64),
                        np.uint64(block) | (minus << np.uint64(31))], axis=-1)
        words = philox4x32_10(ctr, key).astype(np.uint64)
        for j in np.nonzero((reps >> 2) == block)[0]:
            u = words[:, reps[j] & 3]
            hit = u[:, None] < cum
            labels[:, j] = np.where(hit.any(axis=1), hit.argmax(axis=1) + 1, 0)
    return (labels, status) if with_status else labels


def simulate_annot_host(prob, start, strand, n_class, chrom_key, seed, pieces, n_groups, n_rep, into=None):
    """The numpy twin of ``mural_simulate_annot_rows``: (table uint32 [n_groups][n_class - 1][n_rep], status).  Cell [g][c - 1][r]: the
    rows inside the pieces of group g (b0 <= start < b1; once per name that covers the row, as ``summary_annot_host``) whose
    replicate-r draw of ``simulate_rows_host`` is class c.  `into`: the table of earlier parts and chromosomes, added to in place."""
    nc, ng, R = int(n_class), int(n_groups), int(n_rep)
    start = np.asarray(start, np.int64)
    labels, status = simulate_rows_host(prob, start, strand, nc, chrom_key, seed, np.arange(R), with_status=True)
    if len(start) > 1 and (start[1:] < start[:-1]).any():
        status |= 4
    table = np.zeros((ng, max(nc - 1, 0), R), np.uint32) if into is None else into
    if pieces is None or len(pieces[0]) == 0 or nc < 2 or R == 0:
        return table, status
    b0, b1, grp = (np.asarray(x) for x in pieces)
    order = np.argsort(start, kind="stable")
    st = start[order]
    prefix = np.zeros((len(st) + 1, nc - 1, R), np.uint32)
    np.cumsum(labels[order][:, None, :] == np.arange(1, nc, dtype=np.uint8)[None, :, None], axis=0, dtype=np.uint32, out=prefix[1:])
    i0 = np.searchsorted(st, b0, "left")
    i1 = np.maximum(np.searchsorted(st, b1, "left"), i0)
    live = np.nonzero((i1 > i0) & (grp >= 0) & (grp < ng))[0]
    np.add.at(table, grp[live], prefix[i1[live]] - prefix[i0[live]])
    return table, status


def simulate_conseq_host(genome, prob, start, strand, segments, n_transcripts, chrom_key, seed, n_rep, aa=None, alt_order=None, into=None):
    """The numpy twin of ``mural_simulate_conseq_rows`` -- and its specification -- for SNV rows (4 classes; no label is read) of one
    chromosome: (table uint32 [n_transcripts][5][n_rep], status).  Cell [t][b][r]: the rows inside the CDS of transcript t whose
    replicate-r draw is a class c >= 1 whose substitution c falls in bin b of t.  The draw is ``simulate_rows_host``'s, unchanged
    (Philox key and counter, cum, ties); the bin is ``summary_conseq_host``'s rule (0 syn, 1 mis, 2 stop gained, 3 stop lost, 4
    unresolved; `segments`, `aa`, `alt_order` and `strand` as there).  A row counts once per transcript that covers it; class 0 counts
    nowhere.  The row checks are the simulation's: a NaN, negative or infinite p_c of a class c >= 1 sets status 8, a negative start
    status 1 -- such rows draw class 0 in every replicate --, a start below the row before it status 4; p_c >= 1 is taken as 1 and is
    no error here.  The table is a function of the SET of rows and the seed alone, bit for bit, for any parts, shards or ranks.
    `into`: the table of earlier parts and chromosomes, added to in place.

    THE DEFINING IDENTITY.  For rows that both rules accept (finite p in [0, 1], start >= 0), cell [t][b][r] equals cell [t][b][0] --
    the observed count -- of ``summary_conseq_host`` run with label = ``simulate_rows_host(..)[:, r]``: two specifications with
    independent oracles, composed, are the oracle of this one."""
    from .tables import check_alt_order, check_codon_table
    n_tx, R = int(n_transcripts), int(n_rep)
    if not 1 <= R <= SIMULATE_MAX_REPLICATES:
        raise ValueError("simulate: 1 .. 2^20 replicates")
    aa = check_codon_table(aa).astype(np.int64)
    alt_of = check_alt_order(alt_order).astype(np.int64)
    start = np.asarray(start, np.int64)
    labels, status = simulate_rows_host(prob, start, strand, 4, chrom_key, seed, np.arange(R), with_status=True)
    if len(start) > 1 and (start[1:] < start[:-1]).any():
        status |= 4
    table = np.zeros((n_tx, 5, R), np.uint32) if into is None else into
    if segments is None or len(segments["seg_b0"]) == 0 or len(start) == 0:
        return table, status
    rs = np.zeros(len(start), np.int64) if strand is None else strand_u8(strand).astype(np.int64)
    order = np.argsort(start, kind="stable")
    start, labels, rs = start[order], labels[order], rs[order]
    flat = table.reshape(-1, R)
    for i, tx, bins in _conseq_pairs(genome, start, rs, segments, aa, alt_of):
        lab = labels[i].astype(np.int64)                                                 # [pairs][R]
        lb = np.take_along_axis(bins, np.maximum(lab - 1, 0), axis=1)                    # the bin of the drawn class
        for b in range(5):
            hit = ((lab > 0) & (lb == b)).astype(np.uint32)
            np.add.at(flat, tx * 5 + b, hit)
    return table, status


def _fill_draw(s, name, n_rep, seed, table, status):
    s.chrom_key, s.n_rep, s.seed = simulate_chrom_key(name), int(n_rep), int(seed)
    s.table, s.status = table.data_ptr(), status.data_ptr()


def simulate_conseq_rows_device(table, status, acc, name, n_transcripts, aa, alt_order, genome_struct, dev, n_rep, seed, *, prob, prob_f64,
                                prob_stride, start, strand, n):
    """One ``mural_simulate_conseq_rows`` call on device pointers into `table`
    (int32 [n_transcripts * 5 * n_rep]) and `status`, on the segment arrays ``conseq_rows_device`` uploaded into `acc` for chromosome
    `name` just before; the workspace is `acc`'s (24 bytes a segment in both entries)."""
    lib = _lib.lib()
    on_dev = acc["segments"][name]
    s = _lib.MuralSimulateConseqRows()
    _fill_rows(s, 4, prob, prob_f64, prob_stride, start, n, strand)
    _fill_draw(s, name, n_rep, seed, table, status)
    _fill_transcripts(s, n_transcripts, acc["tx"], on_dev, 6, codons=(aa, alt_order, genome_struct))
    ws = _grow_ws(acc, int(lib.mural_simulate_conseq_workspace_bytes(int(on_dev[0].shape[0]))), dev)
    _lib.check(lib.mural_simulate_conseq_rows(C.byref(s), *ws, _lib.current_stream_ptr(dev)))


def simulate_txstruct_host(genome, prob, start, strand, segments, features, n_transcripts, chrom_key, seed, n_rep, aa=None, alt_order=None,
                           into=None):
    """The numpy twin of ``mural_simulate_txstruct_rows`` -- and its specification -- for SNV rows (4 classes; no label is read) of one
    chromosome: (table uint32 [n_transcripts][9][n_rep], status).  Cell [t][b][r]: the rows inside [chromStart, chromEnd) of transcript
    t whose replicate-r draw is a class c >= 1 that falls in structure bin b of t.  The draw is ``simulate_rows_host``'s, unchanged
    (Philox key and counter, cum, ties, p_c >= 1 taken as 1); the bin is ``summary_txstruct_host``'s rule through the same item walk
    (``_txstruct_pairs``; `segments`, `features`, `aa`, `alt_order` and `strand` as there).  A row counts once per transcript whose
    span covers it; class 0 counts nowhere.  The row checks are the simulation's, as ``simulate_conseq_host``: status 8 a NaN, negative
    or infinite p_c, status 1 a negative start -- such rows draw class 0 in every replicate --, status 4 a start below the row before
    it.  The table is a function of the SET of rows and the seed alone, bit for bit, for any parts, shards or ranks.  `into`: the table
    of earlier parts and chromosomes, added to in place.

    THE DEFINING IDENTITIES.  (a) For rows that both rules accept, cell [t][b][r] equals the observed word [t][b][0] of
    ``summary_txstruct_host`` run with label = ``simulate_rows_host(..)[:, r]``.  (b) For every t and r, bins 7 + 8 add up to the five
    bins of ``simulate_conseq_host``'s table at the same key, seed and replicate.  (c) ``simulate_lof_counts`` of that table and this
    one is the observed_lof of ``tables.write_structure_outputs`` for a run labelled with replicate r."""
    from .tables import check_alt_order, check_codon_table
    n_tx, R = int(n_transcripts), int(n_rep)
    if not 1 <= R <= SIMULATE_MAX_REPLICATES:
        raise ValueError("simulate: 1 .. 2^20 replicates")
    aa = check_codon_table(aa).astype(np.int64)
    alt_of = check_alt_order(alt_order).astype(np.int64)
    start = np.asarray(start, np.int64)
    labels, status = simulate_rows_host(prob, start, strand, 4, chrom_key, seed, np.arange(R), with_status=True)
    if len(start) > 1 and (start[1:] < start[:-1]).any():
        status |= 4
    table = np.zeros((n_tx, TX_BINS, R), np.uint32) if into is None else into
    if features is None or len(features["feat_b0"]) == 0 or len(start) == 0:
        return table, status
    rs = np.zeros(len(start), np.int64) if strand is None else strand_u8(strand).astype(np.int64)
    order = np.argsort(start, kind="stable")
    start, labels, rs = start[order], labels[order], rs[order]
    flat = table.reshape(-1, R)
    for i, tx, bins in _txstruct_pairs(genome, start, rs, segments, features, aa, alt_of):
        lab = labels[i].astype(np.int64)                                                 # [pairs][R]
        lb = np.take_along_axis(bins, np.maximum(lab - 1, 0), axis=1)                    # the bin of the drawn class
        for b in np.unique(bins):
            hit = ((lab > 0) & (lb == b)).astype(np.uint32)
            np.add.at(flat, tx * TX_BINS + b, hit)
    return table, status


def simulate_lof_counts(conseq_counts, struct_counts):
    """lof int64 [transcripts][R] of the simulated loss-of-function count: stop gained (bin 2 of ``simulate_conseq_host``'s table
    [transcripts][5][R]) + splice donor + splice acceptor + start lost (bins 3, 4, 7 of ``simulate_txstruct_host``'s table
    [transcripts][9][R]) of the SAME draws -- the four terms by which ``tables.write_structure_outputs`` forms observed_lof."""
    conseq_counts, struct_counts = np.asarray(conseq_counts), np.asarray(struct_counts)
    if conseq_counts.ndim != 3 or struct_counts.ndim != 3 or conseq_counts.shape[1] != 5 or struct_counts.shape[1] != TX_BINS or \
            conseq_counts.shape[::2] != struct_counts.shape[::2]:
        raise ValueError("simulate_lof_counts: counts [transcripts][5][R] and [transcripts][9][R] of the same transcripts and replicates")
    lof = conseq_counts[:, 2].astype(np.int64)
    for term in (struct_counts[:, 3], struct_counts[:, 4], struct_counts[:, 7]):
        lof += term
    return lof


def simulate_txstruct_rows_device(table, status, acc, conseq_acc, name, n_transcripts, aa, alt_order, genome_struct, dev, n_rep, seed, *,
                                  prob, prob_f64, prob_stride, start, strand, n):
    """One ``mural_simulate_txstruct_rows`` call on device pointers into `table` (int32
    [n_transcripts * 9 * n_rep]) and `status`, on the item arrays ``txstruct_rows_device`` uploaded into `acc` for chromosome `name`
    just before and the segment arrays of `conseq_acc`; the workspace is `acc`'s (24 bytes an item in both entries)."""
    lib = _lib.lib()
    on_dev = acc["features"][name]
    s = _lib.MuralSimulateTxstructRows()
    _fill_rows(s, 4, prob, prob_f64, prob_stride, start, n, strand)
    _fill_draw(s, name, n_rep, seed, table, status)
    _fill_transcripts(s, n_transcripts, conseq_acc["tx"], conseq_acc["segments"].get(name), 6, on_dev, codons=(aa, alt_order, genome_struct))
    ws = _grow_ws(acc, int(lib.mural_simulate_txstruct_workspace_bytes(int(on_dev[0].shape[0]))), dev)
    _lib.check(lib.mural_simulate_txstruct_rows(C.byref(s), *ws, _lib.current_stream_ptr(dev)))


def simulate_txindel_host(prob, start, strand, n_class, segments, features, n_transcripts, kind, chrom_key, seed, n_rep,
                          breakpoint_offset=1, class_len=None, chrom_length=None, links=None, into=None):
    """The numpy twin of ``mural_simulate_txindel_rows`` -- and its specification -- for INDEL rows (any order; no label is read) of one
    chromosome: (counts uint32 [n_transcripts][10][n_rep], status).  Cell [t][b][r]: the rows that transcript t counts whose
    replicate-r draw is a class c >= 1 with bin(row, t, c) == b; class 0 counts nowhere.  2 <= n_class <= 8, the bound of the
    simulation's draw (``SIM_MAX_CLASS`` of csrc/simulate_draw.h).

    DRAW.  ``simulate_rows_host``'s, unchanged: the Philox key (seed) and counter (start, chrom_key, replicate >> 2, the strand bit),
    cum, ties, p_c >= 1 taken as 1.  A row with a NaN, negative or infinite p_c (status 8) or a negative start (status 1) draws class 0
    in every replicate; a start below the row before it sets status 4.  A draw depends on (seed, chromosome, start, strand, replicate)
    alone, so two rows with equal chromosome, start and strand -- two events recorded at one position -- draw the SAME value, as
    DESIGN.md section 3.20 documents for every simulation here: their counts move together, they are not independent.
    BIN.  ``summary_txindel_host``'s, unchanged, through the same item walk (``_txindel_pairs``): the home base by `kind` and
    `breakpoint_offset`, the insertion on one item or on the boundary of two, the deletion's walk located by L = lo(c), the clipping
    by `chrom_length`, what ends a walk, skipped home items; `segments`, `features`, `links`, `class_len` as there.  "Counted" is that
    rule's as well: once per transcript whose span holds the home base (an insertion: and base j).
    The table is a function of the SET of rows and the seed alone, bit for bit, for any parts, shards or ranks.  `into`: the table of
    earlier parts and chromosomes, added to in place.

    THE DEFINING IDENTITIES.  (a) For rows that both rules accept (finite p in [0, 1], start >= 0), cell [t][b][r] equals the observed
    word [t][b][0] of ``summary_txindel_host`` run with label = ``simulate_rows_host(..)[:, r]``.  (b) ``simulate_indel_lof_counts`` of
    this table gives, per replicate r, the observed_lof / observed_lof_upper of ``tables.write_indel_structure_outputs`` for a run
    labelled with replicate r.  (c) Any split of the rows into parts, any permutation of rows with equal starts and any number of
    ranks give the same bytes."""
    k = int(n_class)
    if not 2 <= k <= 8:
        raise ValueError(f"simulate: the INDEL structure simulation takes rows of 2 .. 8 classes, the bound of the draw (SIM_MAX_CLASS = 8; "
                         f"got {k})")
    n_tx, R = int(n_transcripts), int(n_rep)
    if not 1 <= R <= SIMULATE_MAX_REPLICATES:
        raise ValueError("simulate: 1 .. 2^20 replicates")
    kind, off, cl = check_indel_kind(kind), check_breakpoint_offset(breakpoint_offset), check_indel_lengths(class_len, k)
    start = np.asarray(start, np.int64)
    labels, status = simulate_rows_host(prob, start, strand, k, chrom_key, seed, np.arange(R), with_status=True)
    if len(start) > 1 and (start[1:] < start[:-1]).any():
        status |= 4
    table = np.zeros((n_tx, TXINDEL_BINS, R), np.uint32) if into is None else into
    if features is None or len(features["feat_b0"]) == 0 or len(start) == 0:
        return table, status
    order = np.argsort(start, kind="stable")
    start, labels = start[order], labels[order]
    flat = table.reshape(-1, R)
    for i, tx, counted, bins in _txindel_pairs(start, segments, features, links, n_tx, kind, off, cl, chrom_length):
        i, tx, bins = i[counted], tx[counted], bins[counted]
        lab = labels[i].astype(np.int64)                                                 # [pairs][R]
        lb = np.take_along_axis(bins, np.maximum(lab - 1, 0), axis=1)                    # the bin of the drawn class
        for b in np.unique(bins):
            hit = ((lab > 0) & (lb == b)).astype(np.uint32)
            np.add.at(flat, tx * TXINDEL_BINS + b, hit)
    return table, status


def simulate_indel_lof_counts(counts):
    """(lof, lof_upper) int64 [transcripts][R] of the simulated INDEL loss-of-function count from ``simulate_txindel_host``'s table
    [transcripts][10][R]: lof = splice + start_lost + frameshift (bins 3 + 6 + 7) of the SAME draws, lof_upper = lof + cds_mixed (bin
    9) -- the terms by which ``tables._indel_lof_cells`` forms observed_lof / observed_lof_upper."""
    counts = np.asarray(counts)
    if counts.ndim != 3 or counts.shape[1] != TXINDEL_BINS:
        raise ValueError("simulate_indel_lof_counts: counts [transcripts][10][R]")
    lof = counts[:, 3].astype(np.int64) + counts[:, 6] + counts[:, 7]
    return lof, lof + counts[:, 9]


def simulate_txindel_rows_device(table, status, acc, name, n_transcripts, kind, breakpoint_offset, class_len, chrom_length, dev, n_rep,
                                 seed, *, prob, prob_f64, prob_stride, start, strand, n, n_class):
    """One ``mural_simulate_txindel_rows`` call on device pointers into `table` (int32
    [n_transcripts * 10 * n_rep]) and `status`, on the item, link and segment arrays ``txindel_rows_device`` uploaded into `acc` for
    chromosome `name` just before; the workspace is `acc`'s (24 bytes an item in both entries)."""
    lib = _lib.lib()
    on_dev = acc["features"][name]
    s = _lib.MuralSimulateTxindelRows()
    _fill_rows(s, n_class, prob, prob_f64, prob_stride, start, n, strand)
    _fill_draw(s, name, n_rep, seed, table, status)
    _fill_indel(s, kind, breakpoint_offset, class_len, chrom_length)
    _fill_transcripts(s, n_transcripts, acc["tx"], acc["segments"].get(name), 4, on_dev)
    ws = _grow_ws(acc, int(lib.mural_simulate_txindel_workspace_bytes(int(on_dev[0].shape[0]))), dev)
    _lib.check(lib.mural_simulate_txindel_rows(C.byref(s), *ws, _lib.current_stream_ptr(dev)))


def simulate_pvalues(counts, observed=None):
    """Per row of `counts` int [m][R] (the simulated counts of a name and class): (sim_mean, sim_min, sim_max, n_ge, n_le, p_upper,
    p_lower), the last four None without `observed` [m]: n_ge / n_le the replicates with a count at least / at most the observed one,
    p_upper = (n_ge + 1) / (R + 1), p_lower = (n_le + 1) / (R + 1)."""
    counts = np.asarray(counts, np.int64)
    R = counts.shape[1]
    out = []
    for j, row in enumerate(counts):
        total = int(row.sum())
        head = (total / R, int(row.min()), int(row.max()))
        if observed is None:
            out.append(head + (None,) * 4)
        else:
            n_ge, n_le = int((row >= int(observed[j])).sum()), int((row <= int(observed[j])).sum())
            out.append(head + (n_ge, n_le, (n_ge + 1) / (R + 1), (n_le + 1) / (R + 1)))
    return out


# ---- loss and calibration metrics (csrc/summary_calib.hip: mural_summary_calib_rows): integer sums behind NLL / ECE / CwECE / Brier ----
# Scaling of the two-limb sums: a term v >= 0 is quantised once to rne(v * 2^(S + 46)), hi = floor(v * 2^S), lo = rint((v * 2^S - hi) *
# 2^46), every step exact in float64; S = 16 for the scores (in [0, 1]) and the Brier terms (in [0, 2]) -- a row's error at most 2^-63
# --, S = 13 for the NLL terms (below 2^10: -log of the smallest positive double is 744.5) -- at most 2^-60.  A folded pair has
# lo < 2^46; hi grows by at most 2^23 a row plus the carries, so 2^40 rows stay below 2^64.
_CALIB_LO_BITS, _CALIB_SCORE_BITS, _CALIB_NLL_BITS = 46, 16, 13
_CALIB_LO_MASK = np.uint64((1 << _CALIB_LO_BITS) - 1)
_CALIB_FOLD_ROWS = 1 << 17         # rows between two folds here: lo < 2^46 + 2^17 * 2^46 < 2^64
_CALIB_MAX_CELLS = 4096            # the table a workgroup of csrc/summary_calib.hip holds


def calib_cells(n_class, n_bins):
    """Cells of the table of ``mural_summary_calib_rows``: 6 + n_class header cells and 4 per bin of the n_class + 1 groups."""
    return 6 + int(n_class) + 4 * int(n_bins) * (int(n_class) + 1)


def calib_bounds(n_bins):
    """The reference's bin bounds: float32 ``torch.linspace(0, 1, n_bins + 1)`` (evaluation.py:218)."""
    return torch.linspace(0, 1, int(n_bins) + 1).numpy()


def _calib_lo_cells(n_class, n_bins):
    h = 6 + n_class
    return np.r_[3 + n_class, 5 + n_class, h + 2 + 4 * np.arange(n_bins * (n_class + 1))].astype(np.int64)


def _calib_fold(table, n_class, n_bins):
    """Carry the lo limbs' overflow into the hi limbs in front of them: table uint64 [cells], in place."""
    lo = _calib_lo_cells(n_class, n_bins)
    table[lo - 1] += table[lo] >> np.uint64(_CALIB_LO_BITS)
    table[lo] &= _CALIB_LO_MASK
    return table


def _calib_quantise(v, bits):
    """(hi, lo) uint64 of float64 terms v >= 0 (the rule above)."""
    v = np.where(v > 0.0, v, 0.0)
    s = v * float(1 << bits)
    h = np.floor(s)
    return h.astype(np.uint64), np.rint((s - h) * float(1 << _CALIB_LO_BITS)).astype(np.uint64)


def summary_calib_host(prob, label, n_class, n_bins=50, bounds=None, into=None):
    """The numpy twin of ``mural_summary_calib_rows`` -- and its specification -- for rows in any order: (table uint64 [6 + n_class +
    4 n_bins (n_class + 1)], status).  Per row, in the probabilities' own precision (float32 or float64; anything else is taken as
    float32): q = softmax(log(prob)), summed over the classes in ascending order; confidence = max q, the prediction its first maximum;
    Brier term = sum_c ([c == label] - q_c)^2, the squares widened to float64 and added in class order; NLL term = -log q_label; bins
    (lower, upper] on `bounds` (default ``calib_bounds(n_bins)``), compared in float64.  Cells, H = 6 + n_class:
      [0] rows  [1] inf_rows  [2 + c] rows with label c  [2 + nc], [3 + nc] NLL hi, lo  [4 + nc], [5 + nc] Brier hi, lo
      [H + 4 (g n_bins + b) + 0 .. 3] rows, score hi, score lo, hits of bin b of group g: g = 0 the top-label bins (score = confidence,
      hit = the prediction is the label), g = 1 + c class c (score = q_c, hit = the label is c); a score in no bin (0) adds nowhere.
    The real-valued sums are the two-limb integers described above this function, so the table depends on the SET of valid rows alone,
    bit for bit.  `into`: the table of earlier parts to add to (in place).  Status bits as on the device: 2 a label outside
    0 .. n_class - 1 (or no whole number), 8 a probability that is NaN, negative or above 1 -- or a row without a positive probability,
    whose softmax is undefined; such rows are skipped everywhere.  A valid row with q_label == 0 counts in inf_rows and everywhere but
    the NLL sum.

    Device and twin agree EXACTLY in what no transcendental's last bit decides: rows, label counts, status, inf_rows for exact zeros.
    The score sums and the bin a score falls in go through ``log`` and ``exp`` of two math libraries: they are compared through the
    derived metrics (``calib_metrics_from_sums``), not bit for bit."""
    nc, nb = int(n_class), int(n_bins)
    prob = np.asarray(prob)[:, :nc]
    if prob.dtype not in (np.float32, np.float64):
        prob = prob.astype(np.float32)
    P = prob.dtype.type
    bounds = (calib_bounds(nb) if bounds is None else np.asarray(bounds, np.float32)).astype(np.float64)
    if len(bounds) != nb + 1:
        raise ValueError(f"{nb} bins need {nb + 1} bounds")
    table = np.zeros(calib_cells(nc, nb), np.uint64) if into is None else into
    label = np.asarray(label)
    lab = np.where(np.isfinite(label.astype(np.float64)), label, -1).astype(np.int64)
    bad_label = (lab < 0) | (lab >= nc) | (lab != label)
    with np.errstate(invalid="ignore"):
        bad_prob = ~((prob >= 0) & (prob <= 1)).all(axis=1) | ~(prob > 0).any(axis=1)
    status = (2 if bad_label.any() else 0) | (8 if bad_prob.any() else 0)
    ok = ~(bad_label | bad_prob)
    prob, lab = prob[ok], lab[ok]
    H = 6 + nc
    for r0 in range(0, len(lab), _CALIB_FOLD_ROWS):
        p, y = prob[r0:r0 + _CALIB_FOLD_ROWS], lab[r0:r0 + _CALIB_FOLD_ROWS]
        rows = np.arange(len(y))
        with np.errstate(divide="ignore"):
            lg = np.log(p)
        e = np.exp(lg - lg.max(axis=1, keepdims=True))
        s = np.zeros(len(y), P)
        for c in range(nc):
            s = s + e[:, c]
        q = e / s[:, None]
        conf, arg = q.max(axis=1), q.argmax(axis=1)
        brier = np.zeros(len(y))
        for c in range(nc):
            d = (y == c).astype(P) - q[:, c]
            brier = brier + (d * d).astype(np.float64)
        q_lab = q[rows, y]
        inf = ~(q_lab > 0)
        table[0] += np.uint64(len(y))
        table[1] += np.uint64(int(inf.sum()))
        table[2:2 + nc] += np.bincount(y, minlength=nc).astype(np.uint64)
        hi, lo = _calib_quantise(-np.log(q_lab[~inf]).astype(np.float64), _CALIB_NLL_BITS)
        table[2 + nc] += hi.sum(dtype=np.uint64)
        table[3 + nc] += lo.sum(dtype=np.uint64)
        hi, lo = _calib_quantise(brier, _CALIB_SCORE_BITS)
        table[4 + nc] += hi.sum(dtype=np.uint64)
        table[5 + nc] += lo.sum(dtype=np.uint64)
        for g in range(nc + 1):
            v = (conf if g == 0 else q[:, g - 1]).astype(np.float64)
            hit = (arg == y) if g == 0 else (y == g - 1)
            b = np.searchsorted(bounds, v, side="left") - 1      # bounds[b] < v <= bounds[b + 1]
            live = (b >= 0) & (b < nb)
            cell = H + 4 * (g * nb + b[live])
            hi, lo = _calib_quantise(v[live], _CALIB_SCORE_BITS)
            np.add.at(table, cell, np.uint64(1))
            np.add.at(table, cell + 1, hi)
            np.add.at(table, cell + 2, lo)
            np.add.at(table, cell + 3, hit[live].astype(np.uint64))
        _calib_fold(table, nc, nb)
    return table, status


def calib_rows_device(prob, label, n_class, n_bins, bounds, table, status):
    """One call of ``mural_summary_calib_rows`` on the current stream of `prob`'s device: prob (n, >= n_class) float32 / float64 with unit
    column stride, label (n,) float32 / int32 / int64, bounds float32 [n_bins + 1], table int64 [calib_cells] and status int32 [1] -- all
    device tensors; table and status are added to."""
    s = _lib.MuralSummaryCalibRows()
    s.prob, s.prob_f64, s.prob_stride = prob.data_ptr(), int(prob.dtype == torch.float64), prob.stride(0) if prob.shape[0] > 1 else prob.shape[1]
    s.label, s.label_kind = label.data_ptr(), _LABEL_KIND[label.dtype]
    s.n, s.n_class, s.n_bins = prob.shape[0], int(n_class), int(n_bins)
    s.bounds, s.table, s.status = bounds.data_ptr(), table.data_ptr(), status.data_ptr()
    with torch.cuda.device(prob.device):
        _lib.check(_lib.lib().mural_summary_calib_rows(C.byref(s), _lib.current_stream_ptr(prob.device)))


def calib_metrics_from_sums(tables, n_bins, n_class):
    """{"rows", "nll", "ece", "c_ece", "brier", "label_counts"} from the integer table of ``summary_calib_host`` /
    ``mural_summary_calib_rows``, formed from Python integers (true division rounds correctly): nll = NLL sum / rows (inf where a row
    had q_label == 0, as the reference's mean would be), brier = Brier sum / rows, ece = sum over the top-label bins of
    |score sum / rows_b - hits_b / rows_b| * rows_b / rows -- which is |score sum - hits_b| / rows, summed exactly --, c_ece the mean of
    the same over the bins of class c for c < (the highest label seen) + 1: the reference's ClasswiseECELoss sizes itself by
    max(labels) + 1.  NaN where there is no row."""
    nc, nb = int(n_class), int(n_bins)
    t = np.asarray(tables).astype(np.uint64).tolist()
    rows, inf_rows, counts = t[0], t[1], t[2:2 + nc]
    out = {"rows": rows, "label_counts": counts}
    if rows == 0:
        return dict(out, nll=float("nan"), ece=float("nan"), c_ece=float("nan"), brier=float("nan"))
    pair = lambda at: (t[at] << _CALIB_LO_BITS) + t[at + 1]      # noqa: E731
    one = 1 << (_CALIB_SCORE_BITS + _CALIB_LO_BITS)
    H = 6 + nc

    def gap(g):
        """sum over the bins of group g of |score sum - hits|, in units of 2^-62"""
        return sum(abs(pair(at + 1) - t[at + 3] * one) for at in range(H + 4 * g * nb, H + 4 * (g + 1) * nb, 4) if t[at])

    n_seen = max(c for c in range(nc) if counts[c]) + 1
    out["nll"] = float("inf") if inf_rows else pair(2 + nc) / (rows << (_CALIB_NLL_BITS + _CALIB_LO_BITS))
    out["brier"] = pair(4 + nc) / (rows * one)
    out["ece"] = gap(0) / (rows * one)
    out["c_ece"] = sum(gap(1 + c) for c in range(n_seen)) / (n_seen * rows * one)
    return out


def _merge_window_table(have, bin0, table):
    """(bin0, table) of a chromosome's windows so far + one part's: the covering table, the part added behind what was there."""
    if have is None or have[1].shape[0] == 0:
        return bin0, table.copy()
    if table.shape[0] == 0:
        return have
    b0, t = have
    lo, hi = min(b0, bin0), max(b0 + t.shape[0], bin0 + table.shape[0])
    if lo != b0 or hi != b0 + t.shape[0]:
        grown = np.zeros((hi - lo, t.shape[1]))
        grown[b0 - lo:b0 - lo + t.shape[0]] = t
        b0, t = lo, grown
    t[bin0 - b0:bin0 - b0 + table.shape[0]] += table
    return b0, t


# ------------------------------------------------------------------------------------------------------------------
# One reducer per summary kind, and SummarySink over them.  A reducer is a plain class with a `name` (its key in a rank's state) and
#   host_part / device_part(name, prob, start, end, strand, label, k)   reduce a part of host rows -> status bits / enqueue the same for
#                                                   device columns -> what must outlive the part.  The columns are calibrated and ascend in
#                                                   start; `strand` is None unless k-mers are reduced
#   read_back(k) -> (state, status bits)            once, at close(): the picklable state of this rank
#   merge(states, k) -> state                       the ranks' states, in rank order
#   finish(state, k, result)                        the entries of result() (and the reducer's own sums)
#   write(out_prefix, result, k, written)           the files; a path goes to `written` before it is created
#   reset()                                         drop everything (abort())
# ------------------------------------------------------------------------------------------------------------------
def _calls_of(items):
    """`items` in the groups of 4 (MURAL_SUMMARY_MAX_WINDOWS, MURAL_SUMMARY_MAX_KMERS) that one call of an entry point takes; one call
    even for none (the totals of the window reduction)."""
    return [items[at:at + 4] for at in range(0, max(len(items), 1), 4)]


def _row_fields(s, prob, start, end, label):
    """The fields every ``MuralSummary*Rows`` struct has for the rows of a part (device tensors)."""
    s.prob, s.prob_f64, s.prob_stride = prob.data_ptr(), int(prob.dtype == torch.float64), prob.stride(0)
    s.start, s.end, s.label, s.label_kind = start.data_ptr(), end.data_ptr(), label.data_ptr(), _LABEL_KIND[label.dtype]
    s.n = start.shape[0]


class _WindowReducer:
    """The window tables per chromosome and window size, prob_sum and n_sites (counted per overlapping benchmark region where there are
    regions).  A device part is reduced one part late: its first and last start size its tables, and they are read back while the next
    part is computed.  The tables are float64 sums: parts are added in arrival order, ranks in rank order."""
    name = "windows"

    def __init__(self, sizes, benchmark_regions, ratio_cutoff):
        self.sizes = tuple(int(w) for w in sizes)
        if any(w <= 0 for w in self.sizes) or len(set(self.sizes)) != len(self.sizes):
            raise ValueError(f"window sizes must be positive and distinct (got {self.sizes})")
        if isinstance(benchmark_regions, (str, os.PathLike)):
            benchmark_regions = read_regions(benchmark_regions)
        self.regions = None if benchmark_regions is None else {
            c: (np.sort(np.asarray(a, np.int64)), np.sort(np.asarray(b, np.int64))) for c, (a, b) in benchmark_regions.items()}
        self.ratio_cutoff = ratio_cutoff
        self.reset()

    def reset(self):
        self.tables = {}               # chromosome -> {W: (bin0, table)}
        self.prob_sum, self.n_sites, self.status = 0.0, 0, 0
        self.pending = None            # a staged device part: reduced when the next one arrives (or at close)
        self.inflight = []             # [(event, pinned result, chromosome, n_class, [(W, bin0, bins, offset)])] of launched parts
        self.dev_regions = {}

    def _take(self, name, tables, total, n_sites):
        mine = self.tables.setdefault(name, {})
        for W, (bin0, t) in tables.items():
            mine[W] = _merge_window_table(mine.get(W), bin0, t)
        self.prob_sum += total
        self.n_sites += n_sites

    def host_part(self, name, prob, start, end, strand, label, k):
        regs = None if self.regions is None else self.regions.get(name, (np.zeros(0, np.int64),) * 2)
        *sums, status = summary_rows_host(prob, start, end, label, k, self.sizes, regs)
        self._take(name, *sums)
        return status

    def device_part(self, name, prob, start, end, strand, label, k, held=None):
        """Stage the part -- the read-back of its first and last start goes behind what the other reducers enqueued for it -- and launch
        the part staged before it, complete by now.  The staged part keeps its columns and `held` (the packed genome of the keyed
        reductions) alive until its own reduction has run."""
        staged = None
        if start.shape[0]:
            dev = prob.device
            with torch.cuda.device(dev):
                ends = torch.empty(2, dtype=torch.int64).pin_memory()
                ends.copy_(torch.stack([start[0], start[-1]]), non_blocking=True)
                ev = torch.cuda.Event()
                ev.record()
            staged = dict(name=name, prob=prob, start=start, end=end, label=label, k=k, ends=ends, event=ev, dev=dev, strand=strand,
                          genome=held)
        self._launch_pending()
        self.pending = staged

    def _launch_pending(self):
        """Reduce the staged part: its first and last start (read back by now) size the part's window tables."""
        p, self.pending = self.pending, None
        if p is None:
            return
        lib = _lib.lib()
        p["event"].synchronize()
        self._harvest(done_only=True)                      # (every part launched before is complete by now: same stream)
        dev, k, n = p["dev"], p["k"], p["start"].shape[0]
        lo = max(int(p["ends"][0]), 0)
        hi = max(int(p["ends"][1]), lo)
        stride = 1 + 2 * k
        layout, off = [], 3
        for W in self.sizes:
            bin0, bins = lo // W, hi // W - lo // W + 1
            if bins * stride >= 2 ** 31:
                raise ValueError(f"the rows of one part span {bins} windows of {W} bp: too many for one table")
            layout.append((W, bin0, bins, off))
            off += bins * stride
        with torch.cuda.device(dev):
            out = torch.zeros(off, dtype=torch.float64, device=dev)      # total | n_sites (int64) | status (int32) | the tables
            regs = None
            if self.regions is not None:
                regs = self.dev_regions.get((p["name"], dev))
                if regs is None:
                    b0, b1 = self.regions.get(p["name"], (np.zeros(0, np.int64),) * 2)
                    regs = (torch.from_numpy(np.r_[b0, 0]).to(dev), torch.from_numpy(np.r_[b1, 0]).to(dev), len(b0))
                    self.dev_regions = {(p["name"], dev): regs}
            stream = _lib.current_stream_ptr(dev)
            for g, group in enumerate(_calls_of(layout)):      # the totals (and the benchmark regions) go with the first call
                s = _lib.MuralSummaryRows()
                _row_fields(s, p["prob"], p["start"], p["end"], p["label"])
                s.n_class, s.n_windows = k, len(group)
                for j, (W, bin0, bins, o) in enumerate(group):
                    s.window[j], s.bin0[j], s.n_bins[j], s.table[j] = W, bin0, bins, out[o:].data_ptr()
                if regs is not None and g == 0:
                    s.reg_b0, s.reg_b1, s.n_reg = regs[0].data_ptr(), regs[1].data_ptr(), regs[2]
                # the totals of a later group of window sizes go to a scratch cell: they are counted once
                tot = out if g == 0 else torch.zeros(2, dtype=torch.float64, device=dev)
                s.total, s.n_sites, s.status = tot.data_ptr(), tot[1:].data_ptr(), out[2:].data_ptr()
                ws = torch.empty(int(lib.mural_summary_workspace_bytes(n, k, len(group))) // 8 + 1, dtype=torch.int64, device=dev)
                _lib.check(lib.mural_summary_rows(C.byref(s), ws.data_ptr(), ws.numel() * 8, stream))
            host = torch.empty(off, dtype=torch.float64).pin_memory()
            host.copy_(out, non_blocking=True)
            ev = torch.cuda.Event()
            ev.record()
        self.inflight.append((ev, host, p["name"], k, layout))

    def _harvest(self, done_only=False):
        keep = []
        for item in self.inflight:
            ev, host, name, k, layout = item
            if done_only and (keep or not ev.query()):      # (in arrival order: nothing overtakes an unfinished part)
                keep.append(item)
                continue
            ev.synchronize()
            a = host.numpy()
            stride = 1 + 2 * k
            tables = {W: (bin0, a[o:o + bins * stride].reshape(bins, stride)) for W, bin0, bins, o in layout}
            self._take(name, tables, float(a[0]), int(a[1:2].view(np.int64)[0]))
            self.status |= int(a[2:3].view(np.int32)[0])
        self.inflight = keep

    def read_back(self, k):
        self._launch_pending()
        self._harvest()
        return (self.tables, self.prob_sum, self.n_sites), self.status

    def merge(self, states, k):
        tables, prob_sum, n_sites = {}, 0.0, 0
        for t, s, c in states:
            for name, per_w in t.items():
                mine = tables.setdefault(name, {})
                for W, (bin0, tab) in per_w.items():
                    mine[W] = _merge_window_table(mine.get(W), bin0, tab)
            prob_sum, n_sites = prob_sum + s, n_sites + c
        return tables, prob_sum, n_sites

    def finish(self, state, k, result):
        tables, prob_sum, n_sites = state
        windows = {}
        for W in self.sizes:
            keys, rows = [], []
            for name in sorted(tables):
                bin0, t = tables[name].get(W, (0, np.zeros((0, 1))))
                live = np.nonzero(t[:, 0] > 0)[0]
                keys += [(name, int((bin0 + g) * W + W)) for g in live]
                rows.append(t[live])
            windows[W] = (keys, np.concatenate(rows) if rows else np.zeros((0, 1 + 2 * (k or 0))))
        result.update(prob_sum=prob_sum, n_sites=n_sites, windows=windows)

    def write(self, out_prefix, result, k, written):
        for W in self.sizes:
            written += list(regional_output_names(out_prefix, W)[:2])
            write_regional_outputs(*result["windows"][W], k, W, out_prefix, self.ratio_cutoff)


def _kmer_part_host(genome, prob, start, end, strand, label, k, lengths, fields, into):
    return summary_kmer_host(genome, prob, start, end, strand, label, k, lengths, bool(fields["indel"]), fields["mode"], into=into)


def _motif_part_host(genome, prob, start, end, strand, label, k, lengths, fields, into):
    return summary_motif_host(genome, prob, start, end, label, k, lengths, bool(fields["indel"]), into=into)


# what tells the k-mer reduction from the motif reduction (`fields`, the struct's own settings, come from the sink)
_KMERS = dict(name="kmers", what="k-mer", check=check_kmer_length, struct=_lib.MuralSummaryKmerRows, entry="mural_summary_kmer_rows",
              count="n_k", length="k", strand=True, host=_kmer_part_host, shift=_KMER_ORD_SHIFT, from_sums=kmer_table_from_sums,
              output_names=kmer_output_names, write=write_kmer_outputs)
_MOTIFS = dict(name="motifs", what="motif", check=check_motif_length, struct=_lib.MuralSummaryMotifRows, entry="mural_summary_motif_rows",
               count="n_m", length="m", strand=False, host=_motif_part_host, shift=_MOTIF_ORD_SHIFT, from_sums=motif_table_from_sums,
               output_names=motif_output_names, write=write_motif_outputs)


class _KeyedReducer:
    """The rate tables keyed by a sequence word around the site, for each of `lengths`: the k-mer tables (`kind` = _KMERS) or the motif
    tables (_MOTIFS).  Exact integer sums in accumulators of a fixed size -- the tables per length, the first-appearance words per
    chromosome and length (two chromosomes share words, and their order, by name as in the written table, is known only when all have
    arrived) --, on the host and per device, read back once."""

    def __init__(self, kind, lengths, genome):
        self.kind, self.name = kind, kind["name"]
        self.lengths = tuple(kind["check"](n) for n in lengths)
        if len(set(self.lengths)) != len(self.lengths):
            raise ValueError(f"{kind['what']} lengths must be distinct (got {self.lengths})")
        if self.lengths and genome is None:
            raise ValueError(f"SummarySink({self.name}=...) needs genome=: a callable chromosome name -> packed genome")
        self.genome = genome
        self.fields = {}               # the struct's settings beside rows and tables (indel, mode / order_by_row): the sink's to set
        self.reset()

    def reset(self):
        self.host = ({}, {})           # ({length: table}, {chromosome: {length: first}}) of the host shards
        self.dev = {}                  # device -> ({length: table}, {chromosome: {length: first}}, status)
        self.sums = None

    def host_part(self, name, prob, start, end, strand, label, k):
        tabs, firsts = self.host
        for n in self.lengths:
            tabs.setdefault(n, np.zeros((4 ** n, 3, k), np.uint64))
        mine = firsts.setdefault(name, {n: np.full(4 ** n, _KMER_NEVER, np.uint64) for n in self.lengths})
        _, status = self.kind["host"](self.genome(name), prob, start, end, strand, label, k, self.lengths, self.fields,
                                      {n: (tabs[n], mine[n]) for n in self.lengths})
        return status

    def device_part(self, name, prob, start, end, strand, label, k):
        """Enqueue the reduction of a part behind its forward: the part's chromosome is the resident one now."""
        kind, dev = self.kind, prob.device
        genome = self.genome(name)
        if genome.length >= 1 << (_KMER_ORD_SHIFT - 1):
            raise ValueError(f"{kind['what']} summary: chromosome {name} has 2^39 bases or more")
        acc = self.dev.get(dev)
        if acc is None:
            acc = self.dev[dev] = ({n: torch.zeros(4 ** n * 3 * k, dtype=torch.int64, device=dev) for n in self.lengths}, {},
                                   torch.zeros(1, dtype=torch.int32, device=dev))
        first = acc[1].get(name)
        if first is None:              # (all ones: the largest unsigned value)
            first = acc[1][name] = {n: torch.full((4 ** n,), -1, dtype=torch.int64, device=dev) for n in self.lengths}
        g = genome.as_struct(dev)
        entry, stream = getattr(_lib.lib(), kind["entry"]), _lib.current_stream_ptr(dev)
        for group in _calls_of(self.lengths):
            s = kind["struct"]()
            s.genome = C.pointer(g)
            _row_fields(s, prob, start, end, label)
            if kind["strand"]:
                s.strand = strand.data_ptr()
            s.n_class = k
            setattr(s, kind["count"], len(group))
            for key, value in self.fields.items():
                setattr(s, key, value)
            lengths = getattr(s, kind["length"])
            for j, n in enumerate(group):
                lengths[j], s.table[j], s.first[j] = n, acc[0][n].data_ptr(), first[n].data_ptr()
            s.order_base, s.status = 0, acc[2].data_ptr()
            _lib.check(entry(C.byref(s), stream))
        return genome

    def read_back(self, k):
        """The one read-back of the device accumulators, merged with the host rows'."""
        status, mine = 0, [self.host]
        for tabs, firsts, dev_status in self.dev.values():
            status |= int(dev_status.item())
            mine.append(({n: t.cpu().numpy().view(np.uint64).reshape(4 ** n, 3, -1) for n, t in tabs.items()},
                         {nm: {n: f.cpu().numpy().view(np.uint64) for n, f in per_n.items()} for nm, per_n in firsts.items()}))
        shift = self.kind["shift"]
        return _kmer_merge([_kmer_collapse(tabs, firsts, shift) for tabs, firsts in mine if tabs], shift), status

    def merge(self, states, k):
        return _kmer_merge(states, self.kind["shift"])

    def finish(self, state, k, result):
        self.sums = state[1]
        none = ([], np.zeros((0, 1 + 2 * (k or 0))))
        result[self.name] = {n: (self.kind["from_sums"](*self.sums[n], n, k) if n in self.sums else none) for n in self.lengths}

    def write(self, out_prefix, result, k, written):
        for n in self.lengths:
            written += list(self.kind["output_names"](out_prefix, n))
            self.kind["write"](*result[self.name][n], k, n, out_prefix)


_DEVICE_DTYPE = {np.uint64: torch.int64, np.uint32: torch.int32}


class _TableReducer:
    """The lifecycle of a reducer whose state is one or more integer tables that are plain sums over the rows: ONE set of tables for
    the whole run on the host (created by the first host part) and one per device (created by the first device part, with a status
    word), read back once and added.  ``_tables(k)`` describes them: (key of the device dict, shape, dtype, fold or None) each, the
    fold being the carry of the lo limbs that follows every addition of two such tables (``_kmer_fold``, ``_conseq_fold``).  The state
    -- ``host``, what ``read_back`` and ``merge`` return, what ``finish`` keeps under the attribute named by `kept` -- is the table
    itself where there is one and the tuple of them otherwise.  A subclass keeps what is its own: the chromosomes it skips, its class
    check, its host and device calls, ``finish`` and ``write``."""
    kept = "sums"

    def _tables(self, k):
        raise NotImplementedError

    def reset(self):
        self.host = None               # the tables of the host shards
        self.dev = {}                  # device -> dict(<key>: flat table ..., status, and what the subclass uploads)
        setattr(self, self.kept, None)

    def _state(self, tables, k):
        return tables[0] if len(self._tables(k)) == 1 else tuple(tables)

    def _zeros(self, k):
        return self._state([np.zeros(shape, dtype) for _, shape, dtype, _ in self._tables(k)], k)

    def _host(self, k):
        if self.host is None:
            self.host = self._zeros(k)
        return self.host

    def _acc(self, dev, k, **own):
        """The device's accumulators, zeros the first time, with the subclass's `own` entries (caches, workspace)."""
        acc = self.dev.get(dev)
        if acc is None:
            acc = self.dev[dev] = {key: torch.zeros(max(int(np.prod(shape)), 1), dtype=_DEVICE_DTYPE[dtype], device=dev)
                                   for key, shape, dtype, _ in self._tables(k)}
            acc.update(own, status=torch.zeros(1, dtype=torch.int32, device=dev))
        return acc

    def _added(self, states, k):
        """The states added table by table, carries folded; None where there is none; never one of `states` itself."""
        spec, out = self._tables(k), None
        for st in states:
            if st is None:
                continue
            st = (st,) if len(spec) == 1 else st
            if out is None:
                out = [t.copy() for t in st]
                continue
            for have, t, (_, _, _, fold) in zip(out, st, spec):
                np.add(have, t, out=have)
                if fold is not None:
                    fold(have)
        return None if out is None else self._state(out, k)

    def read_back(self, k):
        """The one read-back of the device tables, added to the host rows'."""
        status, mine = 0, [self.host]
        for acc in self.dev.values():
            status |= int(acc["status"].item())
            mine.append(self._state([acc[key].cpu().numpy().view(dtype)[:int(np.prod(shape))].reshape(shape)
                                     for key, shape, dtype, _ in self._tables(k)], k))
        return self._added(mine, k), status

    def merge(self, states, k):
        return self._added(states, k)

    def finish(self, state, k, result):
        setattr(self, self.kept, self._zeros(k) if state is None else state)


def _check_simulation(n_rep, seed, table_bytes_max=None, cells=0, what="", seed_text="simulate_seed is an unsigned 64-bit integer"):
    """The checks every simulation reducer makes: the replicates, the seed and -- given `table_bytes_max` -- the bytes of its uint32
    table of `cells` cells (`what`: their description) per replicate.  `seed_text` is there for the INDEL structure simulation alone,
    whose seed message has always been worded differently: callers match on these texts, so it stays."""
    if not 1 <= n_rep <= SIMULATE_MAX_REPLICATES:
        raise ValueError("simulate: 1 .. 2^20 replicates")
    if not 0 <= seed < 1 << 64:
        raise ValueError(seed_text)
    need = cells * n_rep * 4
    if table_bytes_max is not None and need > table_bytes_max:
        raise ValueError(f"simulate: the table of {what} x {n_rep} replicates takes {need} bytes, above simulate_table_bytes_max = "
                         f"{table_bytes_max}")


def _device_rows(prob, start, **cols):
    """The row keywords of the ``*_rows_device`` functions from a device part's tensors; `cols`: strand= (a tensor or None) and label=
    where the function takes them."""
    rows = dict(prob=prob.data_ptr(), prob_f64=prob.dtype == torch.float64, prob_stride=prob.stride(0), start=start.data_ptr(),
                n=start.shape[0])
    if "strand" in cols:
        rows["strand"] = None if cols["strand"] is None else cols["strand"].data_ptr()
    if "label" in cols:
        rows.update(label=cols["label"].data_ptr(), label_kind=_LABEL_KIND[cols["label"].dtype])
    return rows


class _AnnotationReducer(_TableReducer):
    """Expected and observed mutations per name of an annotation BED (``tables.read_annotations``): ONE integer table [names][3][n_class]
    for the whole run on the host and one per device -- the group ids are global --, a chromosome's pieces uploaded the first time the
    chromosome arrives on a device, read back once.  A chromosome without pieces reduces nothing."""
    name = "annotations"

    def __init__(self, annotations):
        self.names, self.meta, self.pieces = read_annotations(annotations)
        if len(self.names) >= 2 ** 31:
            raise ValueError("annotations: 2^31 names or more")
        self.reset()

    def _tables(self, k):
        return (("table", (len(self.names), 3, k or 0), np.uint64, _kmer_fold),)

    def host_part(self, name, prob, start, end, strand, label, k):
        pieces = self.pieces.get(name)
        if pieces is None:
            return 0
        return summary_annot_host(prob, start, label, k, pieces, len(self.names), into=self._host(k))[1]

    def device_part(self, name, prob, start, end, strand, label, k):
        """Enqueue the reduction of a part behind its forward, into the device's one table."""
        pieces = self.pieces.get(name)
        if pieces is None or start.shape[0] == 0:
            return None
        dev, lib = prob.device, _lib.lib()
        acc = self._acc(dev, k, pieces={}, ws=None)
        on_dev = _upload_once(acc["pieces"], name, pieces, dev)
        s = _lib.MuralSummaryAnnotRows()
        _fill_rows(s, k, **_device_rows(prob, start, label=label))
        s.n_groups = len(self.names)
        s.piece_b0, s.piece_b1, s.piece_group, s.n_pieces = (on_dev[0].data_ptr(), on_dev[1].data_ptr(), on_dev[2].data_ptr(),
                                                             on_dev[0].shape[0])
        s.table, s.status = acc["table"].data_ptr(), acc["status"].data_ptr()
        ws = _grow_ws(acc, int(lib.mural_summary_annot_workspace_bytes(start.shape[0], k)), dev)
        _lib.check(lib.mural_summary_annot_rows(C.byref(s), *ws, _lib.current_stream_ptr(dev)))
        return None

    def finish(self, state, k, result):
        super().finish(state, k, result)
        result[self.name] = (list(self.names), annotation_meta(self.names, self.meta), annot_table_from_sums(self.sums, k or 0))

    def write(self, out_prefix, result, k, written):
        written += list(annotation_output_names(out_prefix))
        write_annotation_outputs(*result[self.name], k, out_prefix)


class _ConsequenceReducer(_TableReducer):
    """Expected and observed mutations per transcript of a BED12 file by consequence (``summary_conseq_host`` is the rule): ONE integer
    table [transcripts][5][3] + row counters [transcripts][2] for the whole run on the host and one pair per device -- the transcript
    ids are global --, a chromosome's segment arrays uploaded the first time the chromosome arrives on a device, read back once.  A
    chromosome without CDS segments reduces nothing."""
    name = "consequences"

    def __init__(self, transcripts, genome, codon_table, alt_order, labels=True):
        self.names, self.meta, self.segments = read_transcripts(transcripts, codon_table)
        self.alt_order, self.labels = check_alt_order(alt_order), bool(labels)
        if genome is None:
            raise ValueError("SummarySink(transcripts=...) needs genome=: a callable chromosome name -> packed genome")
        self.genome = genome
        self.reset()

    def _tables(self, k):
        return (("table", (len(self.names), 5, 3), np.uint64, _conseq_fold), ("rows", (len(self.names), 2), np.uint64, None))

    def _check(self, k):
        if k != 4:
            raise ValueError(f"SummarySink(transcripts=...) takes SNV rows of 4 classes (got {k}; INDEL tables are out of scope)")

    def host_part(self, name, prob, start, end, strand, label, k):
        self._check(k)
        segments = self.segments.get(name)
        if segments is None:
            return 0
        return summary_conseq_host(self.genome(name), prob, start, strand, label, segments, len(self.names), self.meta["aa"],
                                   self.alt_order, into=self._host(k))[2]

    def device_part(self, name, prob, start, end, strand, label, k):
        """Enqueue the reduction of a part behind its forward, into the device's one pair of tables."""
        self._check(k)
        segments = self.segments.get(name)
        if segments is None or start.shape[0] == 0:
            return None
        dev, genome = prob.device, self.genome(name)
        conseq_rows_device(self._acc(dev, k, segments={}, ws=None), name, segments, len(self.names), self.meta["aa"], self.alt_order,
                           genome.as_struct(dev), dev, **_device_rows(prob, start, strand=strand, label=label))
        return genome

    def finish(self, state, k, result):
        super().finish(state, k, result)
        result[self.name] = (list(self.names), self.meta, consequence_table_from_sums(*self.sums))

    def write(self, out_prefix, result, k, written):
        written.append(consequence_output_name(out_prefix))
        write_consequence_outputs(*result[self.name], out_prefix, labels=self.labels)


class _StructureReducer(_TableReducer):
    """Expected and observed mutations per transcript by where a row lies in the transcript's structure (``summary_txstruct_host`` is
    the rule), behind the consequence reducer `conseq`, whose names, genome, codon table and device segment arrays it uses: ONE integer
    table [transcripts][9][3] + row counters [transcripts][2] for the whole run on the host and one pair per device, a chromosome's item
    arrays uploaded the first time the chromosome arrives on a device, read back once.  A chromosome without items reduces nothing."""
    name = "transcript_structure"

    def __init__(self, features, conseq):
        self.features, self.conseq = features, conseq
        self.reset()

    def _tables(self, k):
        n_tx = len(self.conseq.names)
        return (("table", (n_tx, TX_BINS, 3), np.uint64, _conseq_fold), ("rows", (n_tx, 2), np.uint64, None))

    def host_part(self, name, prob, start, end, strand, label, k):
        self.conseq._check(k)
        features = self.features.get(name)
        if features is None:
            return 0
        return summary_txstruct_host(self.conseq.genome(name), prob, start, strand, label, self.conseq.segments.get(name), features,
                                     len(self.conseq.names), self.conseq.meta["aa"], self.conseq.alt_order, into=self._host(k))[2]

    def device_part(self, name, prob, start, end, strand, label, k):
        """Enqueue the reduction of a part behind its consequence reduction, into the device's one pair of tables."""
        self.conseq._check(k)
        features = self.features.get(name)
        if features is None or start.shape[0] == 0:
            return None
        dev, genome = prob.device, self.conseq.genome(name)
        acc = self._acc(dev, k, features={}, ws=None, no_cds=dict(segments={}))
        # (the consequence reducer has no accumulators on a device that saw only chromosomes without CDS: the strands go to `no_cds`)
        txstruct_rows_device(acc, self.conseq.dev.get(dev, acc["no_cds"]), name, self.conseq.segments.get(name), features,
                             len(self.conseq.names), self.conseq.meta["aa"], self.conseq.alt_order, genome.as_struct(dev), dev,
                             **_device_rows(prob, start, strand=strand, label=label))
        return genome

    def finish(self, state, k, result):
        super().finish(state, k, result)
        result[self.name] = (list(self.conseq.names), *self.sums)

    def write(self, out_prefix, result, k, written):
        written.append(structure_output_name(out_prefix))
        names, table, rows = result[self.name]
        write_structure_outputs(names, self.conseq.meta, table, rows, self.conseq.sums[0][:, 2], out_prefix, labels=self.conseq.labels)


class _IndelStructureReducer(_TableReducer):
    """Expected and observed INDEL events per transcript of a BED12 file by what they do to the transcript's structure
    (``summary_txindel_host`` is the rule): ONE integer table [transcripts][10][3] + row counters [transcripts][2] for the whole run on
    the host and one pair per device -- the transcript ids are global --, a chromosome's item, link and segment arrays uploaded the
    first time the chromosome arrives on a device, read back once.  A chromosome without items reduces nothing.  `genome` (optional)
    gives the chromosomes' lengths; no base is read."""
    name = "indel_structure"

    def __init__(self, transcripts, kind, lengths, breakpoint_offset, genome=None, labels=True):
        self.names, self.meta, self.segments, self.features = read_transcript_structure(transcripts)
        if kind is None:
            raise ValueError("SummarySink(indel_transcripts=...) needs indel_kind=: 'insertion', 'deletion_start' or 'deletion_end'")
        self.kind, self.offset = check_indel_kind(kind), check_breakpoint_offset(breakpoint_offset)
        self.lengths = lengths if lengths is None else check_indel_lengths(lengths)      # (the count is checked when the classes are known)
        self.genome, self.labels = genome, bool(labels)
        self.links, self.class_len = {}, None
        self.reset()

    def _tables(self, k):
        return (("table", (len(self.names), TXINDEL_BINS, 3), np.uint64, _conseq_fold), ("rows", (len(self.names), 2), np.uint64, None))

    def _part(self, name, k):
        """(features, links, chromosome length or None) of chromosome `name`, None where it has no items; the classes' lengths checked."""
        if not 2 <= k <= 16:
            raise ValueError(f"SummarySink(indel_transcripts=...) takes INDEL rows of 2 .. 16 classes (got {k})")
        if self.class_len is None or len(self.class_len) != k:
            self.class_len = check_indel_lengths(self.lengths, k)
        features = self.features.get(name)
        if features is None:
            return None
        if name not in self.links:
            self.links[name] = structure_links(features)
        length = None
        if self.genome is not None:
            genome = self.genome(name)
            length = int(genome.length) if hasattr(genome, "length") else len(genome)
        return features, self.links[name], length

    def host_part(self, name, prob, start, end, strand, label, k):
        part = self._part(name, k)
        if part is None:
            return 0
        return summary_txindel_host(prob, start, label, k, self.segments.get(name), part[0], len(self.names), self.kind, self.offset,
                                    self.class_len, part[2], links=part[1], into=self._host(k))[2]

    def device_part(self, name, prob, start, end, strand, label, k):
        """Enqueue the reduction of a part behind its forward, into the device's one pair of tables."""
        part = self._part(name, k)
        if part is None or start.shape[0] == 0:
            return None
        dev = prob.device
        txindel_rows_device(self._acc(dev, k, features={}, segments={}, ws=None), name, self.segments.get(name), part[0], part[1],
                            len(self.names), self.kind, self.offset, self.class_len, part[2], dev, n_class=k,
                            **_device_rows(prob, start, label=label))
        return None

    def finish(self, state, k, result):
        super().finish(state, k, result)
        result[self.name] = (list(self.names), *self.sums)

    def write(self, out_prefix, result, k, written):
        written.append(indel_structure_output_name(out_prefix))
        names, table, rows = result[self.name]
        write_indel_structure_outputs(names, self.meta, table, rows, self.kind, out_prefix, labels=self.labels)


class _SimulationReducer(_TableReducer):
    """Mutation sets drawn from the rates (``simulate_rows_host`` is the rule): per name of the annotation reducer beside it the counts
    of every class in each of `n_rep` replicates -- ONE uint32 table [names][n_class - 1][n_rep] on the host and one per device, the
    pieces the annotation reducer uploaded, read back once --, and the replicates of `write` as mutation lists, a file per replicate
    written part by part (a rank's parts into its own part file; rank 0 strings them together in (shard, rank) order at close)."""
    name, kept = "simulation", "counts"

    def __init__(self, n_rep, seed, write, annot, table_bytes_max, out_prefix, labels, rank, world):
        self.n_rep, self.seed, self.write_reps = int(n_rep), int(seed), tuple(int(r) for r in write)
        _check_simulation(self.n_rep, self.seed)
        if any(not 0 <= r < self.n_rep for r in self.write_reps) or len(set(self.write_reps)) != len(self.write_reps):
            raise ValueError(f"simulate_write: distinct replicates in 0 .. {self.n_rep - 1}")
        if self.write_reps and out_prefix is None:
            raise ValueError("simulate_write needs an out_prefix")
        self.annot, self.table_bytes_max, self.out_prefix, self.labels = annot, int(table_bytes_max), out_prefix, bool(labels)
        self.rank, self.world = rank, world
        self.reset()

    def _tables(self, k):
        return (("table", (self._groups(), max((k or 1) - 1, 0), self.n_rep), np.uint32, None),)

    def reset(self):
        super().reset()
        self.pending = []              # device mutation lists not yet on the host: (event, chrom, shard number, {replicate: buffers})
        self.shard, self.last = -1, None
        self.index = {r: [] for r in self.write_reps}      # replicate -> [chromosome, bytes] per run of parts of one chromosome, in file order
        for fh in getattr(self, "files", {}).values():
            fh.close()
        self.files = {}

    def _groups(self):
        return 0 if self.annot is None else len(self.annot.names)

    def _check_table(self, k):
        _check_simulation(self.n_rep, self.seed, self.table_bytes_max, self._groups() * (k - 1), f"{self._groups()} names x {k - 1} classes")
        if k < 2:
            raise ValueError("simulate needs at least 2 classes")

    def _next_shard(self, name):
        """Parts of one chromosome continue its shard (the sink takes the chromosomes one after the other)."""
        if name != self.last:
            self.shard, self.last = self.shard + 1, name
            for r in self.write_reps:
                self.index[r].append([name, 0])

    def _path(self, r):
        path = simulation_bed_name(self.out_prefix, r)
        return path + (".part%04d" % self.rank if self.world > 1 else "")

    def _emit(self, chrom, r, start, strand, label):
        if r not in self.files:
            self.files[r] = open(self._path(r), "w")
        text = simulation_bed_text(chrom, start, strand, label)
        self.files[r].write(text)
        self.index[r][-1][1] += len(text)

    def host_part(self, name, prob, start, end, strand, label, k):
        self._check_table(k)
        self._next_shard(name)
        key = simulate_chrom_key(name)
        status = 0
        pieces = None if self.annot is None else self.annot.pieces.get(name)
        if pieces is not None:
            status |= simulate_annot_host(prob, start, strand, k, key, self.seed, pieces, self._groups(), self.n_rep, into=self._host(k))[1]
        if self.write_reps:
            self._drain()
            labels, st = simulate_rows_host(prob, start, strand, k, key, self.seed, self.write_reps, with_status=True)
            status |= st
            for j, r in enumerate(self.write_reps):
                hit = labels[:, j] > 0
                self._emit(name, r, np.asarray(start)[hit], np.asarray(strand)[hit], labels[hit, j])
        return status

    def device_part(self, name, prob, start, end, strand, label, k):
        self._check_table(k)
        self._next_shard(name)
        n = start.shape[0]
        if n == 0:
            return None
        dev, lib = prob.device, _lib.lib()
        acc = self._acc(dev, k, ws=None)
        if "copy" not in acc:
            acc["copy"] = torch.cuda.Stream(dev)
        key, stream, rows = simulate_chrom_key(name), _lib.current_stream_ptr(dev), _device_rows(prob, start, strand=strand)
        on_dev = None if self.annot is None else self.annot.dev.get(dev, {}).get("pieces", {}).get(name)      # uploaded just before
        if on_dev is not None:
            s = _lib.MuralSimulateAnnotRows()
            _fill_rows(s, k, **rows)
            s.chrom_key, s.n_rep, s.seed = key, self.n_rep, self.seed
            s.piece_b0, s.piece_b1, s.piece_group, s.n_pieces = (on_dev[0].data_ptr(), on_dev[1].data_ptr(), on_dev[2].data_ptr(),
                                                                 on_dev[0].shape[0])
            s.n_groups, s.table, s.status = self._groups(), acc["table"].data_ptr(), acc["status"].data_ptr()
            ws = _grow_ws(acc, int(lib.mural_simulate_annot_workspace_bytes(on_dev[0].shape[0])), dev)
            _lib.check(lib.mural_simulate_annot_rows(C.byref(s), *ws, stream))
        if self.write_reps:
            self._drain()
            lists = {}
            for r in self.write_reps:
                out = dict(start=torch.empty(n, dtype=torch.int64, device=dev), strand=torch.empty(n, dtype=torch.uint8, device=dev),
                           label=torch.empty(n, dtype=torch.uint8, device=dev), count=torch.zeros(1, dtype=torch.int64, device=dev))
                s = _lib.MuralSimulateRows()
                _fill_rows(s, k, **rows)
                s.chrom_key, s.replicate, s.seed = key, r, self.seed
                s.out_start, s.out_strand, s.out_label = out["start"].data_ptr(), out["strand"].data_ptr(), out["label"].data_ptr()
                s.count, s.status = out["count"].data_ptr(), acc["status"].data_ptr()
                ws = _grow_ws(acc, int(lib.mural_simulate_rows_workspace_bytes(n)), dev)
                _lib.check(lib.mural_simulate_rows(C.byref(s), *ws, stream))
                lists[r] = out
            event = torch.cuda.Event()
            event.record(torch.cuda.current_stream(dev))
            self.pending.append((event, name, len(self.index[self.write_reps[0]]) - 1, lists, acc["copy"]))
        return None

    def _drain(self, wait=False):
        """Bring the finished device lists to the host, in order, and write them.  The copies run on a stream of their own, so that
        they do not wait for the forward that is already enqueued; without `wait` the lists still in flight stay (they keep their
        place: nothing later is written before them)."""
        while self.pending:
            event, name, shard, lists, copy = self.pending[0]
            if not wait and not event.query():
                return
            event.synchronize()
            with torch.cuda.stream(copy):
                for r, out in lists.items():
                    m = int(out["count"].cpu().item())
                    cols = [out[key][:m].cpu().numpy() for key in ("start", "strand", "label")]
                    if r not in self.files:
                        self.files[r] = open(self._path(r), "w")
                    text = simulation_bed_text(name, *cols)
                    self.files[r].write(text)
                    self.index[r][shard][1] += len(text)
            self.pending.pop(0)

    def read_back(self, k):
        """The one read-back of the device tables, added to the host rows'; the mutation lists are flushed."""
        table, status = super().read_back(k)
        self._drain(wait=True)
        for r in self.write_reps:      # a rank without rows still has its (empty) file
            if r not in self.files:
                self.files[r] = open(self._path(r), "w")
        for fh in self.files.values():
            fh.close()
        return dict(table=table, index={r: [tuple(v) for v in segs] for r, segs in self.index.items()}), status

    def merge(self, states, k):
        return dict(table=self._added([st["table"] for st in states], k), index=[st["index"] for st in states])

    def finish(self, state, k, result):
        super().finish(state["table"], k, result)
        self._index = state["index"]
        if self.annot is not None:
            names, _, annot = result["annotations"]
            observed = annot[:, 2:1 + k] if (k and self.labels) else None
            expected = annot[:, 2 + k:1 + 2 * k] if k else None
            result[self.name] = (names, self.counts, observed, expected)

    def write(self, out_prefix, result, k, written):
        if self.annot is not None:
            written.append(simulation_output_name(out_prefix))
            write_simulation_outputs(*result[self.name], k, out_prefix)
        for r in self.write_reps:
            path = simulation_bed_name(out_prefix, r)
            written.append(path)
            if self.world > 1:             # every rank closed its part before the sink's collective returned
                index = [st[r] for st in self._index]
                order = list(dict.fromkeys(name for segs in index for name, _ in segs))      # rank 0's shard order, then the others'
                srcs = [open(path + ".part%04d" % rank, "r") for rank in range(self.world)]
                try:
                    with open(path, "w") as dst:
                        for name in order:
                            for rank, src in enumerate(srcs):
                                at = 0
                                for seg_name, size in index[rank]:
                                    if seg_name == name and size:
                                        src.seek(at)
                                        dst.write(src.read(size))
                                    at += size
                finally:
                    for src in srcs:
                        src.close()
                for rank in range(self.world):
                    os.unlink(path + ".part%04d" % rank)


class _ConsequenceSimulationReducer(_TableReducer):
    """The simulated null of the consequence table (``simulate_conseq_host`` is the rule): per transcript of the consequence reducer
    before it, consequence bin and replicate the simulated count -- ONE uint32 table [transcripts][5][n_rep] on the host and one per
    device, on the segment arrays the consequence reducer uploaded just before, read back once."""
    name, kept = "consequence_simulation", "counts"

    def __init__(self, n_rep, seed, conseq, table_bytes_max):
        self.n_rep, self.seed, self.conseq, self.table_bytes_max = int(n_rep), int(seed), conseq, int(table_bytes_max)
        _check_simulation(self.n_rep, self.seed, self.table_bytes_max, len(conseq.names) * 5, f"{len(conseq.names)} transcripts x 5 consequences")
        self.reset()

    def _tables(self, k):
        return (("table", (len(self.conseq.names), 5, self.n_rep), np.uint32, None),)

    def host_part(self, name, prob, start, end, strand, label, k):
        self.conseq._check(k)
        segments = self.conseq.segments.get(name)
        if segments is None:
            return 0
        return simulate_conseq_host(self.conseq.genome(name), prob, start, strand, segments, len(self.conseq.names), simulate_chrom_key(name),
                                    self.seed, self.n_rep, self.conseq.meta["aa"], self.conseq.alt_order, into=self._host(k))[1]

    def device_part(self, name, prob, start, end, strand, label, k):
        """Enqueue the draws of a part behind its consequence reduction, into the device's one table."""
        self.conseq._check(k)
        if self.conseq.segments.get(name) is None or start.shape[0] == 0:
            return None
        dev, genome = prob.device, self.conseq.genome(name)
        acc = self._acc(dev, k)
        simulate_conseq_rows_device(acc["table"], acc["status"], self.conseq.dev[dev], name, len(self.conseq.names), self.conseq.meta["aa"],
                                    self.conseq.alt_order, genome.as_struct(dev), dev, self.n_rep, self.seed,
                                    **_device_rows(prob, start, strand=strand))
        return genome

    def finish(self, state, k, result):
        super().finish(state, k, result)
        names, _, table = result["consequences"]
        observed = table[:, 4:11:2] if self.conseq.labels else None
        result[self.name] = (names, self.counts, observed, table[:, 3:11:2])

    def write(self, out_prefix, result, k, written):
        written.append(consequence_simulation_output_name(out_prefix))
        write_consequence_simulation_outputs(*result[self.name], out_prefix)


class _StructureSimulationReducer(_TableReducer):
    """The simulated null of the structure table and of the loss-of-function count (``simulate_txstruct_host`` is the rule): per
    transcript, structure bin and replicate the simulated count -- ONE uint32 table [transcripts][9][n_rep] on the host and one per
    device, behind the structure reducer `struct` (whose item arrays and workspace it uses) and the consequence simulation `conseq_sim`
    (whose stop-gained counts of the same draws complete the LoF count), read back once."""
    name, kept = "structure_simulation", "counts"

    def __init__(self, n_rep, seed, struct, conseq_sim, table_bytes_max):
        self.n_rep, self.seed, self.struct, self.conseq_sim = int(n_rep), int(seed), struct, conseq_sim
        self.conseq, self.table_bytes_max = struct.conseq, int(table_bytes_max)
        _check_simulation(self.n_rep, self.seed, self.table_bytes_max, len(self.conseq.names) * TX_BINS,
                          f"{len(self.conseq.names)} transcripts x {TX_BINS} structure bins")
        self.reset()

    def _tables(self, k):
        return (("table", (len(self.conseq.names), TX_BINS, self.n_rep), np.uint32, None),)

    def reset(self):
        super().reset()
        self.lof = None

    def host_part(self, name, prob, start, end, strand, label, k):
        self.conseq._check(k)
        features = self.struct.features.get(name)
        if features is None:
            return 0
        return simulate_txstruct_host(self.conseq.genome(name), prob, start, strand, self.conseq.segments.get(name), features,
                                      len(self.conseq.names), simulate_chrom_key(name), self.seed, self.n_rep, self.conseq.meta["aa"],
                                      self.conseq.alt_order, into=self._host(k))[1]

    def device_part(self, name, prob, start, end, strand, label, k):
        """Enqueue the draws of a part behind its structure reduction, into the device's one table."""
        self.conseq._check(k)
        if self.struct.features.get(name) is None or start.shape[0] == 0:
            return None
        dev, genome = prob.device, self.conseq.genome(name)
        acc, items = self._acc(dev, k), self.struct.dev[dev]
        simulate_txstruct_rows_device(acc["table"], acc["status"], items, self.conseq.dev.get(dev, items["no_cds"]), name,
                                      len(self.conseq.names), self.conseq.meta["aa"], self.conseq.alt_order, genome.as_struct(dev), dev,
                                      self.n_rep, self.seed, **_device_rows(prob, start, strand=strand))
        return genome

    def finish(self, state, k, result):
        super().finish(state, k, result)
        self.lof = simulate_lof_counts(self.conseq_sim.counts, self.counts)
        names, table, _ = result["transcript_structure"]
        expected, observed = structure_cells_from_sums(table, self.conseq.sums[0][:, 2])
        result[self.name] = (names, self.counts, self.lof, observed if self.conseq.labels else None, expected)

    def write(self, out_prefix, result, k, written):
        written.append(structure_simulation_output_name(out_prefix))
        write_structure_simulation_outputs(*result[self.name], out_prefix)


class _IndelStructureSimulationReducer(_TableReducer):
    """The simulated null of the INDEL structure table and of its loss-of-function counts (``simulate_txindel_host`` is the rule): per
    transcript, INDEL structure bin and replicate the simulated count -- ONE uint32 table [transcripts][10][n_rep] on the host and one
    per device, behind the INDEL structure reducer `struct`, whose item, link and segment arrays and workspace it uses, read back once.
    A cell takes one count per row that its transcript counts: the run keeps those below 2^32, as the structure simulation does."""
    name, kept = "indel_structure_simulation", "counts"

    def __init__(self, n_rep, seed, struct, table_bytes_max):
        self.n_rep, self.seed, self.struct, self.table_bytes_max = int(n_rep), int(seed), struct, int(table_bytes_max)
        _check_simulation(self.n_rep, self.seed, self.table_bytes_max, len(struct.names) * TXINDEL_BINS,
                          f"{len(struct.names)} transcripts x {TXINDEL_BINS} INDEL structure bins",
                          seed_text="simulate: the seed is an unsigned 64-bit integer")
        self.reset()

    def _tables(self, k):
        return (("table", (len(self.struct.names), TXINDEL_BINS, self.n_rep), np.uint32, None),)

    def reset(self):
        super().reset()
        self.lof = self.lof_upper = None

    def _part(self, name, k):
        if not 2 <= k <= 8:
            raise ValueError(f"SummarySink(simulate_indel_structure=True) takes INDEL rows of 2 .. 8 classes, the bound of the "
                             f"simulation's draw (got {k})")
        return self.struct._part(name, k)

    def host_part(self, name, prob, start, end, strand, label, k):
        part = self._part(name, k)
        if part is None:
            return 0
        return simulate_txindel_host(prob, start, strand, k, self.struct.segments.get(name), part[0], len(self.struct.names), self.struct.kind,
                                     simulate_chrom_key(name), self.seed, self.n_rep, self.struct.offset, self.struct.class_len, part[2],
                                     links=part[1], into=self._host(k))[1]

    def device_part(self, name, prob, start, end, strand, label, k):
        """Enqueue the draws of a part behind its INDEL structure reduction, into the device's one table."""
        part = self._part(name, k)
        if part is None or start.shape[0] == 0:
            return None
        dev, acc = prob.device, self._acc(prob.device, k)
        simulate_txindel_rows_device(acc["table"], acc["status"], self.struct.dev[dev], name, len(self.struct.names), self.struct.kind,
                                     self.struct.offset, self.struct.class_len, part[2], dev, self.n_rep, self.seed, n_class=k,
                                     **_device_rows(prob, start, strand=strand))
        return None

    def finish(self, state, k, result):
        super().finish(state, k, result)
        self.lof, self.lof_upper = simulate_indel_lof_counts(self.counts)
        names, table, _ = result["indel_structure"]
        expected, observed = indel_structure_cells_from_sums(table)
        result[self.name] = (names, self.counts, self.lof, self.lof_upper, observed if self.struct.labels else None, expected)

    def write(self, out_prefix, result, k, written):
        written.append(indel_structure_simulation_output_name(out_prefix))
        write_indel_structure_simulation_outputs(*result[self.name], out_prefix)


class _CalibrationReducer:
    """The integer tables behind NLL / ECE / classwise ECE / Brier per chromosome and, with `fit_calibrator`, the retained rows and the
    calibrator fit on them at close()."""
    name = "calibration"

    def __init__(self, calibration, n_bins, fit_calibrator, fit_rows_max, fit_row_terms, calibrated, group, world):
        self.fit_calibrator, self.fit_rows_max, self.fit_row_terms = fit_calibrator, int(fit_rows_max), fit_row_terms
        if fit_calibrator is not None:
            if fit_calibrator not in CALIBRATORS:
                raise ValueError(f"unknown calibrator {fit_calibrator!r} (one of {sorted(CALIBRATORS)})")
            _refuse_fit_on_calibrated(calibrated)
        self.active = bool(calibration) or fit_calibrator is not None
        self.n_bins = int(n_bins)
        if self.active and self.n_bins < 1:
            raise ValueError(f"calibration_bins must be positive (got {n_bins})")
        self.bounds = calib_bounds(self.n_bins) if self.active else None
        self.group, self.world = group, world
        self.reset()

    def reset(self):
        self.host = {}                 # chromosome -> table uint64 [cells] of the host shards
        self.dev = {}                  # device -> ({chromosome: table}, status, bounds): read back once, at close()
        self.fit_blocks, self.fit_rows = [], 0      # [(prob float32 [n][n_class], label uint8 [n])], on a device or on the host
        self.sums = None

    def _table(self, tables, name, k):
        cells = calib_cells(k, self.n_bins)
        if cells > _CALIB_MAX_CELLS:
            raise ValueError(f"calibration_bins * (n_class + 1) = {self.n_bins * (k + 1)} is too large: the table of {cells} "
                             f"cells does not fit the {_CALIB_MAX_CELLS} a workgroup holds")
        if name not in tables:
            tables[name] = np.zeros(cells, np.uint64)
        return tables[name]

    def _retain(self, prob, label):
        """Keep a part's (float32 probabilities, uint8 labels -- 255 where the label is none) for the fit at close().  Every row of the
        part counts against `fit_rows_max`: an invalid row makes close() raise before anything is fitted."""
        if self.fit_rows + len(label) > self.fit_rows_max:
            raise ValueError(f"fit_calibrator={self.fit_calibrator!r}: this shard takes the rows retained on this rank from {self.fit_rows} to "
                             f"{self.fit_rows + len(label)}, beyond fit_rows_max={self.fit_rows_max}; raise the budget or fit on fewer rows "
                             "(nothing is subsampled silently)")
        self.fit_rows += len(label)
        self.fit_blocks.append((prob, label))

    def host_part(self, name, prob, start, end, strand, label, k):
        _, status = summary_calib_host(prob, label, k, self.n_bins, self.bounds, into=self._table(self.host, name, k))
        if self.fit_calibrator is not None:
            lab = np.asarray(label)
            good = np.isfinite(lab.astype(np.float64)) & (lab >= 0) & (lab < k) & (lab == np.floor(lab.astype(np.float64)))
            self._retain(np.ascontiguousarray(prob, np.float32), np.where(good, lab, 255).astype(np.uint8))
        return status

    def device_part(self, name, prob, start, end, strand, label, k):
        """Enqueue the metrics reduction of a part behind its forward -- one launch (and the fold of the carries) into the chromosome's
        accumulator on that device --, then the fit's copy of the part."""
        dev = prob.device
        acc = self.dev.get(dev)
        if acc is None:
            acc = self.dev[dev] = ({}, torch.zeros(1, dtype=torch.int32, device=dev), torch.from_numpy(self.bounds).to(dev))
        table = acc[0].get(name)
        if table is None:
            cells = len(self._table({}, name, k))
            table = acc[0][name] = torch.zeros(cells, dtype=torch.int64, device=dev)
        calib_rows_device(prob, label, k, self.n_bins, acc[2], table, acc[1])
        if self.fit_calibrator is not None:
            good = (label >= 0) & (label < k) & (label == label.to(torch.int64))
            self._retain(prob[:, :k].to(torch.float32, copy=True).contiguous(), torch.where(good, label, 255).to(torch.uint8))

    def read_back(self, k):
        status, mine = 0, [self.host]
        for tables, dev_status, _ in self.dev.values():
            status |= int(dev_status.item())
            mine.append({name: t.cpu().numpy().view(np.uint64) for name, t in tables.items()})
        return self._added([m for m in mine if m], k), status

    def _added(self, per_rank, k):
        """[{chromosome: table}] of the ranks (or of a rank's devices and its host rows) -> one such dict: integer tables added, carries
        folded."""
        out = {}
        for tables in per_rank:
            for name, t in tables.items():
                if name in out:
                    _calib_fold(np.add(out[name], t, out=out[name]), k, self.n_bins)
                else:
                    out[name] = t.copy()
        return out

    def merge(self, states, k):
        return self._added([s for s in states if s], k)

    def _total(self, per_chrom, k):
        total = np.zeros(calib_cells(k or 1, self.n_bins), np.uint64)
        for t in per_chrom.values():
            _calib_fold(np.add(total, t, out=total), k or 1, self.n_bins)
        return total

    def finish(self, state, k, result):
        per_chrom = state or {}
        total = self._total(per_chrom, k)
        self.sums = {"all": total, "per_chromosome": per_chrom}
        res = calib_metrics_from_sums(total, self.n_bins, k or 1)
        res["per_chromosome"] = {name: calib_metrics_from_sums(per_chrom[name], self.n_bins, k) for name in sorted(per_chrom)}
        result["calibration"] = res
        if self.fit_calibrator is not None:
            self._fit(res, k)

    def _block_terms(self, prob, label, w, need_hessian):
        """(loss sum, gradient sum, Hessian sum) of one retained block: the device kernel, or the stand-in given as `fit_row_terms`."""
        k = prob.shape[1]
        km = k * (k + 1)
        if self.fit_row_terms is not None:
            loss, g, h = self.fit_row_terms(_np(prob), _np(label), w, need_hessian)
            return np.r_[loss, np.ravel(g), np.ravel(h)]
        out = torch.zeros(1 + km + km * km, dtype=torch.float64, device=prob.device)
        status = torch.zeros(1, dtype=torch.int32, device=prob.device)
        wd = torch.from_numpy(np.ascontiguousarray(w, dtype=np.float64)).to(prob.device)
        with torch.cuda.device(prob.device):
            _lib.check(_lib.lib().mural_eval_dirichlet_fit_terms(prob.data_ptr(), 0, label.to(torch.int32).data_ptr(), prob.shape[0], k,
                                                                wd.data_ptr(), int(need_hessian), out.data_ptr(), status.data_ptr(),
                                                                _lib.current_stream_ptr(prob.device)))
        return out.cpu().numpy()

    def _fit(self, res, k):
        """Fit the named calibrator on the retained raw-softmax rows (training.py:478) and reduce the metrics of the calibrated rows
        through the same entry.  The data terms are the float64 atomic sums of ``mural_eval_dirichlet_fit_terms`` per block, added
        over blocks and -- one small all_reduce per evaluation -- over ranks: the weights are reproducible to rounding, not bit for bit.
        Only the metrics carry the bit-exact promise."""
        method, ref_row, reg_lambda, reg_mu, reg_norm = CALIBRATORS[self.fit_calibrator]
        if k is None or k < 2 or k > _FIT_MAX_CLASSES:
            raise ValueError(f"fit_calibrator supports 2..{_FIT_MAX_CLASSES} classes, got {k}")
        if any(c == 0 for c in res["label_counts"]):
            raise ValueError("every class 0..n_class-1 must occur in the labels (the reference sizes the map by unique(y))")
        if reg_norm:                                              # multinomial.py:81-86
            if reg_mu is None:
                reg_lambda = reg_lambda / (k * (k + 1))
            else:
                reg_lambda, reg_mu = reg_lambda / (k * (k - 1)), reg_mu / k
        if self.fit_row_terms is None:                            # host shards are uploaded now, beside the device blocks
            dev = next((p.device for p, _ in self.fit_blocks if isinstance(p, torch.Tensor)), None)
            dev = torch.device("cuda", torch.cuda.current_device()) if dev is None else dev
            self.fit_blocks = [(p, y) if isinstance(p, torch.Tensor) else (torch.from_numpy(p).to(dev), torch.from_numpy(y).to(dev))
                               for p, y in self.fit_blocks]
        km = k * (k + 1)
        n = res["rows"]

        def row_terms(w, need_hessian):
            sums = np.zeros(1 + km + km * km)
            for p, y in self.fit_blocks:
                sums += self._block_terms(p, y, w, need_hessian)
            if self.world > 1:
                t = torch.from_numpy(sums)                        # (shares its memory)
                if dist.get_backend(self.group) == "nccl":
                    t = t.cuda()
                dist.all_reduce(t, group=self.group)
                sums = t.cpu().numpy()
            return sums[0] / n, sums[1:1 + km] / n, sums[1 + km:].reshape(km, km) / n

        weights, loss = newton_calibrator(row_terms, k, method, ref_row, reg_lambda, reg_mu)
        after = {}
        bounds = {}
        for p, y in self.fit_blocks:
            if isinstance(p, torch.Tensor):
                dev = p.device
                if dev not in after:
                    after[dev] = (torch.zeros(calib_cells(k, self.n_bins), dtype=torch.int64, device=dev),
                                  torch.zeros(1, dtype=torch.int32, device=dev))
                    bounds[dev] = torch.from_numpy(self.bounds).to(dev)
                with torch.cuda.device(dev):
                    cal = calibrate_device(p, dirichlet_weights=weights, input_is_prob=True)
                    calib_rows_device(cal, y.to(torch.int32), k, self.n_bins, bounds[dev], *after[dev])
            else:
                summary_calib_host(dirichlet_calibrate(p, weights), y, k, self.n_bins, self.bounds, into=self._table(after, "host", k))
        tables = {key: (v if isinstance(v, np.ndarray) else v[0].cpu().numpy().view(np.uint64)) for key, v in after.items()}
        if self.world > 1:
            every = [None] * self.world
            dist.all_gather_object(every, tables, group=self.group)
            tables = {(r, key): t for r, ts in enumerate(every) for key, t in ts.items()}
        total = self._total(tables, k)
        self.sums["after"] = total
        res["after"] = calib_metrics_from_sums(total, self.n_bins, k)
        res["weights"], res["fit_loss"] = weights, float(loss)

    def write(self, out_prefix, result, k, written):
        res = result["calibration"]
        path = out_prefix + ".calibration.txt"
        written.append(path)
        line = lambda tag, m: "%s\t%d\t%.8f\t%.8f\t%.8f\t%.8f\n" % (tag, m["rows"], m["nll"], m["ece"], m["c_ece"], m["brier"])      # noqa: E731
        with open(path, "w") as fh:
            fh.write("chrom\trows\tnll\tece\tc_ece\tbrier\n" + line("all", res))
            if "after" in res:
                fh.write(line(f"all (after {self.fit_calibrator})", res["after"]))
            for name, m in res["per_chromosome"].items():
                fh.write(line(name, m))
        if "weights" in res:
            written.append(out_prefix + ".fdiri_cal.pkl")
            save_dirichlet_calibrator(res["weights"], written[-1])


class SummarySink:
    """Consumer of shards (the TsvSink protocol) that keeps no row: per window size of `windows` the table ``tables.regional_table``
    would read back from the written prediction table, and the (prob_sum, n_sites) of ``tables.prob_sum_file`` -- optionally counted per
    overlapping benchmark region (`benchmark_regions`: a BED path or ``tables.read_regions``' dict) --, reduced from the probabilities
    the table would hold, before they are rounded to four digits.  Device shards go through csrc/summary.hip (one pass per part, the
    tables of a part sized from its first and last start and merged on the host in arrival order; nothing waits for work just enqueued:
    a part is reduced when the next one arrives); host shards through numpy.  Calibration: as TsvSink (`poisson`, `dirichlet_weights`;
    refused for shards that are calibrated already).  ``parts=True`` under torch.distributed: every rank reduces its rows and close()
    gathers the ranks' tables -- not rows -- and adds them in rank order.

    close() writes, with an `out_prefix` and on rank 0, ``{out_prefix}.{W/1000}Kb.mut_rates.tsv`` / ``.corr.txt`` per window size
    (``tables.write_regional_outputs``: the files of ``evaluate --window_size``); ``result()`` and ``scaling_factor()`` are valid after
    it.

    `kmers`: k-mer lengths (1 .. ``tables.MAX_KMER``) whose rate tables -- ``tables.kmer_table``'s, the third thing ``evaluate`` reads
    from the written table -- are reduced as well (csrc/summary_kmer.hip: exact integer sums of the probabilities quantised to 2^-71,
    so the tables depend on the set of rows alone, bit for bit, whatever the parts, chunks or ranks).  `genome`: chromosome name ->
    packed genome (``HipShardForward.genome``; a sequence will do for host shards); `kmer_strand`: None for SNV rows (each row's own
    strand), 'pos' / 'neg' / 'both' for INDEL rows (``tables.strand_mode``).  A device part is reduced when it arrives, into accumulators
    that live with the sink and are read back once, at close(); ranks exchange the integer tables in the same collective.  close() then
    also writes ``{out_prefix}.{k}-mer.mut_rates.tsv`` / ``.corr.txt`` (``tables.write_kmer_outputs``), and result() has "kmers".

    `motifs`: motif lengths (odd, 3 .. ``tables.MAX_MOTIF``) whose rate tables -- ``tables.motif_table``'s, what ``evaluate --motif_only``
    reads from the written table -- are reduced the same way (``mural_summary_motif_rows``: every window of m bases that holds a row's
    site, on the reference strand, a motif and its reverse complement in one entry), alone or beside `kmers` and
    `windows`; `motif_indel`: the rows are INDEL rows (m - 1 windows each).  They need `genome` as well.  close() writes
    ``{out_prefix}.{m}-motif.mut_rates.tsv`` / ``.corr.txt`` (``tables.write_motif_outputs``), and result() has "motifs".

    `calibration`: the NLL / ECE / classwise ECE / Brier block of the reference's validation report (``calibrate_prob``,
    evaluation.py:297-365) from the rows' own labels, on `calibration_bins` bins, alone or beside the other summaries; it needs no
    `genome`.  Device parts go through ``mural_summary_calib_rows`` (csrc/summary_calib.hip), host shards through
    ``summary_calib_host``: integer tables per chromosome, read back once at close(), exchanged between ranks in the same collective and
    added -- the metrics depend on the set of rows alone, bit for bit.  result()["calibration"] = ``calib_metrics_from_sums`` of all rows
    + "per_chromosome": {name: the same}; close() writes ``{out_prefix}.calibration.txt`` (a header, an `all` line, a line per
    chromosome by name: rows nll ece c_ece brier, '%.8f'); ``calibration_sums()`` has the integers.

    `fit_calibrator`: a key of ``evaluation.CALIBRATORS`` ('FullDiri', ...) to fit on the same rows (training.py:478 fits the raw
    softmax, so the option is refused where the sink or the forward calibrates); it turns `calibration` on.  The sink retains (float32
    prob[n_class], uint8 label) of every row -- device parts in device blocks, host shards on the host until close() uploads them -- and
    raises ValueError at the shard that takes a rank beyond `fit_rows_max` retained rows; nothing is subsampled.  close() runs
    ``evaluation.newton_calibrator`` on the sums ``mural_eval_dirichlet_fit_terms`` makes of each block (all_reduced over the ranks, one
    small collective per evaluation), saves ``{out_prefix}.fdiri_cal.pkl`` on rank 0, calibrates the blocks and reduces their metrics
    through the same entry: result()["calibration"] gains "after", "weights" and "fit_loss", the text file an `all (after NAME)` line.
    The fit's sums are float64 atomics: the weights are reproducible to rounding, not bit for bit; only the metrics are bit-exact.
    `fit_row_terms`: (prob, label, weights, need_hessian) -> (loss, gradient, Hessian) SUMS over the given rows, a stand-in for the
    device kernel that keeps host shards on the host (tests without a device).

    `annotations`: a BED path or ``tables.read_annotations``' result: per NAME of the file (column 4; the exons of a gene share one) the
    observed mutations and the expected ones -- the label counts and the probability sums of the rows whose start lies in one of the
    name's intervals, which may be unsorted, overlap and nest --, alone or beside the other summaries; no `genome` is needed.  Device
    parts go through ``mural_summary_annot_rows`` (csrc/summary_annot.hip; DESIGN.md section 3.19: row prefix sums and one lookup per
    merged piece), host shards through ``summary_annot_host``: one integer table for the run, read back once at close(), exchanged
    between ranks in the same collective and added -- a function of the set of rows alone, bit for bit.  result()["annotations"] =
    (names, meta int64 [n][2] of n_intervals / length, table float64 [n][1 + 2 n_class] of rows / per-class counts / per-class
    probability sums); a name whose chromosomes never arrive stays, with zeros.  close() writes
    ``{out_prefix}.annotation.mut_rates.tsv`` / ``.corr.txt`` (``tables.write_annotation_outputs``); ``annotation_sums()`` has the
    integers.

    `simulate`: R replicates (1 .. 2^20) of the run's mutations drawn from its probabilities with `simulate_seed` (required: an unsigned
    64-bit integer; there is no default randomness).  The rule is ``simulate_rows_host``: stateless Philox
    draws keyed by (seed, chromosome, start, strand, replicate), so the results depend on the set of rows and the seed alone, bit for
    bit, for any parts, shards or ranks; two rows with the same chromosome, start and strand draw the same value.  With `annotations`
    the counts of every name, class and replicate are reduced beside the annotation table (``mural_simulate_annot_rows``,
    csrc/simulate.hip, on the pieces the annotation reducer uploaded; host shards through ``simulate_annot_host``) into one uint32 table
    [names][n_class - 1][R], refused with ValueError above `simulate_table_bytes_max` bytes (1 GiB: a stated cap, not a tuned value),
    read back once and added across ranks in the same collective.  close() writes ``{out_prefix}.annotation.sim.tsv``
    (``tables.write_simulation_outputs``: name, class, observed, expected, sim_mean, sim_min, sim_max, n_ge, n_le, p_upper = (n_ge + 1)
    / (R + 1), p_lower); `simulate_labels=False` says that the rows carry no labels: the observed column and the four after sim_max are
    NA.  result()["simulation"] = (names, counts, observed or None, expected); ``simulation_counts()`` has the table.
    `simulate_write`: replicates whose mutation lists -- the rows whose draw is not 0, in run order -- are written to
    ``{out_prefix}.sim{r}.mutations.bed`` (chrom start end name score strand, score = class: what ``data.read_mutations`` reads), device
    parts through ``mural_simulate_rows`` (compacted on the device; the lists of a part come to the host when the next part arrives).
    With ranks every rank writes ``....bed.part<rank>`` and rank 0 strings the parts together chromosome by chromosome in its own
    shard order, the ranks' parts of a chromosome in rank order.  The sink takes
    the chromosomes one after the other.

    `transcripts`: a BED12 path or ``tables.read_transcripts``' result: per transcript the expected and observed mutations of the SNV
    rows (4 classes) inside its CDS, split by what each of a row's three substitutions does to its codon -- synonymous, missense, stop
    gained, stop lost, or unresolved (an incomplete or masked codon) --, alone or beside the other summaries; it needs `genome`.
    `codon_table`: 64 characters indexed by 16 b0 + 4 b1 + b2 (A0 C1 G2 T3, '*' a stop; default the standard code); `alt_order`: the
    alternative base of class 1 .. 3 per own base (``tables.check_alt_order``; default the other bases in A < C < G < T order).  Device
    parts go through ``mural_summary_conseq_rows`` (csrc/summary_conseq.hip), host shards through
    ``summary_conseq_host``: one integer table for the run, read back once at close(), exchanged between ranks in the same collective and
    added -- a function of the set of rows alone, bit for bit.  result()["consequences"] = (names, meta, table float64 [n][12] of
    ``tables.consequence_table_from_sums``); close() writes ``{out_prefix}.consequence.mut_rates.tsv``
    (``tables.write_consequence_outputs``; `transcript_labels=False` says that the rows carry no labels: the observed columns are NA);
    ``consequence_sums()`` has the integers.
    `simulate_transcripts=True` (with `simulate`, `simulate_seed` and `transcripts`; opt-in: `simulate` beside `transcripts` alone
    draws nothing per transcript): the null distribution of the observed_* columns -- per transcript, consequence and replicate the
    rows inside the CDS whose draw is a class whose substitution has that consequence (``simulate_conseq_host`` is the rule; DESIGN.md
    section 3.22), device parts through ``mural_simulate_conseq_rows`` (csrc/simulate_conseq.hip) on the segment arrays the consequence
    reduction uploaded, one uint32 table [transcripts][5][R] (checked against `simulate_table_bytes_max` on its own) read back once and
    added across ranks in the same collective.  `simulate` then needs neither `annotations` nor `simulate_write`.
    result()["consequence_simulation"] = (names, counts, observed or None, expected), the last two [transcripts][4] from the
    consequence table; close() writes ``{out_prefix}.consequence.sim.tsv`` (``tables.write_consequence_simulation_outputs``);
    ``consequence_simulation_counts()`` has the table.
    `transcript_structure=True` (with `transcripts`: a BED12 path or ``tables.read_transcript_structure``'s result -- a
    ``read_transcripts`` triple holds no blocks any more; opt-in: without it nothing more is computed or written): a second table per
    transcript over every SNV row inside [chromStart, chromEnd), split into 5'UTR, 3'UTR, non-coding exon, splice donor, splice
    acceptor, splice site of a non-coding intron, intron, start lost and (other) CDS (``summary_txstruct_host`` is the rule; DESIGN.md
    section 3.23).  Device parts go through ``mural_summary_txstruct_rows`` (csrc/summary_txstruct.hip) on the segment arrays the
    consequence reduction uploaded and a chromosome's item arrays, uploaded once; one integer table pair per device, read back once
    and added across ranks in the same collective.  result()["transcript_structure"] = (names, table uint64 [n][9][3], rows uint64
    [n][2]); close() writes ``{out_prefix}.consequence.structure.tsv`` (``tables.write_structure_outputs``: the nine bins and
    expected_lof / observed_lof = stop gained + splice donor + splice acceptor + start lost); ``structure_sums()`` has the integers.
    `simulate_structure=True` (opt-in; with `simulate` and `simulate_seed`, `transcript_structure=True` and
    `simulate_transcripts=True`, ValueError naming what is missing otherwise): the null distribution of the structure table's
    observed_* columns and of observed_lof -- per transcript, structure bin and replicate the rows inside the span whose draw is a
    class that falls in that bin (``simulate_txstruct_host`` is the rule), device parts through
    ``mural_simulate_txstruct_rows`` (csrc/simulate_txstruct.hip) on the item and segment arrays the two reductions before it
    uploaded, one uint32 table [transcripts][9][R] (checked against `simulate_table_bytes_max` on its own) read back once and added
    across ranks in the same collective.  The LoF count of replicate r adds the stop-gained count of the consequence simulation and
    the donor, acceptor and start-lost counts of this table, all of the same draw (``simulate_lof_counts``).
    result()["structure_simulation"] = (names, counts [transcripts][9][R], lof [transcripts][R], observed [transcripts][10] or None,
    expected [transcripts][10]), the last two the structure file's own numbers, LoF last; close() writes
    ``{out_prefix}.consequence.structure.sim.tsv`` (``tables.write_structure_simulation_outputs``);
    ``structure_simulation_counts()`` has the table.

    `indel_transcripts`: a BED12 path or ``tables.read_transcript_structure``'s result, for INDEL rows (2 .. 16 classes; 8 on the
    device, as every summary here): per transcript the expected and observed INDEL events by what they do to the transcript -- utr5,
    utr3, noncoding_exon, splice, splice_utr, intron, start_lost, frameshift, inframe and cds_mixed (``summary_txindel_host`` is the
    rule) --, alone or beside the other summaries.  `indel_kind` (required): 'insertion', 'deletion_start' or
    'deletion_end', of the whole run -- there is one model per kind; `indel_lengths`: the lengths each class >= 1 stands for
    (``tables.check_indel_lengths``; default "1,2,3,4,5,6,7-20" for 8 classes, any other class count needs it); `breakpoint_offset`: 0
    or 1 (default), the event's boundary is start + breakpoint_offset.  No base is read; with `genome` a deletion is clipped to the
    chromosome's length as well.  Device parts go through ``mural_summary_txindel_rows`` (csrc/summary_txindel.hip) on a chromosome's
    item, link and segment arrays, uploaded once; one integer table pair per device, read back once and added across ranks in the
    same collective -- a function of the set of rows alone, bit for bit.  result()["indel_structure"] = (names, table uint64 [n][10][3],
    rows uint64 [n][2]); close() writes ``{out_prefix}.indel_structure.tsv`` (``tables.write_indel_structure_outputs``: the ten bins,
    expected_lof / observed_lof = splice + start lost + frameshift and the _upper pair = that + cds_mixed; `transcript_labels=False`:
    the observed columns are NA); ``indel_structure_sums()`` has the integers.  `transcripts=` keeps refusing rows of other than 4
    classes.
    `simulate_indel_structure=True` (opt-in; with `simulate` and `simulate_seed`, `indel_transcripts` and `indel_kind`, ValueError
    naming what is missing otherwise; `simulate` then needs neither `annotations` nor `simulate_write`): the null distribution of the
    INDEL structure table's observed_* columns and of observed_lof / observed_lof_upper -- per transcript, bin and replicate the rows
    the transcript counts whose draw is a class that falls in that bin (``simulate_txindel_host`` is the rule; DESIGN.md section
    3.26; 2 .. 8 classes), device parts through ``mural_simulate_txindel_rows`` (csrc/simulate_txindel.hip) on the item, link and
    segment arrays the reduction before it uploaded, one uint32 table [transcripts][10][R] (checked against
    `simulate_table_bytes_max` on its own, when the sink is built) read back once and added across ranks in the same collective.
    The LoF counts of replicate r add the splice, start-lost and frameshift counts (and cds_mixed for the upper one) of the same
    draw (``simulate_indel_lof_counts``).  result()["indel_structure_simulation"] = (names, counts [transcripts][10][R], lof
    [transcripts][R], lof_upper [transcripts][R], observed [transcripts][12] or None, expected [transcripts][12]), the last two the
    INDEL structure file's own numbers, lof and lof_upper last; close() writes ``{out_prefix}.indel_structure.sim.tsv``
    (``tables.write_indel_structure_simulation_outputs``); ``indel_structure_simulation_counts()`` has the table.

    The sink checks the shard, calibrates and orders the part and hands its columns to the reducer of every summary asked for; close()
    reads the reducers back, exchanges the ranks' states in ONE collective and lets each reducer merge, finish and write its own."""

    takes_aligned_blocks = True

    def __init__(self, out_prefix=None, windows=(), benchmark_regions=None, ratio_cutoff=0.2, poisson=False, dirichlet_weights=None,
                 group=None, parts=False, kmers=(), genome=None, kmer_strand=None, motifs=(), motif_indel=False, calibration=False,
                 calibration_bins=50, fit_calibrator=None, fit_rows_max=1 << 27, fit_row_terms=None, annotations=None, simulate=None,
                 simulate_seed=None, simulate_write=(), simulate_table_bytes_max=1 << 30, simulate_labels=True, transcripts=None,
                 codon_table=None, alt_order=None, transcript_labels=True, simulate_transcripts=False, transcript_structure=False,
                 simulate_structure=False, indel_transcripts=None, indel_kind=None, indel_lengths=None, breakpoint_offset=1,
                 simulate_indel_structure=False):
        self.out_prefix = None if out_prefix is None else os.fspath(out_prefix)
        by_window = _WindowReducer(windows, benchmark_regions, ratio_cutoff)
        self.windows = by_window.sizes
        self.ratio_cutoff, self.poisson, self.dirichlet_weights, self.group = ratio_cutoff, poisson, dirichlet_weights, group
        self.rank = dist.get_rank(group) if (parts and dist.is_initialized()) else 0
        self.world = dist.get_world_size(group) if (parts and dist.is_initialized()) else 1
        self.parts = self.world > 1
        by_kmer = _KeyedReducer(_KMERS, kmers, genome)
        by_kmer.fields = dict(indel=int(kmer_strand is not None), mode=strand_mode("indel", kmer_strand) if kmer_strand is not None else 0)
        by_motif = _KeyedReducer(_MOTIFS, motifs, genome)
        by_motif.fields = dict(indel=int(bool(motif_indel)), order_by_row=0)
        self.kmers, self.motifs = by_kmer.lengths, by_motif.lengths
        metrics = _CalibrationReducer(calibration, calibration_bins, fit_calibrator, fit_rows_max, fit_row_terms,
                                      poisson or dirichlet_weights is not None, group, self.world)
        self.fit_calibrator, self.fit_rows_max = fit_calibrator, metrics.fit_rows_max
        self.calibration, self.calibration_bins = metrics.active, metrics.n_bins
        # the reducers of the summaries asked for, in the order of their files; the totals go with the windows, so those always run
        active = [by_window] + [r for r, on in ((by_kmer, self.kmers), (by_motif, self.motifs), (metrics, self.calibration)) if on]
        self.annotations = annotations is not None
        if self.annotations:
            active.append(_AnnotationReducer(annotations))
        self.simulate = simulate is not None
        if simulate_structure:      # opt-in, and only on top of the three it builds on
            missing = [what for what, on in (("simulate=R with simulate_seed", simulate is not None and simulate_seed is not None),
                                             ("transcript_structure=True (the item arrays)", transcript_structure and transcripts is not None),
                                             ("simulate_transcripts=True (the stop-gained counts of the same draws)",
                                              simulate_transcripts and transcripts is not None)) if not on]
            if missing:
                raise ValueError("simulate_structure needs " + ", ".join(missing))
        if simulate_indel_structure:      # opt-in as well, behind the INDEL structure reducer
            missing = [what for what, on in (("simulate=R with simulate_seed", simulate is not None and simulate_seed is not None),
                                             ("indel_transcripts= with indel_kind= (the item arrays and the bin rule)",
                                              indel_transcripts is not None and indel_kind is not None)) if not on]
            if missing:
                raise ValueError("simulate_indel_structure needs " + ", ".join(missing))
        if self.simulate:
            if simulate_seed is None:
                raise ValueError("simulate needs simulate_seed: there is no default randomness")
            if annotations is None and not tuple(simulate_write) and not simulate_transcripts and not simulate_indel_structure:
                raise ValueError("simulate needs annotations= (the counts per name) or a replicate in simulate_write")
            if self.annotations or tuple(simulate_write):      # (otherwise the draws are the consequence simulation's alone)
                active.append(_SimulationReducer(simulate, simulate_seed, simulate_write, active[-1] if self.annotations else None,
                                                 simulate_table_bytes_max, self.out_prefix, simulate_labels, self.rank, self.world))
        elif simulate_seed is not None or tuple(simulate_write):
            raise ValueError("simulate_seed and simulate_write go with simulate=R")
        self.transcripts = transcripts is not None
        if transcript_structure and not self.transcripts:
            raise ValueError("transcript_structure goes with transcripts= (a BED12 path or tables.read_transcript_structure's result)")
        if self.transcripts:
            features = None
            if transcript_structure:
                *transcripts, features = read_transcript_structure(transcripts, codon_table)
                transcripts = tuple(transcripts)
            elif isinstance(transcripts, tuple) and len(transcripts) == 4:
                transcripts = transcripts[:3]
            by_tx = _ConsequenceReducer(transcripts, genome, codon_table, alt_order, transcript_labels)
            active.append(by_tx)
            if simulate_transcripts and self.simulate:      # behind the consequence reducer: it uploads the segment arrays
                active.append(_ConsequenceSimulationReducer(simulate, simulate_seed, by_tx, simulate_table_bytes_max))
            if features is not None:                        # behind it as well
                active.append(_StructureReducer(features, by_tx))
            if simulate_structure:                          # behind both: the item arrays, and the stop-gained counts of the same draws
                active.append(_StructureSimulationReducer(simulate, simulate_seed, active[-1], active[-2], simulate_table_bytes_max))
        elif codon_table is not None or alt_order is not None:
            raise ValueError("codon_table and alt_order go with transcripts=")
        if simulate_transcripts and not self.transcripts:
            raise ValueError("simulate_transcripts goes with transcripts= (and simulate=R)")
        if simulate_transcripts and not self.simulate:
            raise ValueError("simulate_transcripts goes with simulate=R and simulate_seed")
        if indel_transcripts is not None:
            active.append(_IndelStructureReducer(indel_transcripts, indel_kind, indel_lengths, breakpoint_offset, genome, transcript_labels))
            if simulate_indel_structure:      # behind it: its item, link and segment arrays and its workspace
                active.append(_IndelStructureSimulationReducer(simulate, simulate_seed, active[-1], simulate_table_bytes_max))
        elif indel_kind is not None or indel_lengths is not None or breakpoint_offset != 1:
            raise ValueError("indel_kind, indel_lengths and breakpoint_offset go with indel_transcripts=")
        self._reducers = {r.name: r for r in active}
        self.rows = 0
        self._n_class = None
        self._status = 0
        self._written = []
        self._result = None

    @property
    def _pending(self):
        """The staged device part of the window reduction (None between parts on the host)."""
        return self._reducers["windows"].pending

    # -- one part ---------------------------------------------------------------------------------------------------------
    def _host_part(self, name, shard, k):
        """Calibrate and order the part, reduce it in every reducer."""
        prob = host_calibrate(np.asarray(shard["prob"])[:, :k], self.poisson, self.dirichlet_weights)
        start = np.asarray(shard["start"])
        cols = [prob, start, np.asarray(shard["end"]), strand_u8(shard["strand"]) if (self.kmers or self.simulate or self.transcripts) else None,
                np.asarray(shard["label"])]
        if not shard.get("aligned"):
            perm = np.argsort(start, kind="stable")
            if self.parts:
                perm = perm[slice(*shard_bounds(len(perm), self.rank, self.world))]
            cols = [c if c is None else c[perm] for c in cols]
        for r in self._reducers.values():
            self._status |= r.host_part(name, *cols, k)

    def _device_part(self, name, shard, k):
        """Calibrate and order the part on its device, enqueue every reducer's work behind this part's forward: the fixed-size tables
        (k-mers, motifs, calibration) now, while this part's chromosome is the resident one; the windows last -- they stage this part and
        reduce the one before it."""
        prob = shard["prob"]
        dev = prob.device
        with torch.cuda.device(dev):
            if self.dirichlet_weights is not None or self.poisson:
                prob = calibrate_device(prob[:, :k].contiguous() if prob.stride(0) != k else prob, dirichlet_weights=self.dirichlet_weights,
                                        poisson=self.poisson, input_is_prob=True)
            if prob.dtype not in (torch.float32, torch.float64):
                prob = prob.to(torch.float32)
            if prob.stride(1) != 1:
                prob = prob.contiguous()
            to = lambda a, dt: (a if isinstance(a, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(a))).to(dev, dt).contiguous()   # noqa: E731
            start, end = to(shard["start"], torch.int64), to(shard["end"], torch.int64)
            label = shard["label"]
            label = to(label, label.dtype if isinstance(label, torch.Tensor) and label.dtype in (torch.int32, torch.int64) else torch.float32)
            strand = to(strand_u8(shard["strand"]), torch.uint8) if (self.kmers or self.simulate or self.transcripts) else None
            if not shard.get("aligned"):
                perm = torch.sort(start, stable=True).indices
                if self.parts:
                    perm = perm[slice(*shard_bounds(perm.shape[0], self.rank, self.world))]
                prob, start, end, label = prob[perm], start[perm], end[perm], label[perm]
                strand = strand[perm] if strand is not None else None
            cols = (name, prob, start, end, strand, label, k)
            held = None
            by_window, *others = self._reducers.values()
            if start.shape[0]:
                for r in others:
                    keep = r.device_part(*cols)
                    held = held if keep is None else keep
        by_window.device_part(*cols, held=held)

    def __call__(self, shard):
        name = shard_name(shard)
        n = len(shard["start"])
        if name is None or n == 0:
            return
        _refuse_second_calibration(shard, self.poisson, self.dirichlet_weights)
        if self.fit_calibrator is not None:
            _refuse_fit_on_calibrated(shard.get("calibrated"))
        k = int(shard.get("n_class", shard["prob"].shape[1]))
        if self._n_class not in (None, k):
            raise ValueError(f"shards of {self._n_class} and of {k} classes in one summary")
        self._n_class = k
        self.rows += n
        if isinstance(shard["prob"], torch.Tensor) and shard["prob"].is_cuda:
            if k > 8:
                raise ValueError("SummarySink reduces at most 8 classes on the device")
            self._device_part(name, shard, k)
        else:
            if isinstance(shard["prob"], torch.Tensor):
                shard = dict(shard, prob=shard["prob"].numpy())
            self._host_part(name, {key: (_np(v) if isinstance(v, torch.Tensor) else v) for key, v in shard.items()}, k)

    # -- close ------------------------------------------------------------------------------------------------------------
    def close(self):
        state = {"n_class": self._n_class}
        for r in self._reducers.values():
            state[r.name], status = r.read_back(self._n_class)
            self._status |= status
        state["status"] = self._status
        k = self._n_class
        if self.world > 1:
            every = [None] * self.world
            dist.all_gather_object(every, state, group=self.group)      # the one collective: tables, not rows
            k = next((st["n_class"] for st in every if st["n_class"] is not None), None)
            state = {r.name: r.merge([st[r.name] for st in every], k) for r in self._reducers.values()}
            state["status"] = 0
            for st in every:
                state["status"] |= st["status"]
        for bit, what in _SUMMARY_STATUS:
            if state["status"] & bit:
                raise ValueError(f"summary: {what}")
        self._result = {}
        for r in self._reducers.values():
            r.finish(state[r.name], k, self._result)
        if self.out_prefix is not None and self.rank == 0 and k is not None:
            for r in self._reducers.values():
                r.write(self.out_prefix, self._result, k, self._written)

    def abort(self):
        """Drop what was reduced and remove any file close() began: the caller's run failed."""
        for r in self._reducers.values():
            r.reset()
        self._result = None
        for path in self._written:
            if os.path.exists(path):
                os.unlink(path)
        self._written = []

    def result(self):
        """{"prob_sum", "n_sites", "windows": {W: ([(chrom, window_end)], table [windows][1 + 2 n_class])}} after close(): the pair of
        ``tables.prob_sum_file`` and, per window size, of ``tables.regional_table`` (chromosomes by name, windows ascending); with `kmers`
        also "kmers": {k: (names, table [k-mers][1 + 2 n_class])}, the pair of ``tables.kmer_table``, and with `motifs` "motifs": {m: the
        pair of ``tables.motif_table``}, with `calibration` "calibration": ``calib_metrics_from_sums``' dict of all rows + "per_chromosome"
        (and "after", "weights", "fit_loss" with `fit_calibrator`).  ``kmer_sums()``, ``motif_sums()`` and ``calibration_sums()`` have the
        integers."""
        if self._result is None:
            raise RuntimeError("SummarySink.result() is valid after close()")
        return self._result

    def kmer_sums(self):
        """{k: (table uint64 [4^k][3][n_class] of label counts | sums of hi | sums of lo, first uint64 [4^k])} after close(): the exact
        sums behind result()["kmers"] (``summary_kmer_host``'s layout)."""
        self.result()
        return self._reducers["kmers"].sums

    def motif_sums(self):
        """{m: (table uint64 [4^m][3][n_class], first uint64 [4^m])} after close(): the exact sums behind result()["motifs"]
        (``summary_motif_host``'s layout, the chromosome's ordinal by name above each first-appearance word)."""
        self.result()
        return self._reducers["motifs"].sums

    def annotation_sums(self):
        """table uint64 [names][3][n_class] of label counts | sums of hi | sums of lo after close(): the exact sums behind
        result()["annotations"] (``summary_annot_host``'s layout, the names in ``read_annotations``' order)."""
        self.result()
        return self._reducers["annotations"].sums

    def consequence_sums(self):
        """(table uint64 [transcripts][5][3] of label counts | sums of hi | sums of lo per bin, rows uint64 [transcripts][2]) after close():
        the exact sums behind result()["consequences"] (``summary_conseq_host``'s layout, the transcripts in file order)."""
        self.result()
        return self._reducers["consequences"].sums

    def structure_sums(self):
        """(table uint64 [transcripts][9][3] of label counts | sums of hi | sums of lo per bin of ``tables.STRUCTURE_BINS``, rows uint64
        [transcripts][2]) after close(): ``summary_txstruct_host``'s layout, the transcripts in file order."""
        self.result()
        return self._reducers["transcript_structure"].sums

    def indel_structure_sums(self):
        """(table uint64 [transcripts][10][3] of label counts | sums of hi | sums of lo per bin of ``tables.INDEL_STRUCTURE_BINS``, rows
        uint64 [transcripts][2]) after close(): ``summary_txindel_host``'s layout, the transcripts in file order."""
        self.result()
        return self._reducers["indel_structure"].sums

    def simulation_counts(self):
        """table uint32 [names][n_class - 1][simulate] after close(): the simulated count of every name, class >= 1 and replicate
        (``simulate_annot_host``'s layout, the names in ``read_annotations``' order)."""
        self.result()
        return self._reducers["simulation"].counts

    def consequence_simulation_counts(self):
        """table uint32 [transcripts][5][simulate] after close(): the simulated count of every transcript, consequence bin (0 syn, 1
        mis, 2 stop gained, 3 stop lost, 4 unresolved) and replicate (``simulate_conseq_host``'s layout, the transcripts in file order)."""
        self.result()
        return self._reducers["consequence_simulation"].counts

    def structure_simulation_counts(self):
        """table uint32 [transcripts][9][simulate] after close(): the simulated count of every transcript, structure bin of
        ``tables.STRUCTURE_BINS`` and replicate (``simulate_txstruct_host``'s layout, the transcripts in file order)."""
        self.result()
        return self._reducers["structure_simulation"].counts

    def indel_structure_simulation_counts(self):
        """table uint32 [transcripts][10][simulate] after close(): the simulated count of every transcript, bin of
        ``tables.INDEL_STRUCTURE_BINS`` and replicate (``simulate_txindel_host``'s layout, the transcripts in file order)."""
        self.result()
        return self._reducers["indel_structure_simulation"].counts

    def calibration_sums(self):
        """{"all": table, "per_chromosome": {name: table}[, "after": table]} after close(): the integer tables behind
        result()["calibration"] (``summary_calib_host``'s layout)."""
        self.result()
        return self._reducers["calibration"].sums

    def scaling_factor(self, genomewide_mu, m_proportion, g_proportion=1.0):
        """``tables.calc_mu_scaling_factor``'s factor for the summarised rows, with the lines it prints."""
        res = self.result()
        factor = mu_scaling_factor(genomewide_mu, res["n_sites"], m_proportion, g_proportion, res["prob_sum"])
        print_scaling_factor(genomewide_mu, res["n_sites"], g_proportion, m_proportion, res["prob_sum"], factor)
        return factor


