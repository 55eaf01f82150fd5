"""Sharded genome-wide prediction: one process per GPU, sites split into contiguous blocks, ONE RCCL all_gather of the
per-rank probabilities per call (the reference itself is single-process and only advises to
split the BED file by hand, MuRaL/commands/predict.py:134-137).

The host logic (block partition, padded all_gather, trimming back to the reference's row order) is backend-agnostic
and covered by world_size-2 gloo tests on CPU; the compute function is the HIP model's ``forward_packed`` /
``forward_packed_reuse``; the prediction table is formatted by ``csrc/tsv.hip`` (device kernel or host threads).
"""
import contextlib
import ctypes as C
import os
import queue
import re
import threading
import time

import numpy as np
import torch
import torch.distributed as dist

from . import _lib


def shard_bounds(n, rank, world):
    """Contiguous block [lo, hi) of `n` rows for `rank`: the first n % world ranks take one extra row."""
    if world <= 0 or not (0 <= rank < world):
        raise ValueError(f"bad rank/world {rank}/{world}")
    base, extra = divmod(n, world)
    lo = rank * base + min(rank, extra)
    return lo, lo + base + (1 if rank < extra else 0)


def all_gather_rows(local, n_total, group=None):
    """Gather row blocks of unequal length (block partition of shard_bounds) into the full (n_total, C) tensor on
    every rank with a single all_gather_into_tensor of equally padded blocks."""
    world = dist.get_world_size(group) if dist.is_initialized() else 1
    if world == 1:
        if local.shape[0] != n_total:
            raise ValueError("single-process gather expects all rows")
        return local
    width = local.shape[1]
    per = (n_total + world - 1) // world                       # longest block
    padded = torch.zeros((per, width), dtype=local.dtype, device=local.device)
    padded[: local.shape[0]] = local
    gathered = torch.empty((world * per, width), dtype=local.dtype, device=local.device)
    dist.all_gather_into_tensor(gathered, padded, group=group)
    if n_total == world * per:
        return gathered
    out = torch.empty((n_total, width), dtype=local.dtype, device=local.device)
    for r in range(world):
        lo, hi = shard_bounds(n_total, r, world)
        out[lo:hi] = gathered[r * per: r * per + (hi - lo)]
    return out


class OverlappedGather:
    """The per-step collective of a weak-scaling run (every rank contributes `rows` rows per step, every rank ends the step with all
    of them) issued asynchronously into one of TWO buffers: the all-gather of step s runs on the collective's stream while step s + 1
    is computed; a buffer is waited for when it comes up again and at ``finish()``.  Same bytes as a blocking
    ``all_gather_into_tensor`` per step; on xGMI the 64 MB of an 8-rank step then hide behind the next step's 29 ms of compute instead
    of adding to them."""

    def __init__(self, rows, width, dtype, device, group=None):
        self.group = group
        self.world = dist.get_world_size(group)
        self.bufs = [torch.empty((self.world * rows, width), dtype=dtype, device=device) for _ in range(2)]
        self.works = [None, None]
        self.turn = 0

    def submit(self, local):
        """Start gathering `local` (rows, width); returns the index of the buffer that will hold the step's rows."""
        i = self.turn
        self.turn ^= 1
        if self.works[i] is not None:
            self.works[i][0].wait()
        # (the source stays referenced until its collective was waited for)
        self.works[i] = (dist.all_gather_into_tensor(self.bufs[i], local.contiguous(), group=self.group, async_op=True), local)
        return i

    def finish(self):
        for w in self.works:
            if w is not None:
                w[0].wait()
        self.works = [None, None]

    def result(self, i):
        return self.bufs[i]


def predict_sites(forward_fn, pos, strand, group=None, steps=1):
    """Run `forward_fn(pos_block, strand_block) -> (rows, n_class)` on this rank's block of sites and return the
    full (N, n_class) result in input order on every rank.  `pos` / `strand` hold ALL sites on every rank (they are
    8 + 1 bytes per site; the genome and the weights are replicated).  The block is evaluated in `steps` slices (bounded
    workspace; the benchmark's timed steps) and ends with ONE all_gather of the whole block."""
    world = dist.get_world_size(group) if dist.is_initialized() else 1
    rank = dist.get_rank(group) if dist.is_initialized() else 0
    n = pos.shape[0]
    lo, hi = shard_bounds(n, rank, world)
    parts = []
    for k in range(max(int(steps), 1)):
        a, b = shard_bounds(hi - lo, k, max(int(steps), 1))
        parts.append(forward_fn(pos[lo + a:lo + b], strand[lo + a:lo + b]))
    local = parts[0] if len(parts) == 1 else torch.cat(parts)
    if local.shape[0] != hi - lo:
        raise RuntimeError("forward_fn returned a wrong number of rows")
    return all_gather_rows(local, n, group)


def verify_gathered_rows(forward_fn, pos, strand, full, sample=4096, seed=0):
    """Recompute a random sample of rows of a gathered result on THIS rank alone and compare: (largest absolute difference,
    rows checked, ranks whose blocks the sample touched).  The sample is drawn over all rows, i.e. over every rank's block, so a
    collective that scrambles, drops or pads blocks shows up here; per-site results do not depend on batch composition, so the
    expected difference is exactly 0."""
    world = dist.get_world_size() if dist.is_initialized() else 1
    n = pos.shape[0]
    if n == 0:
        return 0.0, 0, 0
    g = torch.Generator().manual_seed(seed)
    idx = torch.randperm(n, generator=g)[:min(sample, n)].sort().values
    dev_idx = idx.to(pos.device)
    mine = forward_fn(pos[dev_idx], strand[dev_idx])
    diff = float((mine.double() - full[dev_idx].double()).abs().max())
    owners = {r for r in range(world) if ((idx >= shard_bounds(n, r, world)[0]) & (idx < shard_bounds(n, r, world)[1])).any()}
    return diff, int(idx.numel()), len(owners)


class ShardedPredictor:
    """Convenience wrapper binding a HIP model and a resident PackedGenome."""

    def __init__(self, model, genome, local_radius, local_order=3, group=None):
        self.model, self.genome = model, genome
        self.local_radius, self.local_order, self.group = local_radius, local_order, group

    @torch.no_grad()
    def __call__(self, pos, strand):
        fn = lambda p, s: self.model.forward_packed(self.genome, p, s, self.local_radius, self.local_order)
        return predict_sites(fn, pos, strand, self.group)


# ------------------------------------------------------------------------------------------------------------------
# File-level sharded prediction (BASELINE config 5: whole-genome predict on 8 ranks).  Counterpart of the reference's advice
# to split a big BED by hand and run several `predict` processes (MuRaL/commands/predict.py:134-137) around the loop of
# MuRaL/scripts/run_predict.py:188-239.
#
#   * rows keep their bed_reader order (preprocessing.py:39-106); one SHARD = all rows of one chromosome (its runs in that
#     order, concatenated), and the shards are processed in ascending chromosome NAME order -- the order of the final
#     sort_values(['chrom', 'start']) -- so the table can be streamed out shard by shard;
#   * per shard only that chromosome is packed and resident in HBM (<= 70 MB for a human chromosome); the next chromosome is
#     packed on a host thread while this one is computed, and every chromosome is packed exactly once;
#   * rank i evaluates the contiguous block shard_bounds(rows of the shard, i, world), through the cross-position reuse kernels
#     where the block's sites are dense along the chromosome and through the per-window kernels elsewhere;
#   * ONE all_gather per shard returns (rows, n_class + 1): the probabilities and the strand-complemented focal base that the
#     reference's per-(segment, strand) consistency check needs (preprocessing.py:479-484, always run by prepare_local_data
#     :400 with local_order=1) -- groups may straddle rank boundaries, so the check (a streaming kernel) runs on the gathered
#     shard; its verdict is read one shard late, so no rank waits for it;
#   * rank 0 hands the gathered shard to a sink; TsvSink sorts it by start on the device, formats the text rows on the device
#     (csrc/tsv.hip) and leaves the copy to the host and the write() to a writer thread: no rank waits for the writer unless
#     all of its text buffers are full.
# With a host-memory forward (gloo ranks, CPU tests) the same driver runs on numpy arrays and the host formatter.
# ------------------------------------------------------------------------------------------------------------------
def shard_runs(chrom_id):
    """[(lo, hi)] runs of equal chromosome id in a row sequence."""
    chrom_id = np.asarray(chrom_id)
    if len(chrom_id) == 0:
        return []
    cut = np.r_[0, np.nonzero(chrom_id[1:] != chrom_id[:-1])[0] + 1, len(chrom_id)]
    return list(zip(cut[:-1].tolist(), cut[1:].tolist()))


_FOCAL_MSG = ("The positions in input BED file have different bases (A/T and C/G mixed)! The ref_genome or "
              "input BED file could be wrong.")


def check_focal_groups(focal, group):
    """The reference's 'different bases' check: every (segment, strand) group of bed_reader shares one focal base after
    strand complement.  `group` ids are non-decreasing.  Raises ValueError (the reference exits)."""
    focal, group = np.asarray(focal), np.asarray(group)
    if len(focal) == 0:
        return
    first = np.r_[True, group[1:] != group[:-1]]
    ref = focal[np.maximum.accumulate(np.where(first, np.arange(len(focal)), 0))]
    if (focal != ref).any():
        raise ValueError(_FOCAL_MSG)


class FastaGenomes:
    """The chromosomes of a FASTA file on a HIP device, one at a time: packed from the file (C++ packer; the next one on a host thread
    while this one is in use) and uploaded by genome(chrom), which drops the previous one.  A `genome_from` (anything with records /
    prefetch / genome) takes over all three: this object then neither reads the file nor packs or uploads anything."""

    def _init_genomes(self, fasta_path, device, genome_from=None):
        from .data import ingest
        self._ingest = ingest
        self.fasta_path, self.device = fasta_path, torch.device(device)
        if self.device.index is None:
            self.device = torch.device("cuda", torch.cuda.current_device())
        self.genome_from = genome_from
        self._records, self._scan_error, self._early = None, None, None
        self._scan = None
        if genome_from is None and fasta_path is not None:
            # the FASTA index (record offsets: one pass over the file) is built on a host thread -- the C++ scanner releases the GIL --
            # so the driver reads the BED beside it; `records` joins
            self._scan = threading.Thread(target=self._scan_fasta, daemon=True)
            self._scan.start()
        self._resident = (None, None)
        self._prefetch = None          # (chrom, thread, result box)
        self.seconds = {"pack_wait": 0.0, "pack": 0.0}

    def _source(self):
        if self.genome_from is None and self._scan is None:
            raise RuntimeError("this forward was built without a FASTA file (fasta_path=None): it takes its chromosomes from the "
                               "ModelSetForward it becomes a member of, or from genome_from=")
        return self.genome_from

    def _scan_fasta(self):
        try:
            self._records = {r.name: r for r in self._ingest.scan_fasta(self.fasta_path)}
        except Exception as e:      # noqa: BLE001  (re-raised by `records`)
            self._scan_error = e
            return
        # shards come in ascending chromosome-name order, so the first one is most likely the smallest name of the file: pack it
        # right away (still beside the driver's BED read); a BED without that chromosome just leaves the box unused
        if self._records:
            first = min(self._records)
            box = {}
            t0 = time.perf_counter()
            try:
                box["packed"] = self._ingest.pack_fasta_record(self.fasta_path, self._records[first])
            except Exception as e:      # noqa: BLE001  (re-raised by genome())
                box["error"] = e
            box["seconds"] = time.perf_counter() - t0
            self._early = (first, box)

    @property
    def records(self):
        if self._source() is not None:
            return self.genome_from.records
        self._scan.join()      # a finished thread joins at once; safe from the packer thread as well
        if self._scan_error is not None:
            raise self._scan_error
        return self._records

    # -- chromosome residency ---------------------------------------------------------------------------------------------
    def _pack(self, chrom, box):
        t0 = time.perf_counter()
        try:
            box["packed"] = self._ingest.pack_fasta_record(self.fasta_path, self.records[chrom])
        except Exception as e:      # noqa: BLE001  (re-raised by the consumer)
            box["error"] = e
        box["seconds"] = time.perf_counter() - t0

    def prefetch(self, chrom):
        """Start packing `chrom` on a host thread (the C++ packer releases the GIL); genome(chrom) picks the result up."""
        if self._source() is not None:
            return self.genome_from.prefetch(chrom)
        if chrom is None or chrom not in self.records or self._resident[0] == chrom:
            return
        if self._prefetch is not None and self._prefetch[0] == chrom:
            return
        if self._early is not None and self._early[0] == chrom:      # the scan thread already packed it
            return
        box = {}
        th = threading.Thread(target=self._pack, args=(chrom, box), daemon=True)
        th.start()
        self._prefetch = (chrom, th, box)

    def genome(self, chrom):
        if self._source() is not None:
            return self.genome_from.genome(chrom)
        if self._resident[0] != chrom:
            self._resident = (None, None)              # drop the previous chromosome before the next one is uploaded
            if chrom not in self.records:
                raise KeyError(chrom)                  # the reference's seq_records[chrom] lookup
            t0 = time.perf_counter()
            if self._prefetch is not None and self._prefetch[0] == chrom:
                _, th, box = self._prefetch
                th.join()
                self._prefetch = None
            elif self._early is not None and self._early[0] == chrom:      # packed by the scan thread (records joined it above)
                box, self._early = self._early[1], None
            else:
                box = {}
                self._pack(chrom, box)
            self.seconds["pack_wait"] += time.perf_counter() - t0
            self.seconds["pack"] += box.get("seconds", 0.0)
            if "error" in box:
                raise box["error"]
            packed, mask, n, amb = box["packed"]
            from .data.genome import PackedGenome
            self._resident = (chrom, PackedGenome(packed, mask, n, self.device, amb))
            self._early = None                         # an unused early pack is dropped with the first resident chromosome
        return self._resident[1]


class HipShardForward(FastaGenomes):
    """Default compute of predict_bed_sharded: packs the shard's chromosome from the FASTA file (C++ packer; the next one on a
    host thread while this one is computed), keeps exactly one chromosome resident, runs the fused packed-genome forward and
    returns softmax probabilities with the focal base appended as the last column."""

    REUSE_MIN_DENSITY = 0.1        # sites per base of a chunk's span above which the cross-position reuse path pays

    def __init__(self, model, fasta_path, local_radius, local_order=3, distal_radius=None, device="cuda", batch_sites=1 << 20,
                 model_type="snv", dirichlet_weights=None, poisson=None, scale_factor=None, reuse=True, genome_from=None):
        """`dirichlet_weights` / `poisson` / `scale_factor`: apply the post-head calibration chain of run_predict.py:217-225
        (and scripts/scaling.py) on the device, fused behind the head (calibration.calibrate_device); the shard then carries
        float64 calibrated probabilities and the sink must not calibrate again.  `poisson=None` follows the reference's rule
        (run_predict.py:224: `poisson_calib or model_type == 'indel'`): on for indel models, off for snv.  `reuse`: let dense blocks of sites take the
        cross-position reuse kernels (same probabilities within rounding, tests/test_gpu_reuse.py).  `genome_from`: another forward
        (or a FastaGenomes) whose resident chromosome this one computes on instead of packing and uploading its own; `fasta_path`
        may then be None.  With fasta_path=None and no genome_from the forward is a member for a ModelSetForward, which binds it."""
        if poisson is None:
            poisson = model_type == "indel"
        self.calibration = dict(dirichlet_weights=dirichlet_weights, poisson=poisson, scale_factor=scale_factor)
        self.calibrated = dirichlet_weights is not None or bool(poisson) or bool(scale_factor)
        self.model = model.to(device).eval()
        self.local_radius, self.local_order, self.distal_radius = local_radius, local_order, distal_radius
        self.batch_sites, self.model_type, self.reuse = batch_sites, model_type, bool(reuse) and model_type == "snv"
        self._init_genomes(fasta_path, device, genome_from)
        self.reuse_sites = 0           # sites that went through the reuse kernels (diagnostics / tests)

    # -- compute ----------------------------------------------------------------------------------------------------------
    def _to_device(self, a, dtype):
        if isinstance(a, torch.Tensor):
            return a.to(self.device, dtype)
        return torch.from_numpy(np.ascontiguousarray(a)).to(self.device, dtype)

    @torch.no_grad()
    def __call__(self, chrom, pos, strand):
        """(rows, n_class + 1) for this rank's block of the chromosome's sites (numpy arrays or tensors, any device)."""
        g = self.genome(chrom)
        pos, strand = self._to_device(pos, torch.int64), self._to_device(strand, torch.uint8)
        n = pos.shape[0]
        k = self.model.n_class
        out = torch.empty((n, k + 1), dtype=torch.float64 if self.calibrated else torch.float32, device=self.device)
        with torch.cuda.device(self.device):
            if self.model_type == "snv" and self.reuse and n > 0:
                logp, used = self.model.forward_packed_reuse(g, pos, strand, local_radius=self.local_radius, local_order=self.local_order,
                                                             min_density=self.REUSE_MIN_DENSITY, batch_sites=self.batch_sites,
                                                             return_reuse_count=True)
                self.reuse_sites += used
                self._finish(out, 0, logp, g, pos, strand)
                return out
            for r0 in range(0, n, self.batch_sites):
                p, st = pos[r0:r0 + self.batch_sites], strand[r0:r0 + self.batch_sites]
                if self.model_type == "snv":
                    logp = self.model.forward_packed(g, p, st, local_radius=self.local_radius, local_order=self.local_order)
                else:
                    logp = self.model.forward_packed(g, p, st, self.distal_radius)
                self._finish(out, r0, logp, g, p, st)
        return out

    def _finish(self, out, r0, logp, g, p, st):
        m = logp.shape[0]
        if self.model_type == "snv":
            out[r0:r0 + m, -1] = g.encode_kmer(p, st, 1, 1)[:, 1].to(out.dtype)     # complemented focal base 0..4
        else:
            out[r0:r0 + m, -1] = 0.0
        if self.calibrated:
            from .calibration import calibrate_device
            out[r0:r0 + m, :-1] = calibrate_device(logp, **self.calibration)
        else:
            out[r0:r0 + m, :-1] = torch.softmax(logp, dim=1)


class ModelSetForward(FastaGenomes):
    """One forward for the rows of several site classes, each class served by its own model: the compute of a regions run over a
    union of classes (predict_regions_sharded, focal "SET").  `members`: {class: HipShardForward} with keys from 'A' (A/T sites),
    'nonCpG', 'CpG' and 'C' (= nonCpG and CpG through one model; not together with either).  Radii, weights, calibrators,
    scale_factor and reuse are each member's own; device, model_type 'snv', n_class and "calibrated or not" (the rows' dtype) must
    agree.

    The set alone packs and uploads a chromosome (FastaGenomes, `fasta_path`: by default the first member's); every member is bound
    to it and computes on that resident copy -- build the members with fasta_path=None and they never read the file.  A call
    classifies its rows on the device (PackedGenome.classify_sites), partitions them stably by member (data.genome.split_rows),
    gives every member its rows in ascending order and scatters the members' outputs into one (rows, n_class + 1) tensor
    (data.genome.scatter_rows).  The class counts are the one host read-back per call: they size the members' outputs."""

    KEYS = ("A", "C", "nonCpG", "CpG")

    def __init__(self, members, fasta_path=None):
        from .data.genome import ROW_CLASSES, SITE_CLASSES
        members = dict(members)
        unknown = [k for k in members if k not in self.KEYS]
        if unknown:
            raise ValueError(f"ModelSetForward: unknown site class {unknown[0]!r} (the keys are 'A', 'C', 'nonCpG', 'CpG')")
        if not members:
            raise ValueError("ModelSetForward: no member (at least one of 'A', 'C', 'nonCpG', 'CpG')")
        if "C" in members and ("CpG" in members or "nonCpG" in members):
            raise ValueError("ModelSetForward: 'C' serves the CpG and the nonCpG sites: it does not go with a 'CpG' or 'nonCpG' member")
        self.names = [k for k in self.KEYS if k in members]                    # member order: the order of `perm`'s blocks
        self.members = [members[k] for k in self.names]
        for k, m in zip(self.names, self.members):
            if not isinstance(m, HipShardForward):
                raise ValueError(f"ModelSetForward: member {k!r} is no HipShardForward")
        first = self.members[0]
        for k, m in zip(self.names[1:], self.members[1:]):
            for what, a, b in (("device", first.device, m.device), ("n_class", first.model.n_class, m.model.n_class),
                               ("calibrated", first.calibrated, m.calibrated)):
                if a != b:
                    raise ValueError(f"ModelSetForward: members {self.names[0]!r} and {k!r} differ in {what}: {a} and {b} "
                                     + ("(every member calibrated behind its head, or none)" if what == "calibrated" else ""))
        for k, m in zip(self.names, self.members):
            if m.model_type != "snv":
                raise ValueError(f"ModelSetForward: member {k!r} has model_type {m.model_type!r}: the site classes are the SNV models'")
        if fasta_path is None:
            fasta_path = next((m.fasta_path for m in self.members if m.fasta_path is not None), None)
        if fasta_path is None:
            raise ValueError("ModelSetForward: no FASTA file (fasta_path=, or a member built with one)")
        self.classes = 0
        slot = np.full(256, 255, np.uint8)                                     # row class -> member number
        for j, k in enumerate(self.names):
            self.classes |= SITE_CLASSES[k]
            for c, name in enumerate(ROW_CLASSES):
                if SITE_CLASSES[name] & SITE_CLASSES[k]:
                    slot[c] = j
        self.model, self.calibrated, self.model_type = first.model, first.calibrated, "snv"
        self._init_genomes(fasta_path, first.device)
        self._slot = torch.from_numpy(slot).to(self.device)
        for m in self.members:
            m.genome_from = self

    @property
    def reuse_sites(self):
        return sum(m.reuse_sites for m in self.members)

    @torch.no_grad()
    def __call__(self, chrom, pos, strand):
        """(rows, n_class + 1) for sites of `chrom`, every row by the member of its class.  A row that belongs to no member (an N, a
        position outside the record, the wrong strand, a class the set lacks) raises ValueError."""
        from .data.genome import scatter_rows, split_rows
        g = self.genome(chrom)
        pos, strand = g._prep(pos, strand)
        n, k = pos.shape[0], self.model.n_class
        out = torch.empty((n, k + 1), dtype=torch.float64 if self.calibrated else torch.float32, device=self.device)
        if n == 0:
            return out
        with torch.cuda.device(self.device):
            slot = self._slot[g.classify_sites(pos, strand).long()]
            perm, counts = split_rows(slot, len(self.members))
            counts = counts.tolist()                                           # the one read-back: the members' outputs must be sized
            if counts[-1]:
                i = int(torch.nonzero(slot == 255)[0])
                raise ValueError(f"ModelSetForward: {chrom}:{int(pos[i])} on strand '{'+-'[int(strand[i]) & 1]}' is a site of no member "
                                 f"({', '.join(self.names)}): an N or ambiguous base, a position outside the record, the other strand's "
                                 f"base or a class the set has no model for ({counts[-1]} such rows)")
            a = 0
            for m, rows in zip(self.members, counts):
                if rows:
                    idx = perm[a:a + rows]
                    scatter_rows(m(chrom, pos[idx], strand[idx]), idx, out)
                a += rows
        return out


# ------------------------------------------------------------------------------------------------------------------
# the prediction table
# ------------------------------------------------------------------------------------------------------------------
_NAME_STRIDE = 256


def _name_table(names):
    buf = C.create_string_buffer(max(len(names), 1) * _NAME_STRIDE)
    for i, nm in enumerate(names):
        raw = str(nm).encode()
        if len(raw) >= _NAME_STRIDE:
            raise ValueError(f"chromosome name longer than {_NAME_STRIDE - 1} bytes: {nm!r}")
        buf[i * _NAME_STRIDE:i * _NAME_STRIDE + len(raw)] = raw
    return buf


def _tsv_struct(names_buf, n_names, chrom_id, start, end, strand, label, prob, prob_f64, n_class, prob_stride, perm, n):
    t = _lib.MuralTsvRows()
    t.chrom_names, t.n_chroms, t.name_stride = C.cast(names_buf, C.c_char_p), max(n_names, 1), _NAME_STRIDE
    t.chrom_id, t.start, t.end, t.strand, t.label, t.prob, t.perm = chrom_id, start, end, strand, label, prob, perm
    t.prob_f64, t.n_class, t.prob_stride, t.n = int(prob_f64), int(n_class), int(prob_stride), int(n)
    return t


def format_rows_host(names, chrom_id, start, end, strand, label, prob, perm=None, threads=0):
    """Text of the prediction-table rows (no header) for host arrays, formatted by the C++ row formatter (csrc/tsv.hip): bytes.
    `names`: list of chromosome names, `chrom_id` indexes it (None = every row is names[0]); `strand` uint8 (1 = '-');
    `perm`: output row i = input row perm[i] (len(perm) rows are written: a sub-range of the sorted rows in the part-file mode)."""
    n = len(start)
    prob = np.asarray(prob)
    if prob.dtype not in (np.float32, np.float64):
        prob = prob.astype(np.float64)
    if prob.ndim != 2:
        prob = prob.reshape(n, -1)
    prob = np.ascontiguousarray(prob)
    cols = dict(start=np.ascontiguousarray(start, np.int64), end=np.ascontiguousarray(end, np.int64),
                strand=np.ascontiguousarray(strand, np.uint8), label=np.ascontiguousarray(label, np.float32))
    cid = None if chrom_id is None else np.ascontiguousarray(chrom_id, np.int32)
    pm = None if perm is None else np.ascontiguousarray(perm, np.int64)
    names_buf = _name_table(names)
    ptr = lambda a: None if a is None else a.ctypes.data     # noqa: E731
    t = _tsv_struct(names_buf, len(names), ptr(cid), ptr(cols["start"]), ptr(cols["end"]), ptr(cols["strand"]), ptr(cols["label"]),
                    ptr(prob) if prob.size else None, prob.dtype == np.float64, prob.shape[1], prob.shape[1], ptr(pm),
                    n if pm is None else len(pm))
    lib = _lib.lib()
    bound = int(lib.mural_tsv_row_bound(C.byref(t)))
    if bound < 0:
        _lib.check(_lib.MURAL_E_INVALID)
    out = np.empty(max(int(t.n) * bound, 1), np.uint8)
    nbytes = C.c_int64(0)
    _lib.check(lib.mural_tsv_format_host(C.byref(t), out.ctypes.data, out.size, C.byref(nbytes), int(threads)))
    return out[:nbytes.value].tobytes()


def _header(n_class):
    return ("\t".join(["chrom", "start", "end", "strand", "mut_type"] + ["prob%d" % i for i in range(n_class)]) + "\n").encode()


_PINNED_FREE = []      # pinned staging buffers of finished writers (pinning 100 MB costs ~20 ms: a process that writes many tables pays once)


def _pinned_staging(cap):
    for i, t in enumerate(_PINNED_FREE):
        if t.numel() >= cap:
            return _PINNED_FREE.pop(i)
    return torch.empty(cap, dtype=torch.uint8).pin_memory()


class _TextWriter(threading.Thread):
    """Writer thread of the device path: waits for a piece's format kernels, copies its text to pinned host memory on its own
    stream and write()s it; returns the device buffer to the pool.  One thread, pieces in order."""

    def __init__(self, fh, device, n_buffers, cap):
        super().__init__(daemon=True)
        self.fh, self.device = fh, device
        self.jobs, self.free = queue.Queue(), queue.Queue()
        self.text = [torch.empty(cap, dtype=torch.uint8, device=device) for _ in range(n_buffers)]
        self.count = [torch.zeros(1, dtype=torch.int64, device=device) for _ in range(n_buffers)]
        for i in range(n_buffers):
            self.free.put(i)
        self.host = _pinned_staging(cap)
        self.host_count = torch.zeros(1, dtype=torch.int64).pin_memory()
        self.error = None
        self.seconds = {"wait_device": 0.0, "copy": 0.0, "write": 0.0}
        self.bytes = 0
        self.shard_bytes = {}          # shard number -> bytes written for it (the part-file mode's index)

    def run(self):
        stream = torch.cuda.Stream(self.device)
        while True:
            job = self.jobs.get()
            if job is None:
                return
            idx, event, shard_no = job
            try:
                if self.error is None:
                    t0 = time.perf_counter()
                    event.synchronize()
                    t1 = time.perf_counter()
                    with torch.cuda.stream(stream):
                        self.host_count.copy_(self.count[idx], non_blocking=True)
                        stream.synchronize()
                        nb = int(self.host_count[0])
                        self.host[:nb].copy_(self.text[idx][:nb], non_blocking=True)
                        stream.synchronize()
                    t2 = time.perf_counter()
                    self.fh.write(memoryview(self.host.numpy())[:nb])
                    t3 = time.perf_counter()
                    self.seconds["wait_device"] += t1 - t0
                    self.seconds["copy"] += t2 - t1
                    self.seconds["write"] += t3 - t2
                    self.bytes += nb
                    self.shard_bytes[shard_no] = self.shard_bytes.get(shard_no, 0) + nb
            except Exception as e:      # noqa: BLE001  (surfaced by the sink)
                self.error = e
            finally:
                self.free.put(idx)


class TsvSink:
    """Rank-0 consumer of gathered shards: the prediction table of run_predict.py:217-239 (optional Dirichlet / Poisson
    calibration, columns chrom start end strand mut_type prob0.., rows sorted by (chrom, start), '%.4g'), byte-identical to the
    reference's pandas writer.

    A shard is a dict with the rows of ONE chromosome: ``chrom`` (name, or an array whose first entry is the name), ``start``,
    ``end``, ``strand`` (uint8 1 = '-', or '+' / '-' strings), ``label``, ``prob`` (n, k) -- numpy arrays, or torch tensors on a
    HIP device (then the stable sort by start, the calibration, the formatting and the copy-out all run on that device and a
    writer thread does the file I/O).  Shards whose chromosomes arrive in ascending name order -- what predict_bed_sharded
    produces -- are streamed out at once; any other arrival order is handled by spooling the raw rows and merging at close().
    Nothing is ever parsed back as numbers: chromosome names like '01' or '10' stay strings.

    ``parts=True`` under torch.distributed with more than one rank: EVERY rank is a consumer.  Each rank sorts the gathered shard (the
    all-gather of the probabilities stays the one collective of the path) and formats only ITS contiguous slice of the sorted rows --
    on its own GPU, through its own writer thread, into its own part file ``<path>.part<rank>`` -- so sort, format, copy-out and
    write() scale with the ranks instead of funnelling ~60 bytes of text per row through rank 0.  close() exchanges the per-shard byte
    counts and rank 0 strings the slices together in (shard, rank) order with in-kernel file copies (os.sendfile); the table is
    byte-identical to the single-writer one."""

    PIECE_ROWS = 1 << 20

    takes_aligned_blocks = True      # a shard marked "aligned" holds this rank's own rows in the table's order (no sort, no slicing)

    def __init__(self, path, poisson=False, dirichlet_weights=None, host_threads=0, parts=False, group=None):
        self.path, self.poisson, self.dirichlet_weights = str(path), poisson, dirichlet_weights
        self.host_threads = host_threads
        self.group = group
        self._emulated = isinstance(parts, tuple)      # (rank, world) without a process group: this rank's part file only -- the
        if self._emulated:                              # measurement of one rank's share of an N-rank run (bench.py: sink_only)
            self.rank, self.world = int(parts[0]), int(parts[1])
        else:
            self.rank = dist.get_rank(group) if (parts and dist.is_initialized()) else 0
            self.world = dist.get_world_size(group) if (parts and dist.is_initialized()) else 1
        self.parts = self.world > 1
        self._shard_no = -1
        self._shard_bytes = {}         # host path of the part mode: shard number -> bytes
        self._n_class = None
        self._out_path = self.path + (".part%04d" % self.rank if self.parts else "")
        self._fh = open(self._out_path, "wb")
        self._wrote_header = False
        self._last = None              # name of the last streamed chromosome
        self._spool = []               # out-of-order shards as host arrays
        self._writer = None
        self._ws = None
        self.rows = 0
        self.seconds = {"sort_format_enqueue": 0.0, "wait_buffer": 0.0, "host_format": 0.0, "host_write": 0.0}
        self._writer_totals = {"wait_device": 0.0, "copy": 0.0, "write": 0.0, "bytes": 0}
        self._writer_shard_bytes = {}  # device path of the part mode: shard number -> bytes, over every writer thread this sink had

    # -- helpers ----------------------------------------------------------------------------------------------------------
    @staticmethod
    def _name(shard):
        c = shard["chrom"]
        if isinstance(c, str):
            return c
        return str(c[0]) if len(c) else None

    @staticmethod
    def _strand_u8(s):
        if isinstance(s, torch.Tensor):
            return s
        s = np.asarray(s)
        return s if s.dtype == np.uint8 else (s == "-").astype(np.uint8)

    def _ensure_header(self, n_class):
        self._n_class = n_class
        if self.parts:                 # part files carry rows only; rank 0 writes the header when it strings them together
            return
        if not self._wrote_header:
            self._flush_writer()
            self._fh.write(_header(n_class))
            self._wrote_header = True

    def _flush_writer(self):
        """Wait until the writer thread has written everything handed to it (the file position is then ours)."""
        w = self._writer
        if w is not None:
            held = [w.free.get() for _ in range(len(w.text))]
            for i in held:
                w.free.put(i)
            if w.error is not None:
                raise w.error

    def _host_prob(self, prob):
        prob = np.asarray(prob)
        if self.dirichlet_weights is not None:
            from .calibration import dirichlet_calibrate
            prob = dirichlet_calibrate(prob, self.dirichlet_weights)
        if self.poisson:
            from .data.ingest import poisson_calibrate
            prob = poisson_calibrate(prob)
        return prob

    # -- streaming --------------------------------------------------------------------------------------------------------
    def _stream_host(self, name, shard):
        t0 = time.perf_counter()
        prob = self._host_prob(shard["prob"])
        start = np.asarray(shard["start"])
        if shard.get("aligned"):       # this rank's own rows, already in the table's order (predict_bed_sharded: _ShardTail.aligned)
            perm = np.arange(len(start), dtype=np.int64)
        else:
            perm = np.argsort(start, kind="stable")
            if self.parts:
                s0, s1 = shard_bounds(len(perm), self.rank, self.world)
                perm = perm[s0:s1]
        text = format_rows_host([name], None, start, shard["end"], self._strand_u8(shard["strand"]), shard["label"], prob, perm,
                                self.host_threads) if len(perm) else b""
        t1 = time.perf_counter()
        self._ensure_header(prob.shape[1] if prob.ndim == 2 else 0)
        self._flush_writer()
        self._fh.write(text)
        self._shard_bytes[self._shard_no] = self._shard_bytes.get(self._shard_no, 0) + len(text)
        self.seconds["host_format"] += t1 - t0
        self.seconds["host_write"] += time.perf_counter() - t1

    def _stream_device(self, name, shard):
        t0 = time.perf_counter()
        prob = shard["prob"]
        dev = prob.device
        n, k = prob.shape[0], int(shard.get("n_class", prob.shape[1]))
        lib = _lib.lib()
        with torch.cuda.device(dev):
            if self.dirichlet_weights is not None or self.poisson:
                from .calibration import calibrate_device
                prob = calibrate_device(prob[:, :k].contiguous() if prob.stride(0) != k else prob, dirichlet_weights=self.dirichlet_weights,
                                        poisson=self.poisson, input_is_prob=True)
            if prob.dtype not in (torch.float32, torch.float64):
                prob = prob.to(torch.float32)
            if prob.stride(1) != 1:
                prob = prob.contiguous()
            to = lambda a, dt: (a if isinstance(a, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(a))).to(dev, dt).contiguous()   # noqa: E731
            start, end = to(shard["start"], torch.int64), to(shard["end"], torch.int64)
            strand, label = to(self._strand_u8(shard["strand"]), torch.uint8), to(shard["label"], torch.float32)
            if shard.get("aligned"):   # this rank's own rows, already in the table's order (predict_bed_sharded: _ShardTail.aligned)
                perm = torch.arange(n, dtype=torch.int64, device=dev)
            else:
                perm = torch.sort(start, stable=True).indices
                if self.parts:             # this rank's slice of the sorted rows
                    s0, s1 = shard_bounds(n, self.rank, self.world)
                    perm = perm[s0:s1].contiguous()
                    n = s1 - s0
            names_buf = _name_table([name])
            t = _tsv_struct(names_buf, 1, None, start.data_ptr(), end.data_ptr(), strand.data_ptr(), label.data_ptr(), prob.data_ptr(),
                            prob.dtype == torch.float64, k, prob.stride(0), None, 0)
            bound = int(lib.mural_tsv_row_bound(C.byref(t)))
            piece = self.PIECE_ROWS
            self._ensure_header(k)
            if self._writer is None or self._writer.device != dev or self._writer.text[0].numel() < piece * bound:
                self._close_writer()
                self._writer = _TextWriter(self._fh, dev, 3, piece * (bound + 24))     # slack: a longer chromosome name reuses it
                self._writer.start()
                self._ws = torch.empty(int(lib.mural_tsv_format_workspace_bytes(piece)) + _NAME_STRIDE, dtype=torch.uint8, device=dev)
            w = self._writer
            stream = _lib.current_stream_ptr(dev)
            for r0 in range(0, n, piece):
                m = min(piece, n - r0)
                tw = time.perf_counter()
                idx = w.free.get()                         # back-pressure: all text buffers are with the writer
                self.seconds["wait_buffer"] += time.perf_counter() - tw
                if w.error is not None:
                    w.free.put(idx)
                    raise w.error
                t.perm, t.n = perm[r0:r0 + m].data_ptr(), m
                _lib.check(lib.mural_tsv_format_device(C.byref(t), w.text[idx].data_ptr(), w.text[idx].numel(), w.count[idx].data_ptr(),
                                                      self._ws.data_ptr(), self._ws.numel(), stream))
                ev = torch.cuda.Event()
                ev.record()
                w.jobs.put((idx, ev, self._shard_no))
            # the tensors of this shard must outlive the kernels just enqueued: the caching allocator keeps their memory on this
            # stream, so later allocations of the same stream cannot overwrite them before the kernels ran
        self.seconds["sort_format_enqueue"] += time.perf_counter() - t0

    def __call__(self, shard):
        name = self._name(shard)
        n = len(shard["start"])
        # an aligned shard hands every rank ITS rows of a chromosome, in the table's order and possibly in several parts: the parts after
        # the first continue the shard (same name), and a rank without rows still counts the shard (the part files are strung together by
        # shard number)
        more = bool(shard.get("aligned")) and name is not None and name == self._last and not self._spool
        if name is not None and n == 0 and shard.get("aligned") and self.parts:
            if more:
                return
            if not (self._last is None or name > self._last):
                raise ValueError("TsvSink(parts=True) takes the shards in ascending chromosome order (predict_bed_sharded's order)")
            self._last = name
            self._shard_no += 1
            return
        if name is None or n == 0:
            return
        _refuse_second_calibration(shard, self.poisson, self.dirichlet_weights)
        self.rows += n
        on_device = isinstance(shard["prob"], torch.Tensor) and shard["prob"].is_cuda
        if self.parts and not more and not (self._last is None or name > self._last):
            raise ValueError("TsvSink(parts=True) takes the shards in ascending chromosome order (predict_bed_sharded's order)")
        if more or (not self._spool and (self._last is None or name > self._last)):
            if not more:
                self._last = name
                self._shard_no += 1
            if on_device:
                self._stream_device(name, shard)
            else:
                if isinstance(shard["prob"], torch.Tensor):
                    shard = dict(shard, prob=shard["prob"].numpy())
                self._stream_host(name, shard)
            return
        cpu = lambda a: a.detach().cpu().numpy() if isinstance(a, torch.Tensor) else np.asarray(a)     # noqa: E731
        k = int(shard.get("n_class", shard["prob"].shape[1]))
        self._spool.append({"name": name, "start": cpu(shard["start"]), "end": cpu(shard["end"]),
                            "strand": cpu(self._strand_u8(shard["strand"])), "label": cpu(shard["label"]),
                            "prob": self._host_prob(cpu(shard["prob"])[:, :k])})

    # -- close ------------------------------------------------------------------------------------------------------------
    def _close_writer(self):
        if self._writer is not None:
            self._writer.jobs.put(None)
            self._writer.join()
            if len(_PINNED_FREE) < 2:
                _PINNED_FREE.append(self._writer.host)
            err = self._writer.error
            for key, v in dict(self._writer.seconds, bytes=self._writer.bytes).items():
                self._writer_totals[key] += v
            # per-shard byte counts of EVERY writer this sink has had (a later chromosome name longer than the writer's staging or
            # a device change replaces the writer mid-run): the part-file assembly's index
            for k, v in self._writer.shard_bytes.items():
                self._writer_shard_bytes[k] = self._writer_shard_bytes.get(k, 0) + v
            self._writer = None
            if err is not None:
                raise err

    def writer_seconds(self):
        """Busy seconds of the writer thread(s) by phase and the bytes they wrote (complete after close())."""
        out = dict(self._writer_totals)
        if self._writer is not None:
            for key, v in dict(self._writer.seconds, bytes=self._writer.bytes).items():
                out[key] += v
        return out

    @staticmethod
    def _copy_slices(dst_path, part_path, pieces):
        """Copy [(source offset, destination offset, bytes)] from this rank's part file into the table through a shared mapping: page
        faults of different ranks proceed side by side, where write()s to ONE file are serialised by its inode lock (the copy of a
        7 GB table by rank 0 alone took as long as the prediction)."""
        import mmap
        total = sum(n for _, _, n in pieces)
        if total == 0:
            return
        with open(dst_path, "r+b") as dst, open(part_path, "rb") as src:
            dm = mmap.mmap(dst.fileno(), 0)
            sm = mmap.mmap(src.fileno(), 0, access=mmap.ACCESS_READ)
            try:
                for so, do, n in pieces:
                    step = 64 << 20
                    for o in range(0, n, step):
                        m = min(step, n - o)
                        dm[do + o:do + o + m] = sm[so + o:so + o + m]
                dm.flush()
            finally:
                sm.close()
                dm.close()

    def _close_parts(self):
        """Part mode: exchange the per-shard byte counts; rank 0 creates the table at its final size (header + every slice), then EVERY
        rank copies its own slices to their places in (shard, rank) order -- in parallel -- and the part files go."""
        w_bytes = dict(self._shard_bytes)
        for k, v in self._writer_shard_bytes.items():
            w_bytes[k] = w_bytes.get(k, 0) + v
        mine = [int(w_bytes.get(i, 0)) for i in range(self._shard_no + 1)]
        self._fh.flush()
        self._fh.close()
        size = os.path.getsize(self._out_path)
        if sum(mine) != size:      # an index that does not add up to the part file would mis-order or truncate the table silently
            raise IOError("part file %s holds %d bytes, its per-shard index adds up to %d" % (self._out_path, size, sum(mine)))
        if self._emulated:
            return
        everyone = [None] * self.world
        dist.all_gather_object(everyone, (mine, self._n_class), group=self.group)     # (every rank closed its part before this returns)
        n_shards = max(len(c) for c, _ in everyone)
        k = next((nc for _, nc in everyone if nc is not None), 0)
        head = _header(k)
        count = lambda r, i: everyone[r][0][i] if i < len(everyone[r][0]) else 0      # noqa: E731
        t0 = time.perf_counter()
        pieces, dst_off, src_off = [], len(head), 0
        for i in range(n_shards):
            for r in range(self.world):
                n = count(r, i)
                if r == self.rank and n:
                    pieces.append((src_off, dst_off, n))
                    src_off += n
                dst_off += n
        ok = True
        if self.rank == 0:
            try:
                with open(self.path, "wb") as out:
                    out.write(head)
                    out.truncate(dst_off)
            except OSError:
                ok = False
        dist.barrier(group=self.group)      # the table file exists at its final size
        err = None
        try:
            if not ok:
                raise IOError("cannot create %s" % self.path)
            if src_off != size:
                raise IOError("part file %s: %d of %d bytes have a place in the table" % (self._out_path, src_off, size))
            self._copy_slices(self.path, self._out_path, pieces)
        except Exception as e:      # noqa: BLE001  (every rank reaches the barrier below; the parts stay for inspection)
            err = e
        flags = [None] * self.world
        dist.all_gather_object(flags, err is None, group=self.group)      # (also the barrier: every slice is in place)
        if all(flags):
            os.unlink(self._out_path)
        self.seconds["assemble_parts"] = time.perf_counter() - t0
        if err is not None:
            raise err
        if not all(flags):
            raise IOError("another rank could not copy its slices into %s; the part files stay" % self.path)

    def abort(self):
        """Stop the writer and remove what was written: the caller's run failed (e.g. the focal-base check of a later shard) and,
        like the reference, leaves no table behind."""
        try:
            self._close_writer()
        except Exception:      # noqa: BLE001  (the run is failing already)
            pass
        try:
            self._fh.close()
        finally:
            if os.path.exists(self._out_path):
                os.unlink(self._out_path)
        self._spool = []

    def close(self):
        self._close_writer()
        if self.parts:
            self._close_parts()
            return
        if not self._spool:
            if not self._wrote_header:
                self._fh.write(_header(0))
            self._fh.close()
            return
        # Out-of-order arrival: merge the spooled rows with what was already streamed.  Streamed rows are text already; per
        # chromosome they are merged line-wise by their start field (they arrived first, so they win ties), never re-parsed as
        # numbers.
        self._fh.flush()
        self._fh.close()
        with open(self.path, "rb") as fh:
            blob = fh.read()
        head_len = blob.index(b"\n") + 1 if self._wrote_header else 0
        k = self._spool[0]["prob"].shape[1]
        body = blob[head_len:]
        lines_by_chrom = {}
        if body:
            for line in body.split(b"\n")[:-1]:
                lines_by_chrom.setdefault(line.split(b"\t", 1)[0].decode(), []).append(line)
        spooled = {}
        for sh in self._spool:
            spooled.setdefault(sh["name"], []).append(sh)
        with open(self.path, "wb") as out:
            out.write(_header(k))
            for name in sorted(set(lines_by_chrom) | set(spooled)):
                old = lines_by_chrom.get(name, [])
                new_lines = []
                if name in spooled:
                    parts = spooled[name]
                    cat = lambda key: np.concatenate([p[key] for p in parts])     # noqa: E731
                    text = format_rows_host([name], None, cat("start"), cat("end"), cat("strand"), cat("label"), cat("prob"), None,
                                            self.host_threads)
                    new_lines = text.split(b"\n")[:-1]
                lines = old + new_lines
                starts = np.array([int(ln.split(b"\t", 2)[1]) for ln in lines], np.int64)
                for i in np.argsort(starts, kind="stable"):
                    out.write(lines[i] + b"\n")
        self._spool = []


def _refuse_second_calibration(rows, poisson, dirichlet_weights):
    """`rows` (a shard or a collected result) says whether its probabilities went through the calibration chain on the device
    already (HipShardForward(dirichlet_weights= / poisson= / scale_factor=); `poisson` defaults to ON there for indel models,
    run_predict.py:224).  Calibrating such rows again would be silent and wrong."""
    if rows is not None and rows.get("calibrated") and (poisson or dirichlet_weights is not None):
        raise ValueError("these probabilities are calibrated already (HipShardForward applied its dirichlet_weights / poisson / "
                         "scale_factor chain on the device; poisson defaults to on for model_type='indel'): drop poisson= / "
                         "dirichlet_weights= here, or build the forward with poisson=False")


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
    strand = np.zeros(len(start), np.uint8) if strand is None else TsvSink._strand_u8(strand)
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
    from .tables import kmer_name
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
    from .tables import check_motif_length
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
    from .tables import kmer_name
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
    s.label, s.label_kind = label.data_ptr(), {torch.float32: 0, torch.int32: 1, torch.int64: 2}[label.dtype]
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
    device kernel that keeps host shards on the host (tests without a device)."""

    takes_aligned_blocks = True

    def __init__(self, out_prefix=None, windows=(), benchmark_regions=None, ratio_cutoff=0.2, poisson=False, dirichlet_weights=None,
                 group=None, parts=False, kmers=(), genome=None, kmer_strand=None, motifs=(), motif_indel=False, calibration=False,
                 calibration_bins=50, fit_calibrator=None, fit_rows_max=1 << 27, fit_row_terms=None):
        self.out_prefix = None if out_prefix is None else os.fspath(out_prefix)
        self.windows = tuple(int(w) for w in windows)
        if any(w <= 0 for w in self.windows) or len(set(self.windows)) != len(self.windows):
            raise ValueError(f"window sizes must be positive and distinct (got {self.windows})")
        if isinstance(benchmark_regions, (str, os.PathLike)):
            from .tables import read_regions
            benchmark_regions = read_regions(benchmark_regions)
        self._regions = None if benchmark_regions is None else {
            c: (np.sort(np.asarray(a, np.int64)), np.sort(np.asarray(b, np.int64))) for c, (a, b) in benchmark_regions.items()}
        self.ratio_cutoff, self.poisson, self.dirichlet_weights, self.group = ratio_cutoff, poisson, dirichlet_weights, group
        self.rank = dist.get_rank(group) if (parts and dist.is_initialized()) else 0
        self.world = dist.get_world_size(group) if (parts and dist.is_initialized()) else 1
        self.parts = self.world > 1
        self.rows = 0
        self._n_class = None
        self._tables = {}              # chromosome -> {W: (bin0, table)}
        self._prob_sum, self._n_sites, self._status = 0.0, 0, 0
        self._pending = None           # a staged device part: reduced when the next one arrives (or at close)
        self._inflight = []            # [(event, pinned result, chromosome, [(W, bin0, bins)])] of launched parts
        self._dev_regions = {}
        self._written = []
        self._result = None
        from .tables import check_kmer_length, strand_mode
        self.kmers = tuple(check_kmer_length(k) for k in kmers)
        if len(set(self.kmers)) != len(self.kmers):
            raise ValueError(f"k-mer lengths must be distinct (got {self.kmers})")
        if self.kmers and genome is None:
            raise ValueError("SummarySink(kmers=...) needs genome=: a callable chromosome name -> packed genome")
        self._genome = genome
        self._kmer_indel = kmer_strand is not None
        self._kmer_mode = strand_mode("indel", kmer_strand) if self._kmer_indel else 0
        # accumulators, read back once at close(): the tables per k, the first-appearance words per chromosome and k (two chromosomes
        # share k-mers, and the order between chromosomes -- by name, as in the written table -- is only known when all have arrived)
        self._kmer_host = ({}, {})     # ({k: table}, {chromosome: {k: first}}) of the host shards
        self._kmer_dev = {}            # device -> ({k: table}, {chromosome: {k: first}}, status)
        from .tables import check_motif_length
        self.motifs = tuple(check_motif_length(m) for m in motifs)
        if len(set(self.motifs)) != len(self.motifs):
            raise ValueError(f"motif lengths must be distinct (got {self.motifs})")
        if self.motifs and genome is None:
            raise ValueError("SummarySink(motifs=...) needs genome=: a callable chromosome name -> packed genome")
        self._motif_indel = bool(motif_indel)
        self._motif_host, self._motif_dev = ({}, {}), {}      # as the k-mer accumulators
        self.fit_calibrator, self.fit_rows_max, self._fit_row_terms = fit_calibrator, int(fit_rows_max), fit_row_terms
        if fit_calibrator is not None:
            from .evaluation import CALIBRATORS
            if fit_calibrator not in CALIBRATORS:
                raise ValueError(f"unknown calibrator {fit_calibrator!r} (one of {sorted(CALIBRATORS)})")
            _refuse_fit_on_calibrated(poisson or dirichlet_weights is not None)
        self.calibration = bool(calibration) or fit_calibrator is not None
        self.calibration_bins = int(calibration_bins)
        if self.calibration and self.calibration_bins < 1:
            raise ValueError(f"calibration_bins must be positive (got {calibration_bins})")
        self._calib_bounds = calib_bounds(self.calibration_bins) if self.calibration else None
        self._calib_host = {}          # chromosome -> table uint64 [cells] of the host shards
        self._calib_dev = {}           # device -> ({chromosome: table}, status, bounds): read back once, at close()
        self._fit_blocks, self._fit_rows = [], 0      # [(prob float32 [n][n_class], label uint8 [n])], on a device or on the host

    # -- one part ---------------------------------------------------------------------------------------------------------
    def _take(self, name, tables, total, n_sites, status):
        mine = self._tables.setdefault(name, {})
        for W, (bin0, t) in tables.items():
            mine[W] = _merge_window_table(mine.get(W), bin0, t)
        self._prob_sum += total
        self._n_sites += n_sites
        self._status |= status

    def _host_part(self, name, shard, k):
        prob = TsvSink._host_prob(self, np.asarray(shard["prob"])[:, :k])
        start = np.asarray(shard["start"])
        cols = [start, np.asarray(shard["end"]), np.asarray(shard["label"]), prob]
        if not shard.get("aligned"):
            perm = np.argsort(start, kind="stable")
            if self.parts:
                perm = perm[slice(*shard_bounds(len(perm), self.rank, self.world))]
            cols = [c[perm] for c in cols]
        regs = None if self._regions is None else self._regions.get(name, (np.zeros(0, np.int64),) * 2)
        self._take(name, *summary_rows_host(cols[3], cols[0], cols[1], cols[2], k, self.windows, regs))
        if self.kmers:
            strand = TsvSink._strand_u8(shard["strand"])
            strand = strand if shard.get("aligned") else strand[perm]
            tabs, firsts = self._kmer_host
            for kk in self.kmers:
                tabs.setdefault(kk, np.zeros((4 ** kk, 3, k), np.uint64))
            mine = firsts.setdefault(name, {kk: np.full(4 ** kk, _KMER_NEVER, np.uint64) for kk in self.kmers})
            _, status = summary_kmer_host(self._genome(name), cols[3], cols[0], cols[1], strand, cols[2], k, self.kmers, self._kmer_indel,
                                          self._kmer_mode, into={kk: (tabs[kk], mine[kk]) for kk in self.kmers})
            self._status |= status
        if self.motifs:
            tabs, firsts = self._motif_host
            for m in self.motifs:
                tabs.setdefault(m, np.zeros((4 ** m, 3, k), np.uint64))
            mine = firsts.setdefault(name, {m: np.full(4 ** m, _KMER_NEVER, np.uint64) for m in self.motifs})
            _, status = summary_motif_host(self._genome(name), cols[3], cols[0], cols[1], cols[2], k, self.motifs, self._motif_indel,
                                           into={m: (tabs[m], mine[m]) for m in self.motifs})
            self._status |= status
        if self.calibration:
            _, status = summary_calib_host(cols[3], cols[2], k, self.calibration_bins, self._calib_bounds,
                                           into=self._calib_table(self._calib_host, name, k))
            self._status |= status
        if self.fit_calibrator is not None:
            lab = np.asarray(cols[2])
            good = np.isfinite(lab.astype(np.float64)) & (lab >= 0) & (lab < k) & (lab == np.floor(lab.astype(np.float64)))
            self._retain(np.ascontiguousarray(cols[3], np.float32), np.where(good, lab, 255).astype(np.uint8))

    def _calib_table(self, tables, name, k):
        cells = calib_cells(k, self.calibration_bins)
        if cells > _CALIB_MAX_CELLS:
            raise ValueError(f"calibration_bins * (n_class + 1) = {self.calibration_bins * (k + 1)} is too large: the table of {cells} "
                             f"cells does not fit the {_CALIB_MAX_CELLS} a workgroup holds")
        if name not in tables:
            tables[name] = np.zeros(cells, np.uint64)
        return tables[name]

    def _retain(self, prob, label):
        """Keep a part's (float32 probabilities, uint8 labels -- 255 where the label is none) for the fit at close().  Every row of the
        part counts against `fit_rows_max`: an invalid row makes close() raise before anything is fitted."""
        if self._fit_rows + len(label) > self.fit_rows_max:
            raise ValueError(f"fit_calibrator={self.fit_calibrator!r}: this shard takes the rows retained on this rank from {self._fit_rows} to "
                             f"{self._fit_rows + len(label)}, beyond fit_rows_max={self.fit_rows_max}; raise the budget or fit on fewer rows "
                             "(nothing is subsampled silently)")
        self._fit_rows += len(label)
        self._fit_blocks.append((prob, label))

    def _calib_device(self, name, dev, prob, label, k):
        """Enqueue the metrics reduction of a part behind its forward: one launch (and the fold of the carries) into the chromosome's
        accumulator on that device."""
        acc = self._calib_dev.get(dev)
        if acc is None:
            acc = self._calib_dev[dev] = ({}, torch.zeros(1, dtype=torch.int32, device=dev), torch.from_numpy(self._calib_bounds).to(dev))
        table = acc[0].get(name)
        if table is None:
            cells = len(self._calib_table({}, name, k))
            table = acc[0][name] = torch.zeros(cells, dtype=torch.int64, device=dev)
        calib_rows_device(prob, label, k, self.calibration_bins, acc[2], table, acc[1])

    def _kmer_device(self, name, dev, prob, start, end, strand, label, k):
        """Enqueue the k-mer reduction of a part behind its forward: the part's chromosome is the resident one now."""
        lib = _lib.lib()
        genome = self._genome(name)
        if genome.length >= 1 << (_KMER_ORD_SHIFT - 1):
            raise ValueError(f"k-mer summary: chromosome {name} has 2^39 bases or more")
        acc = self._kmer_dev.get(dev)
        if acc is None:
            acc = self._kmer_dev[dev] = ({kk: torch.zeros(4 ** kk * 3 * k, dtype=torch.int64, device=dev) for kk in self.kmers}, {},
                                         torch.zeros(1, dtype=torch.int32, device=dev))
        first = acc[1].get(name)
        if first is None:              # (all ones: the largest unsigned value)
            first = acc[1][name] = {kk: torch.full((4 ** kk,), -1, dtype=torch.int64, device=dev) for kk in self.kmers}
        g = genome.as_struct(dev)
        stream = _lib.current_stream_ptr(dev)
        for at in range(0, len(self.kmers), 4):          # MURAL_SUMMARY_MAX_KMERS lengths per call
            group = self.kmers[at:at + 4]
            s = _lib.MuralSummaryKmerRows()
            s.genome = C.pointer(g)
            s.prob, s.prob_f64, s.prob_stride = prob.data_ptr(), int(prob.dtype == torch.float64), prob.stride(0)
            s.start, s.end, s.strand, s.label = start.data_ptr(), end.data_ptr(), strand.data_ptr(), label.data_ptr()
            s.label_kind = {torch.float32: 0, torch.int32: 1, torch.int64: 2}[label.dtype]
            s.n, s.n_class, s.n_k, s.indel, s.mode = start.shape[0], k, len(group), int(self._kmer_indel), self._kmer_mode
            for j, kk in enumerate(group):
                s.k[j], s.table[j], s.first[j] = kk, acc[0][kk].data_ptr(), first[kk].data_ptr()
            s.order_base, s.status = 0, acc[2].data_ptr()
            _lib.check(lib.mural_summary_kmer_rows(C.byref(s), stream))
        return genome

    def _motif_device(self, name, dev, prob, start, end, label, k):
        """Enqueue the motif reduction of a part behind its forward, as ``_kmer_device``."""
        lib = _lib.lib()
        genome = self._genome(name)
        if genome.length >= 1 << (_KMER_ORD_SHIFT - 1):
            raise ValueError(f"motif summary: chromosome {name} has 2^39 bases or more")
        acc = self._motif_dev.get(dev)
        if acc is None:
            acc = self._motif_dev[dev] = ({m: torch.zeros(4 ** m * 3 * k, dtype=torch.int64, device=dev) for m in self.motifs}, {},
                                          torch.zeros(1, dtype=torch.int32, device=dev))
        first = acc[1].get(name)
        if first is None:
            first = acc[1][name] = {m: torch.full((4 ** m,), -1, dtype=torch.int64, device=dev) for m in self.motifs}
        g = genome.as_struct(dev)
        stream = _lib.current_stream_ptr(dev)
        for at in range(0, len(self.motifs), 4):         # MURAL_SUMMARY_MAX_KMERS lengths per call
            group = self.motifs[at:at + 4]
            s = _lib.MuralSummaryMotifRows()
            s.genome = C.pointer(g)
            s.prob, s.prob_f64, s.prob_stride = prob.data_ptr(), int(prob.dtype == torch.float64), prob.stride(0)
            s.start, s.end, s.label = start.data_ptr(), end.data_ptr(), label.data_ptr()
            s.label_kind = {torch.float32: 0, torch.int32: 1, torch.int64: 2}[label.dtype]
            s.n, s.n_class, s.n_m, s.indel, s.order_by_row = start.shape[0], k, len(group), int(self._motif_indel), 0
            for j, m in enumerate(group):
                s.m[j], s.table[j], s.first[j] = m, acc[0][m].data_ptr(), first[m].data_ptr()
            s.order_base, s.status = 0, acc[2].data_ptr()
            _lib.check(lib.mural_summary_motif_rows(C.byref(s), stream))
        return genome

    def _stage_device(self, name, shard, k):
        """Calibrate and order the part on its device, start the read-back of its first and last start."""
        prob = shard["prob"]
        dev = prob.device
        with torch.cuda.device(dev):
            if self.dirichlet_weights is not None or self.poisson:
                from .calibration import calibrate_device
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
            strand = to(TsvSink._strand_u8(shard["strand"]), torch.uint8) if self.kmers else None
            if not shard.get("aligned"):
                perm = torch.sort(start, stable=True).indices
                if self.parts:
                    perm = perm[slice(*shard_bounds(perm.shape[0], self.rank, self.world))]
                prob, start, end, label = prob[perm], start[perm], end[perm], label[perm]
                strand = strand[perm] if self.kmers else None
            if start.shape[0] == 0:
                return None
            # the k-mer tables have a fixed size: reduced now, while this part's chromosome is the resident one; the staged part keeps
            # the packed genome (and the columns) alive all the same -- the window tables are reduced one part late
            genome = self._kmer_device(name, dev, prob, start, end, strand, label, k) if self.kmers else None
            if self.motifs:
                genome = self._motif_device(name, dev, prob, start, end, label, k)
            if self.calibration:
                self._calib_device(name, dev, prob, label, k)
            if self.fit_calibrator is not None:
                good = (label >= 0) & (label < k) & (label == label.to(torch.int64))
                self._retain(prob[:, :k].to(torch.float32, copy=True).contiguous(), torch.where(good, label, 255).to(torch.uint8))
            ends = torch.empty(2, dtype=torch.int64).pin_memory()
            ends.copy_(torch.stack([start[0], start[-1]]), non_blocking=True)
            ev = torch.cuda.Event()
            ev.record()
        return dict(name=name, prob=prob, start=start, end=end, label=label, k=k, ends=ends, event=ev, dev=dev, strand=strand,
                    genome=genome)

    def _launch_pending(self):
        """Reduce the staged part: its first and last start (read back by now) size the part's window tables."""
        p, self._pending = self._pending, None
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
        for W in self.windows:
            bin0, bins = lo // W, hi // W - lo // W + 1
            if bins * stride >= 2 ** 31:
                raise ValueError(f"the rows of one part span {bins} windows of {W} bp: too many for one table")
            layout.append((W, bin0, bins, off))
            off += bins * stride
        with torch.cuda.device(dev):
            out = torch.zeros(off, dtype=torch.float64, device=dev)      # total | n_sites (int64) | status (int32) | the tables
            regs = None
            if self._regions is not None:
                regs = self._dev_regions.get((p["name"], dev))
                if regs is None:
                    b0, b1 = self._regions.get(p["name"], (np.zeros(0, np.int64),) * 2)
                    regs = (torch.from_numpy(np.r_[b0, 0]).to(dev), torch.from_numpy(np.r_[b1, 0]).to(dev), len(b0))
                    self._dev_regions = {(p["name"], dev): regs}
            stream = _lib.current_stream_ptr(dev)
            for g in range(0, max(len(layout), 1), 4):      # MURAL_SUMMARY_MAX_WINDOWS window sizes per call; the totals with the first
                group = layout[g:g + 4]
                s = _lib.MuralSummaryRows()
                s.prob, s.prob_f64, s.prob_stride = p["prob"].data_ptr(), int(p["prob"].dtype == torch.float64), p["prob"].stride(0)
                s.start, s.end, s.label, s.n, s.n_class = p["start"].data_ptr(), p["end"].data_ptr(), p["label"].data_ptr(), n, k
                s.label_kind = {torch.float32: 0, torch.int32: 1, torch.int64: 2}[p["label"].dtype]
                s.n_windows = len(group)
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
        self._inflight.append((ev, host, p["name"], k, layout))

    def _harvest(self, done_only=False):
        keep = []
        for item in self._inflight:
            ev, host, name, k, layout = item
            if done_only and (keep or not ev.query()):      # (in arrival order: nothing overtakes an unfinished part)
                keep.append(item)
                continue
            ev.synchronize()
            a = host.numpy()
            stride = 1 + 2 * k
            tables = {W: (bin0, a[o:o + bins * stride].reshape(bins, stride)) for W, bin0, bins, o in layout}
            self._take(name, tables, float(a[0]), int(a[1:2].view(np.int64)[0]), int(a[2:3].view(np.int32)[0]))
        self._inflight = keep

    def __call__(self, shard):
        name = TsvSink._name(shard)
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
            staged = self._stage_device(name, shard, k)      # enqueued behind this part's forward ...
            self._launch_pending()                           # ... while the part before it, complete by now, is reduced
            self._pending = staged
        else:
            if isinstance(shard["prob"], torch.Tensor):
                shard = dict(shard, prob=shard["prob"].numpy())
            self._host_part(name, {key: (_np(v) if isinstance(v, torch.Tensor) else v) for key, v in shard.items()}, k)

    # -- close ------------------------------------------------------------------------------------------------------------
    def _merged(self, states):
        """[(tables, prob_sum, n_sites, status, n_class, k-mer state)] of the ranks, added in rank order."""
        tables, prob_sum, n_sites, status, k = {}, 0.0, 0, 0, None
        for t, s, c, st, kk, *_ in states:
            for name, per_w in t.items():
                mine = tables.setdefault(name, {})
                for W, (bin0, tab) in per_w.items():
                    mine[W] = _merge_window_table(mine.get(W), bin0, tab)
            prob_sum, n_sites, status = prob_sum + s, n_sites + c, status | st
            k = kk if k is None else k
        return (tables, prob_sum, n_sites, status, k, _kmer_merge([st[5] for st in states]) if self.kmers else None,
                _kmer_merge([st[6] for st in states], _MOTIF_ORD_SHIFT) if self.motifs else None,
                self._calib_merged([st[7] for st in states if st[7]], k) if self.calibration else None)

    def _calib_merged(self, per_rank, k):
        """[{chromosome: table}] of the ranks (or of a rank's devices and its host rows) -> one such dict: integer tables added, carries
        folded."""
        out = {}
        for tables in per_rank:
            for name, t in tables.items():
                if name in out:
                    _calib_fold(np.add(out[name], t, out=out[name]), k, self.calibration_bins)
                else:
                    out[name] = t.copy()
        return out

    def _calib_read_back(self):
        mine = [self._calib_host]
        for tables, dev_status, _ in self._calib_dev.values():
            self._status |= int(dev_status.item())
            mine.append({name: t.cpu().numpy().view(np.uint64) for name, t in tables.items()})
        return self._calib_merged([m for m in mine if m], self._n_class)

    def _read_back(self, host, devices, shift):
        """The one read-back of the device accumulators of the k-mer (or motif) tables, merged with the host rows'."""
        mine = [host]
        for tabs, firsts, dev_status in devices.values():
            self._status |= int(dev_status.item())
            mine.append(({kk: t.cpu().numpy().view(np.uint64).reshape(4 ** kk, 3, -1) for kk, t in tabs.items()},
                         {nm: {kk: f.cpu().numpy().view(np.uint64) for kk, f in per_k.items()} for nm, per_k in firsts.items()}))
        return _kmer_merge([_kmer_collapse(tabs, firsts, shift) for tabs, firsts in mine if tabs], shift)

    def close(self):
        self._launch_pending()
        self._harvest()
        kmer_state = self._read_back(self._kmer_host, self._kmer_dev, _KMER_ORD_SHIFT) if self.kmers else None
        motif_state = self._read_back(self._motif_host, self._motif_dev, _MOTIF_ORD_SHIFT) if self.motifs else None
        calib_state = self._calib_read_back() if self.calibration else None
        state = (self._tables, self._prob_sum, self._n_sites, self._status, self._n_class, kmer_state, motif_state, calib_state)
        if self.world > 1:
            every = [None] * self.world
            dist.all_gather_object(every, state, group=self.group)      # the one collective: tables, not rows
            state = self._merged(every)
        tables, prob_sum, n_sites, status, k, kmer_state, motif_state, calib_state = state
        for bit, what in _SUMMARY_STATUS:
            if status & bit:
                raise ValueError(f"summary: {what}")
        windows = {}
        for W in self.windows:
            keys, rows = [], []
            for name in sorted(tables):
                bin0, t = tables[name].get(W, (0, np.zeros((0, 1))))
                live = np.nonzero(t[:, 0] > 0)[0]
                keys += [(name, int((bin0 + g) * W + W)) for g in live]
                rows.append(t[live])
            windows[W] = (keys, np.concatenate(rows) if rows else np.zeros((0, 1 + 2 * (k or 0))))
        self._result = {"prob_sum": prob_sum, "n_sites": n_sites, "windows": windows}
        if self.kmers:
            ktables = kmer_state[1]
            self._kmer_sums = ktables
            self._result["kmers"] = {kk: (kmer_table_from_sums(*ktables[kk], kk, k) if kk in ktables else ([], np.zeros((0, 1 + 2 * (k or 0)))))
                                     for kk in self.kmers}
        if self.motifs:
            mtables = motif_state[1]
            self._motif_sums = mtables
            self._result["motifs"] = {m: (motif_table_from_sums(*mtables[m], m, k) if m in mtables else ([], np.zeros((0, 1 + 2 * (k or 0)))))
                                      for m in self.motifs}
        if self.calibration:
            self._close_calibration(calib_state or {}, k)
        if self.out_prefix is not None and self.rank == 0 and k is not None:
            from .tables import regional_output_names, write_regional_outputs
            for W in self.windows:
                self._written += list(regional_output_names(self.out_prefix, W)[:2])
                write_regional_outputs(*windows[W], k, W, self.out_prefix, self.ratio_cutoff)
            from .tables import kmer_output_names, write_kmer_outputs
            for kk in self.kmers:
                self._written += list(kmer_output_names(self.out_prefix, kk))
                write_kmer_outputs(*self._result["kmers"][kk], k, kk, self.out_prefix)
            from .tables import motif_output_names, write_motif_outputs
            for m in self.motifs:
                self._written += list(motif_output_names(self.out_prefix, m))
                write_motif_outputs(*self._result["motifs"][m], k, m, self.out_prefix)
            if self.calibration:
                self._write_calibration()

    # -- calibration metrics and the calibrator fit ---------------------------------------------------------------------------
    def _calib_total(self, per_chrom, k):
        total = np.zeros(calib_cells(k or 1, self.calibration_bins), np.uint64)
        for t in per_chrom.values():
            _calib_fold(np.add(total, t, out=total), k or 1, self.calibration_bins)
        return total

    def _close_calibration(self, per_chrom, k):
        nb = self.calibration_bins
        total = self._calib_total(per_chrom, k)
        self._calib_sums = {"all": total, "per_chromosome": per_chrom}
        res = calib_metrics_from_sums(total, nb, k or 1)
        res["per_chromosome"] = {name: calib_metrics_from_sums(per_chrom[name], nb, k) for name in sorted(per_chrom)}
        self._result["calibration"] = res
        if self.fit_calibrator is not None:
            self._fit(res, k)

    def _block_terms(self, prob, label, w, need_hessian):
        """(loss sum, gradient sum, Hessian sum) of one retained block: the device kernel, or the stand-in given as `fit_row_terms`."""
        k = prob.shape[1]
        km = k * (k + 1)
        if self._fit_row_terms is not None:
            loss, g, h = self._fit_row_terms(_np(prob), _np(label), w, need_hessian)
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
        """Fit the named calibrator on the retained raw-softmax rows (training.py:478), save it, and reduce the metrics of the calibrated
        rows through the same entry.  The data terms are the float64 atomic sums of ``mural_eval_dirichlet_fit_terms`` per block, added
        over blocks and -- one small all_reduce per evaluation -- over ranks: the weights are reproducible to rounding, not bit for bit.
        Only the metrics carry the bit-exact promise."""
        from .calibration import calibrate_device, dirichlet_calibrate, save_dirichlet_calibrator
        from .evaluation import _FIT_MAX_CLASSES, CALIBRATORS, newton_calibrator
        name = self.fit_calibrator
        method, ref_row, reg_lambda, reg_mu, reg_norm = CALIBRATORS[name]
        if k is None or k < 2 or k > _FIT_MAX_CLASSES:
            raise ValueError(f"fit_calibrator supports 2..{_FIT_MAX_CLASSES} classes, got {k}")
        if any(c == 0 for c in res["label_counts"]):
            raise ValueError("every class 0..n_class-1 must occur in the labels (the reference sizes the map by unique(y))")
        if reg_norm:                                              # multinomial.py:81-86
            if reg_mu is None:
                reg_lambda = reg_lambda / (k * (k + 1))
            else:
                reg_lambda, reg_mu = reg_lambda / (k * (k - 1)), reg_mu / k
        if self._fit_row_terms is None:                           # host shards are uploaded now, beside the device blocks
            dev = next((p.device for p, _ in self._fit_blocks if isinstance(p, torch.Tensor)), None)
            dev = torch.device("cuda", torch.cuda.current_device()) if dev is None else dev
            self._fit_blocks = [(p, y) if isinstance(p, torch.Tensor) else (torch.from_numpy(p).to(dev), torch.from_numpy(y).to(dev))
                                for p, y in self._fit_blocks]
        km = k * (k + 1)
        n = res["rows"]

        def row_terms(w, need_hessian):
            sums = np.zeros(1 + km + km * km)
            for p, y in self._fit_blocks:
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
        for p, y in self._fit_blocks:
            if isinstance(p, torch.Tensor):
                dev = p.device
                if dev not in after:
                    after[dev] = (torch.zeros(calib_cells(k, self.calibration_bins), dtype=torch.int64, device=dev),
                                  torch.zeros(1, dtype=torch.int32, device=dev))
                    bounds[dev] = torch.from_numpy(self._calib_bounds).to(dev)
                with torch.cuda.device(dev):
                    cal = calibrate_device(p, dirichlet_weights=weights, input_is_prob=True)
                    calib_rows_device(cal, y.to(torch.int32), k, self.calibration_bins, bounds[dev], *after[dev])
            else:
                summary_calib_host(dirichlet_calibrate(p, weights), y, k, self.calibration_bins, self._calib_bounds,
                                   into=self._calib_table(after, "host", k))
        tables = {key: (v if isinstance(v, np.ndarray) else v[0].cpu().numpy().view(np.uint64)) for key, v in after.items()}
        if self.world > 1:
            every = [None] * self.world
            dist.all_gather_object(every, tables, group=self.group)
            tables = {(r, key): t for r, ts in enumerate(every) for key, t in ts.items()}
        total = self._calib_total(tables, k)
        self._calib_sums["after"] = total
        res["after"] = calib_metrics_from_sums(total, self.calibration_bins, k)
        res["weights"], res["fit_loss"] = weights, float(loss)
        if self.out_prefix is not None and self.rank == 0:
            path = self.out_prefix + ".fdiri_cal.pkl"
            self._written.append(path)
            save_dirichlet_calibrator(weights, path)

    def _write_calibration(self):
        res = self._result["calibration"]
        path = self.out_prefix + ".calibration.txt"
        self._written.append(path)
        line = lambda tag, m: "%s\t%d\t%.8f\t%.8f\t%.8f\t%.8f\n" % (tag, m["rows"], m["nll"], m["ece"], m["c_ece"], m["brier"])      # noqa: E731
        with open(path, "w") as fh:
            fh.write("chrom\trows\tnll\tece\tc_ece\tbrier\n" + line("all", res))
            if "after" in res:
                fh.write(line(f"all (after {self.fit_calibrator})", res["after"]))
            for name, m in res["per_chromosome"].items():
                fh.write(line(name, m))

    def calibration_sums(self):
        """{"all": table, "per_chromosome": {name: table}[, "after": table]} after close(): the integer tables behind
        result()["calibration"] (``summary_calib_host``'s layout)."""
        self.result()
        return self._calib_sums

    def abort(self):
        """Drop what was reduced and remove any file close() began: the caller's run failed."""
        self._pending, self._inflight, self._tables, self._result = None, [], {}, None
        self._kmer_host, self._kmer_dev = ({}, {}), {}
        self._motif_host, self._motif_dev = ({}, {}), {}
        self._calib_host, self._calib_dev, self._fit_blocks, self._fit_rows = {}, {}, [], 0
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
        return self._kmer_sums

    def motif_sums(self):
        """{m: (table uint64 [4^m][3][n_class], first uint64 [4^m])} after close(): the exact sums behind result()["motifs"]
        (``summary_motif_host``'s layout, the chromosome's ordinal by name above each first-appearance word)."""
        self.result()
        return self._motif_sums

    def scaling_factor(self, genomewide_mu, m_proportion, g_proportion=1.0):
        """``tables.calc_mu_scaling_factor``'s factor for the summarised rows, with the lines it prints."""
        from .tables import mu_scaling_factor, print_scaling_factor
        res = self.result()
        factor = mu_scaling_factor(genomewide_mu, res["n_sites"], m_proportion, g_proportion, res["prob_sum"])
        print_scaling_factor(genomewide_mu, res["n_sites"], g_proportion, m_proportion, res["prob_sum"], factor)
        return factor


class TeeSink:
    """One shard loop, several consumers: every shard, close() and abort() go to each of `sinks` in turn.  The tee takes aligned blocks,
    and is a part-file sink, only if all of them do / are; when one of them raises, the others are aborted before the error goes on."""

    def __init__(self, *sinks):
        if not sinks:
            raise ValueError("TeeSink needs a sink")
        self.sinks = sinks
        self.takes_aligned_blocks = all(getattr(s, "takes_aligned_blocks", False) for s in sinks)
        self.parts = all(getattr(s, "parts", False) for s in sinks)

    def _each(self, call):
        for i, s in enumerate(self.sinks):
            try:
                call(s)
            except BaseException:
                for other in self.sinks[:i] + self.sinks[i + 1:]:
                    if hasattr(other, "abort"):
                        other.abort()
                raise

    def __call__(self, shard):
        self._each(lambda s: s(shard))

    def close(self):
        self._each(lambda s: s.close() if hasattr(s, "close") else None)

    def abort(self):
        for s in self.sinks:
            if hasattr(s, "abort"):
                s.abort()


def write_predictions(res, path, poisson=False, dirichlet_weights=None):
    """The prediction table of run_predict.py:217-239 from the dict returned by ``predict_bed`` / ``predict_bed_sharded``: optional
    Dirichlet calibration (``calibration.load_dirichlet_weights`` of the model's ``model.fdiri_cal.pkl``), optional Poisson
    calibration, then columns chrom, start, end, strand, mut_type, prob0.., rows sorted by (chrom, start) like pandas'
    sort_values (stable), tab-separated, floats as '%.4g' -- byte-identical to the reference's pandas writer, formatted by the
    C++ row formatter.  Returns the number of rows."""
    prob = np.asarray(res["prob"])
    _refuse_second_calibration(res, poisson, dirichlet_weights)
    if dirichlet_weights is not None:
        from .calibration import dirichlet_calibrate
        prob = dirichlet_calibrate(prob, dirichlet_weights)
    if poisson:
        from .data.ingest import poisson_calibrate
        prob = poisson_calibrate(prob)
    chrom = np.asarray(res["chrom"], dtype=object)
    n = len(chrom)
    names = sorted(set(chrom.tolist()))
    rank = {nm: i for i, nm in enumerate(names)}
    cid = np.fromiter((rank[c] for c in chrom), np.int32, n)
    start = np.asarray(res["start"], np.int64)
    perm = np.lexsort((start, cid))                     # stable, like pandas' multi-column sort_values
    strand = np.asarray(res["strand"])
    strand = strand if strand.dtype == np.uint8 else (strand == "-").astype(np.uint8)
    k = prob.shape[1] if prob.ndim == 2 else 0
    with open(path, "wb") as fh:
        fh.write(_header(k))
        if n:
            fh.write(format_rows_host(names, cid, start, res["end"], strand, np.asarray(res["label"], np.float32), prob, perm))
    return n


def _device_of(forward):
    dev = getattr(forward, "device", None)
    if dev is not None and torch.device(dev).type == "cuda":
        return torch.device(dev)
    return None


def _rank_world(group, emulate):
    """(rank, world) of a file-level run: the process group's (0, 1 without one), or the pair `emulate` names."""
    if emulate is not None:
        return int(emulate[0]), int(emulate[1])
    if dist.is_initialized():
        return dist.get_rank(group), dist.get_world_size(group)
    return 0, 1


def _np(a):
    return a.detach().cpu().numpy() if isinstance(a, torch.Tensor) else np.asarray(a)


def _forward_rows(forward, chrom, pos, strand, rows, T, normalise=True):
    """This rank's forward call for `rows` sites of `chrom`: the (rows, n_class + 1) tensor, float32 / float64 with `normalise`."""
    t0 = time.perf_counter()
    local = forward(chrom, pos, strand)
    T["compute_enqueue"] += time.perf_counter() - t0
    if local.shape[0] != rows:
        raise RuntimeError("forward returned a wrong number of rows")
    if not isinstance(local, torch.Tensor):
        local = torch.from_numpy(np.ascontiguousarray(local))
    if normalise and local.dtype not in (torch.float32, torch.float64):
        local = local.to(torch.float32)
    return local


def _aligned_verdict(infos):
    """The focal-base check of an aligned shard from every rank's (rows, first segment, its '+' / '-' focal base, last segment, its
    '+' / '-' focal base, own verdict): a block's own groups were checked by its rank; a (segment, strand) group that runs over a block
    border -- or over several blocks, some of them without a row of that strand -- must carry one base.  Raises ValueError."""
    carry_seg, carry = None, [-1, -1]
    for m, seg_a, fa_p, fa_m, seg_b, fb_p, fb_m, bad in (tuple(int(v) for v in row) for row in infos):
        if bad:
            raise ValueError(_FOCAL_MSG)
        if m == 0:
            continue
        if carry_seg == seg_a:
            for have, mine in ((carry[0], fa_p), (carry[1], fa_m)):
                if have >= 0 and mine >= 0 and have != mine:
                    raise ValueError(_FOCAL_MSG)
        if seg_b != carry_seg:
            carry_seg, carry = seg_b, [-1, -1]
        # (seg_a == seg_b: the two triples describe the same groups)
        carry = [fb_p if fb_p >= 0 else carry[0], fb_m if fb_m >= 0 else carry[1]]


class _ShardTail:
    """What happens to a gathered shard (rows of one chromosome in bed_reader order): the per-(segment, strand) focal-base check --
    its verdict is read one shard late, so no rank waits for work just enqueued --, the sink, the collection for the caller."""

    def __init__(self, forward, check, sink, collect, T, dev, rank):
        self.check, self.sink, self.collect, self.T, self.dev = check, sink, collect, T, dev      # check: the focal-base rule applies
        self.feeds_sink = sink is not None and (rank == 0 or getattr(sink, "parts", False))
        self.need_meta = collect or self.feeds_sink
        # HipShardForward with a calibration chain hands over calibrated probabilities: the flag travels with every shard (and the
        # collected result) so that a sink / write_predictions asked to calibrate as well refuses instead of calibrating twice
        self.calibrated = bool(getattr(forward, "calibrated", False))
        self.kept, self.pending = [], None
        T.update({"compute_enqueue": 0.0, "gather": 0.0, "sink": 0.0, "focal_wait": 0.0})

    def _finish_check(self):
        pc, self.pending = self.pending, None
        if pc is None:
            return
        t = time.perf_counter()
        ev, host = pc
        ev.synchronize()
        self.T["focal_wait"] += time.perf_counter() - t
        if host.dim() == 2:                 # an aligned shard: the ranks' border groups (see aligned_part)
            _aligned_verdict(host.numpy())
        elif int(host[0]) != 0:
            raise ValueError(_FOCAL_MSG)

    def _defer(self, verdict):
        """`verdict` (a device tensor: a status word, or an aligned shard's border records) is read one shard late, the PREVIOUS one now."""
        with torch.cuda.device(self.dev):
            host = torch.zeros(verdict.shape, dtype=verdict.dtype).pin_memory()
            host.copy_(verdict, non_blocking=True)
            ev = torch.cuda.Event()
            ev.record()
        self._finish_check()
        self.pending = (ev, host)

    def _hand_over(self, chrom, rows, start, end, strand, label, aligned=False):
        """The shard dict of `rows` ((n, k + 1): probabilities + focal base) and its site columns -> the sink.  Device tensors stay what
        they are (`prob` keeps the focal column, `n_class` says where it ends); rows of a host forward become numpy arrays."""
        if not self.need_meta:
            return None
        k = rows.shape[1] - 1
        if self.dev is None:
            rows, start, end, strand, label = _np(rows)[:, :k], _np(start), _np(end), _np(strand), _np(label)
        shard = {"chrom": chrom, "start": start, "end": end, "strand": strand, "label": label, "prob": rows, "n_class": k,
                 "calibrated": self.calibrated}
        if aligned:
            shard["aligned"] = True
        if self.feeds_sink:
            t0 = time.perf_counter()
            self.sink(shard)
            self.T["sink"] += time.perf_counter() - t0
        return shard

    def __call__(self, chrom, runs, full, start, end, strand, label, grp, file_rows=None):
        """`full`: (n, k + 1) probabilities + focal base; `grp`: non-decreasing group ids; `runs`: [(lo, hi)] positions of the shard's
        rows in the whole input's bed_reader order; `file_rows`: file row index per row (rank-local ingest) or None."""
        n, k = full.shape[0], full.shape[1] - 1
        if self.check and self.dev is not None:
            status = torch.zeros(1, dtype=torch.int32, device=self.dev)
            with torch.cuda.device(self.dev):
                _lib.check(_lib.lib().mural_focal_group_check(full.data_ptr(), int(full.dtype == torch.float64), full.stride(0), k,
                                                             grp.contiguous().data_ptr(), n, status.data_ptr(),
                                                             _lib.current_stream_ptr(self.dev)))
            self._defer(status)
        elif self.check:
            check_focal_groups(_np(full)[:, -1].astype(np.int64), _np(grp))
        shard = self._hand_over(chrom, full, start, end, strand, label)
        if self.collect:
            self.kept.append((runs, {"start": _np(shard["start"]), "end": _np(shard["end"]), "strand": _np(shard["strand"]),
                                     "label": _np(shard["label"]), "prob": _np(shard["prob"])[:, :k], "chrom": chrom,
                                     "file_rows": None if file_rows is None else _np(file_rows)}))

    # -- a chromosome whose rows already are in the table's order (BedRun.in_order) -------------------------------------------------
    # The file order then IS the output order, this rank's block of the rows IS its slice of the table, and nothing but the focal-base
    # check looks across blocks: a (segment, strand) group that straddles a block border must agree on both sides.  Every rank checks its
    # own groups, the ranks exchange 7 numbers -- rows, first / last segment, focal base of the '+' and the '-' group of each (-1: none) --
    # and every rank walks the chain (verdict read one shard late, like the gathered shards').  No all-gather of rows, no sort of n rows.
    def aligned_part(self, chrom, local, start, end, strand, label, anchor, central_bp):
        """One PART of this rank's block of an aligned chromosome (the block goes through in parts of <= _ALIGNED_PART_ROWS rows, in file
        order: the table writer works on one part while the next is computed, and host / device memory is bounded by a part).  `local`:
        (m, k + 1) probabilities + focal base, start / strand / end / label: the part's site columns, tensors on one device (CPU tensors
        with a host forward).  Returns the part's border record for ``aligned_close`` (None without the focal-base check)."""
        m, k = local.shape[0], local.shape[1] - 1
        info = None
        if self.check:
            e0 = (anchor if anchor is not None else 1) + central_bp
            seg = torch.where(start > e0, (start - e0 + (central_bp - 1)) // central_bp, torch.zeros_like(start))
            key = (seg << 1) | strand.to(torch.int64)
            key_o, order = torch.sort(key, stable=True)
            focal_o = local[:, k][order].contiguous()
            status = torch.zeros(1, dtype=torch.int32, device=local.device)
            info = torch.full((8,), -1, dtype=torch.int64, device=local.device)
            info[0] = m
            if m:
                if self.dev is not None:
                    with torch.cuda.device(self.dev):
                        _lib.check(_lib.lib().mural_focal_group_check(focal_o.data_ptr(), int(focal_o.dtype == torch.float64), 1, 0, key_o.data_ptr(),
                                                                     m, status.data_ptr(), _lib.current_stream_ptr(self.dev)))
                else:
                    try:
                        check_focal_groups(focal_o.numpy().astype(np.int64), key_o.numpy())
                    except ValueError:
                        status[0] = 1
                want = torch.stack([key_o[0] & ~1, (key_o[0] & ~1) | 1, key_o[-1] & ~1, (key_o[-1] & ~1) | 1])
                at = torch.searchsorted(key_o, want).clamp(max=m - 1)
                have = key_o[at] == want
                foc = torch.where(have, focal_o[at].to(torch.int64), torch.full_like(at, -1))
                info[1], info[4] = key_o[0] >> 1, key_o[-1] >> 1
                info[2:4], info[5:7] = foc[0:2], foc[2:4]
            info[7] = status[0].to(torch.int64)
        self._hand_over(chrom, local, start, end, strand, label, aligned=True)
        return info

    def aligned_close(self, infos, group, world, emulated):
        """The border records of this rank's parts of one aligned chromosome -> ONE small all-gather (parts x 8 numbers per rank) -> the
        chain over (rank, part) in table order; the verdict is read one shard late (no rank waits for work just enqueued)."""
        if not self.check:
            return
        mine = torch.stack(infos)                                    # (parts, 8)
        if world > 1 and not emulated:
            every = [torch.empty_like(mine) for _ in range(world)]
            dist.all_gather(every, mine, group=group)
            every = torch.cat(every)                                 # rank-major = table order
        else:
            every = mine
        if self.dev is not None:
            self._defer(every)
        else:
            self._finish_check()
            _aligned_verdict(every.numpy())

    @contextlib.contextmanager
    def frame(self):
        """Around a driver's shard loop: the last verdict and the sink's close() behind it, the sink's abort() on ANY exception.  The
        verdict of a shard's focal-base check is read one shard late, i.e. after that shard's rows went to the sink: a failing run must
        not leave a partial table with a valid-looking header behind (the reference exits before writing anything)."""
        try:
            yield
            self._finish_check()
            if self.feeds_sink and hasattr(self.sink, "close"):
                t0 = time.perf_counter()
                self.sink.close()
                self.T["sink_close"] = time.perf_counter() - t0
        except BaseException:
            if self.feeds_sink and hasattr(self.sink, "abort"):
                self.sink.abort()
            raise

    def result(self, n_all, order):
        if not self.collect:
            return n_all
        if not self.kept:
            return {"chrom": np.zeros(0, object), "start": np.zeros(0, np.int64), "end": np.zeros(0, np.int64),
                    "strand": np.zeros(0, object), "label": np.zeros(0, np.float32), "prob": np.zeros((0, 0), np.float32),
                    "order": np.zeros(0, np.int64)}
        k = self.kept[0][1]["prob"].shape[1]
        if order is None:
            order = np.empty(n_all, np.int64)
        out = {"chrom": np.empty(n_all, object), "start": np.empty(n_all, np.int64), "end": np.empty(n_all, np.int64),
               "strand": np.empty(n_all, object), "label": np.empty(n_all, np.float32),
               "prob": np.empty((n_all, k), self.kept[0][1]["prob"].dtype), "order": order, "calibrated": self.calibrated}
        for runs, sh in self.kept:
            o = 0
            for lo, hi in runs:
                m = hi - lo
                out["chrom"][lo:hi] = sh["chrom"]
                out["start"][lo:hi], out["end"][lo:hi] = sh["start"][o:o + m], sh["end"][o:o + m]
                out["strand"][lo:hi] = np.where(sh["strand"][o:o + m] == 1, "-", "+")
                out["label"][lo:hi], out["prob"][lo:hi] = sh["label"][o:o + m], sh["prob"][o:o + m]
                if sh["file_rows"] is not None:
                    out["order"][lo:hi] = sh["file_rows"][o:o + m]
                o += m
        return out


def predict_bed_sharded(forward, bed_path, segment_center=300000, model_type="snv", group=None, sink=None, collect=True, timings=None,
                        ingest="ranked", emulate=None):
    """Sharded file-level prediction.  `forward(chrom_name, pos, strand) -> (rows, n_class + 1)` tensor (probabilities + focal
    base; see HipShardForward) is called once per shard (= chromosome, in ascending name order) with THIS rank's contiguous block
    of the shard's sites.  Every rank takes part in one all_gather per shard; `sink(shard_dict)` is called on rank 0 (every rank
    for a part-file sink) with the gathered shard in bed_reader order (keys chrom, start, end, strand, label, prob, n_class;
    device tensors when `forward` has a HIP ``device`` attribute, numpy arrays otherwise).  With `collect` the function also returns
    those arrays for ALL rows in bed_reader order on every rank -- leave it off for genome-scale inputs and let the sink stream
    them out.  Returns the dict (or the row count if not collecting).  `timings`: optional dict that receives the wall-clock split.

    `ingest="ranked"` (default): the BED file is indexed once -- every rank scans 1 / world of its bytes -- and a rank parses only
    its own block of every chromosome (``data.ingest.BedIndex``); the gathered row carries the site columns next to the
    probabilities, so host memory per rank is bounded by its share of one chromosome.  `ingest="whole"`: every rank parses the
    whole file (the reference's per-process BedTool, run_predict.py:107); the two produce identical results.
    `emulate=(rank, world)`: no process group -- run ONE rank's share of a `world`-rank run (its index scan, parse, compute,
    sort / format share with a part-file sink) and report the host seconds spent on standing in for the other ranks in
    timings['emulation'] (bench.py: config5_e2e.rank_share)."""
    if ingest == "whole":
        if emulate is not None:
            raise ValueError("emulate=(rank, world) needs ingest='ranked'")
        return _predict_bed_whole(forward, bed_path, segment_center, model_type, group, sink, collect, timings)
    if ingest != "ranked":
        raise ValueError(f"ingest must be 'ranked' or 'whole', got {ingest!r}")
    from .data import ingest as ing
    rank, world = _rank_world(group, emulate)
    T = {} if timings is None else timings
    T["emulation"] = 0.0
    t0 = time.perf_counter()
    index = ing.BedIndex.build(bed_path, rank, world, group, emulate=emulate is not None, seconds=T)
    T["bed_index"] = time.perf_counter() - t0
    if emulate is not None:
        T["emulation"] += T["bed_index"] - T["index_scan"]
    T.update({"bed_parse": 0.0, "pack_rows": 0.0, "reorder": 0.0})
    return _predict_shards(forward, _BedSites(index), int(segment_center), model_type, group, sink, collect, T, rank, world,
                           emulate is not None)


def _row_layout(k, f64):
    """Byte layout of a gathered row: start i64 | end i64 | prob k x (f64 | f32) | focal (same type) | label f32 | strand u8 | pad."""
    e = 8 if f64 else 4
    off_prob = 16
    off_label = off_prob + (k + 1) * e
    off_strand = off_label + 4
    width = (off_strand + 1 + 7) // 8 * 8
    return off_prob, off_label, off_strand, width


def _pack_rows(local, start, end, strand, label):
    """(m, W) uint8 rows of this rank's block: the forward's (m, k + 1) matrix with the site columns beside it."""
    m, k = local.shape[0], local.shape[1] - 1
    f64 = local.dtype == torch.float64
    off_prob, off_label, off_strand, W = _row_layout(k, f64)
    buf = torch.zeros((m, W), dtype=torch.uint8, device=local.device)
    se = buf[:, 0:16].view(torch.int64)
    se[:, 0], se[:, 1] = start, end
    buf[:, off_prob:off_label].view(local.dtype)[:] = local
    buf[:, off_label:off_label + 4].view(torch.float32)[:, 0] = label
    buf[:, off_strand] = strand
    return buf


def _unpack_rows(full, k, dtype):
    off_prob, off_label, off_strand, _ = _row_layout(k, dtype == torch.float64)
    se = full[:, 0:16].view(torch.int64)
    return (full[:, off_prob:off_label].view(dtype), se[:, 0], se[:, 1], full[:, off_strand],
            full[:, off_label:off_label + 4].view(torch.float32)[:, 0])


def _bed_reader_keys(start, strand, run_rows, first_run_anchor, central_bp):
    """Sort key of bed_reader's row order (preprocessing.py:39-106) for the rows of one chromosome in FILE order: the runs restart
    the segment grid (end0 = 1 + central_bp; the file's very first run: its first start + central_bp), a row's segment is the
    number of times `while start > end0: end0 += central_bp` has fired so far -- a function of the running maximum of start --,
    and a segment yields its '+' rows, then its '-' rows: key = ((run << 40 | segment) << 1) | strand, rows stably sorted by it."""
    keys, lo = [], 0
    for j, rows in enumerate(run_rows):
        s = start[lo:lo + rows]
        e0 = (first_run_anchor if (j == 0 and first_run_anchor is not None) else 1) + central_bp
        rm = torch.cummax(s, 0).values
        seg = torch.where(rm > e0, (rm - e0 + (central_bp - 1)) // central_bp, torch.zeros_like(rm))
        keys.append((((j << 40) + seg) << 1) | strand[lo:lo + rows].to(torch.int64))
        lo += rows
    return keys[0] if len(keys) == 1 else torch.cat(keys)


_ALIGNED_BLOCKS = True      # (tests switch it off to compare the two routes of the ranked ingest)
_ALIGNED_PART_ROWS = 1 << 22


def _takes_aligned_blocks(sink, collect, world):
    """Aligned blocks need a consumer that takes a rank's own rows as its slice of the table: every rank's part-file sink (or the one
    rank there is), and nobody who wants all rows back."""
    return (not collect and _ALIGNED_BLOCKS and (sink is None or getattr(sink, "takes_aligned_blocks", False))
            and (world == 1 or sink is None or getattr(sink, "parts", False)))


def _aligned_parts(n, world):
    """Parts of <= _ALIGNED_PART_ROWS rows that the longest block of `n` rows over `world` ranks goes through; every rank makes as many."""
    return max(1, -(-(-(-n // world)) // _ALIGNED_PART_ROWS))


def _gather_rows(local, cols, n, group, T, pack_key, stand_in=None):
    """This rank's (m, k + 1) rows and their site columns (start, end, strand, label) -> the chromosome's `n` rows of every rank, through
    ONE all_gather of packed rows (or `stand_in(packed)` for it): (rows, start, end, strand, label), views of the gathered buffer."""
    t0 = time.perf_counter()
    packed = _pack_rows(local, *cols)
    T[pack_key] += time.perf_counter() - t0
    t0 = time.perf_counter()
    full = all_gather_rows(packed, n, group) if stand_in is None else stand_in(packed)
    T["gather"] += time.perf_counter() - t0
    return _unpack_rows(full, local.shape[1] - 1, local.dtype)


class _BedSites:
    """Site source of the ranked BED ingest: a chromosome's rows in FILE order (its runs concatenated), of which a rank parses only the
    slices it is asked for (data.ingest.BedIndex)."""
    check_focal = True           # the reference's per-(segment, strand) focal-base check
    reorder = True               # gathered rows go from file order to bed_reader order
    read_key = "bed_parse"

    def __init__(self, index):
        self.index, self.names = index, sorted(index.chroms)

    def open(self, chrom, fetch_next):
        runs = [self.index.runs[i] for i in self.index.chroms[chrom]]
        return sum(r.rows for r in runs), len(runs) == 1 and runs[0].in_order

    def columns(self, chrom, lo, hi):
        start, end, label, strand = self.index.read_block(chrom, lo, hi)
        return start, end, strand, label

    def done(self, chrom):
        pass

    def layout(self, chrom, row0, n):
        ids = self.index.chroms[chrom]
        runs = [(self.index.runs[i].row0, self.index.runs[i].row0 + self.index.runs[i].rows) for i in ids]
        return runs, self.index.runs[0].first_start if ids[0] == 0 else None      # (the FILE's first run anchors its segment grid)


def _predict_shards(forward, src, central_bp, model_type, group, sink, collect, T, rank, world, emulated, finish=None):
    """The per-chromosome loop of the file-level drivers, over `src.names` in ascending order: the table's.  Per chromosome `src` answers
    open(chrom, fetch_next) -> (sites, "they are in the table's order") -- a source that counts on the device calls fetch_next() behind
    the work it enqueued --, columns(chrom, lo, hi) -> (start, end, strand, label) of sites [lo, hi), host arrays or device tensors,
    charged to T[src.read_key], and layout(chrom, row0, n) -> ([(lo, hi)] file rows of its runs, the first run's anchor), where `row0`
    rows precede the chromosome in this loop.  src.done(chrom) is called behind the chromosome's last part, `finish()` behind the last
    chromosome; what they raise aborts the sink.  src.check_focal / src.reorder: see _BedSites."""
    clock = time.perf_counter
    dev = _device_of(forward)
    tdev = dev if dev is not None else torch.device("cpu")
    tail = _ShardTail(forward, model_type == "snv" and src.check_focal, sink, collect, T, dev, rank)
    aligned_ok = _takes_aligned_blocks(sink, collect, world)
    up = lambda a: a if isinstance(a, torch.Tensor) else torch.from_numpy(a).to(tdev)     # noqa: E731
    rows_all = 0
    with tail.frame():
        for si, chrom in enumerate(src.names):
            todo = [src.names[si + 1]] if hasattr(forward, "prefetch") and si + 1 < len(src.names) else []
            fetch_next = lambda: todo and forward.prefetch(todo.pop())     # noqa: E731  (the next chromosome's pack is started once)
            n, in_order = src.open(chrom, fetch_next)
            if n == 0:                                     # (a BED file has no rows for such a chromosome either: it is no shard)
                continue
            runs, anchor = src.layout(chrom, rows_all, n)
            rows_all += n
            b0, b1 = shard_bounds(n, rank, world)
            # a chromosome whose rows already are in the table's order: this rank's block is its slice of the table (_ShardTail.aligned_part);
            # it goes through in parts (every rank the same number of them: the one collective of the shard carries a record per part)
            is_aligned = aligned_ok and in_order
            n_parts = _aligned_parts(n, world) if is_aligned else 1
            records = []
            for part in range(n_parts):
                p0, p1 = shard_bounds(b1 - b0, part, n_parts)
                t0 = clock()
                start_h, end_h, strand_h, label_h = src.columns(chrom, b0 + p0, b0 + p1)
                T[src.read_key] += clock() - t0
                fetch_next()                               # during the first part: the pack runs beside this chromosome's compute
                # every site column goes up BEFORE the forward is enqueued: a copy from pageable host memory waits for the stream's earlier
                # work, and behind the forward it would hold the host for the whole compute instead of letting it parse the next chromosome
                pos_b, strand_b, end_b, label_b = up(start_h), up(strand_h), up(end_h), up(label_h)
                local = _forward_rows(forward, chrom, start_h if dev is None else pos_b, strand_h if dev is None else strand_b, p1 - p0, T)
                if is_aligned:
                    records.append(tail.aligned_part(chrom, local, pos_b, end_b, strand_b, label_b, anchor, central_bp))
            src.done(chrom)
            if is_aligned:
                tail.aligned_close(records, group, world, emulated)
                T["aligned_shards"] = T.get("aligned_shards", 0) + 1
                continue

            def stand_in(packed):
                # emulate=(rank, world): the other ranks' blocks are their site columns (parsed here, outside the share) next to copies of
                # this rank's probability rows -- the gathered shard has the size, the sort keys and the text width of the real one
                if dev is not None:
                    torch.cuda.synchronize(dev)            # this rank's own work is charged to the share: the stand-in must not hide it
                te = clock()
                full = torch.empty((n, packed.shape[1]), dtype=torch.uint8, device=tdev)
                for r in range(world):
                    lo, hi = shard_bounds(n, r, world)
                    if r == rank or hi == lo:
                        continue
                    rows = local[torch.arange(hi - lo, device=tdev) % max(local.shape[0], 1)] if local.shape[0] else \
                        torch.zeros((hi - lo, local.shape[1]), dtype=local.dtype, device=tdev)
                    full[lo:hi] = _pack_rows(rows, *[up(c) for c in src.columns(chrom, lo, hi)])
                if dev is not None:
                    torch.cuda.synchronize(dev)            # ... and its device work is excluded with it
                T["emulation"] += clock() - te
                full[b0:b1] = packed                       # (the share's own copy: what the collective would deliver)
                return full

            cols = (pos_b, end_b, strand_b, label_b)
            if src.reorder:
                local, start, end, strand, label = _gather_rows(local, cols, n, group, T, "pack_rows", stand_in if emulated and world > 1 else None)
                t0 = clock()
                grp, order = torch.sort(_bed_reader_keys(start, strand, [hi - lo for lo, hi in runs], anchor, central_bp), stable=True)
                local = local[order]                       # (n, k + 1) probabilities + focal base in bed_reader order
                start, strand = start[order], strand[order]
                end, label = (end[order], label[order]) if tail.need_meta else (None, None)
                file_rows = torch.cat([torch.arange(lo, hi, device=tdev) for lo, hi in runs])[order] if collect else None
                T["reorder"] += clock() - t0
                cols = (start, end, strand, label)
            else:                                          # rows in the table's order: the ranks' blocks one after the other are the shard
                if world > 1:                              # (the pack has no timing key of its own here: it goes with the gather)
                    local, *cols = (c.contiguous() for c in _gather_rows(local, cols, n, group, T, "gather"))
                grp, file_rows = None, torch.arange(*runs[0], device=tdev) if collect else None
            tail(chrom, runs, local, *cols, grp, file_rows)
        if finish is not None:                             # (inside the frame: what it raises aborts the sink)
            finish()
    return tail.result(rows_all, None)


def _predict_bed_whole(forward, bed_path, segment_center, model_type, group, sink, collect, timings):
    """Every rank parses the whole BED (see predict_bed_sharded, ingest="whole")."""
    from .data import ingest
    rank, world = _rank_world(group, None)
    T = {} if timings is None else timings
    clock = time.perf_counter
    t0 = clock()
    sites = ingest.read_bed(bed_path)
    T["bed_read"] = clock() - t0
    t0 = clock()
    order, grp = ingest.bed_order(sites, segment_center)
    T["bed_order"] = clock() - t0
    n_all = len(order)
    dev = _device_of(forward)
    tail = _ShardTail(forward, model_type == "snv", sink, collect, T, dev, rank)
    t0 = clock()
    if dev is not None:
        # every column once to the device in FILE order; the bed_reader order is applied there (gathers at HBM speed)
        up = lambda a: torch.from_numpy(a).to(dev)                                            # noqa: E731
        order_d = up(order)
        cid_o = up(sites.chrom_id)[order_d]
        cut = torch.nonzero(cid_o[1:] != cid_o[:-1]).flatten().cpu().numpy() + 1 if n_all else np.zeros(0, np.int64)
        bounds = np.r_[0, cut, n_all] if n_all else np.zeros(1, np.int64)
        run_ids = cid_o[torch.from_numpy(bounds[:-1]).to(dev)].cpu().numpy() if n_all else np.zeros(0, np.int32)
        start_o, strand_o = up(sites.start)[order_d], up(sites.strand)[order_d]
        end_o = label_o = None
        if tail.need_meta:
            end_o, label_o = up(sites.end)[order_d], up(sites.score)[order_d]
        grp_o = up(grp)
        del cid_o
    else:
        cid_h = sites.chrom_id[order]
        runs = shard_runs(cid_h)
        bounds = np.array([lo for lo, _ in runs] + [n_all], np.int64)
        run_ids = np.array([cid_h[lo] for lo, _ in runs], np.int32)
        start_o, strand_o = sites.start[order], sites.strand[order]
        end_o, label_o = sites.end[order], sites.score[order]
        grp_o = grp
    T["order_columns"] = clock() - t0
    by_id = {}
    for i, c in enumerate(run_ids.tolist()):
        by_id.setdefault(c, []).append((int(bounds[i]), int(bounds[i + 1])))
    shards = [(sites.chrom_names[c], by_id[c]) for c in sorted(by_id, key=lambda c: sites.chrom_names[c])]

    def take(col, runs):
        if col is None:
            return None
        if len(runs) == 1:
            return col[runs[0][0]:runs[0][1]]
        parts = [col[lo:hi] for lo, hi in runs]
        return torch.cat(parts) if isinstance(col, torch.Tensor) else np.concatenate(parts)

    with tail.frame():
        for si, (chrom, runs) in enumerate(shards):
            n = sum(hi - lo for lo, hi in runs)
            b0, b1 = shard_bounds(n, rank, world)
            pos_s, strand_s = take(start_o, runs), take(strand_o, runs)
            if hasattr(forward, "prefetch") and si + 1 < len(shards):
                forward.prefetch(shards[si + 1][0])
            # (this route has never normalised the forward's dtype: only the probabilities are gathered, and they go out as they came)
            local = _forward_rows(forward, chrom, pos_s[b0:b1], strand_s[b0:b1], b1 - b0, T, normalise=False)
            t0 = clock()
            full = all_gather_rows(local, n, group)
            T["gather"] += clock() - t0
            tail(chrom, runs, full, pos_s, take(end_o, runs), strand_s, take(label_o, runs), take(grp_o, runs))
    return tail.result(n_all, order)


# ------------------------------------------------------------------------------------------------------------------
# Prediction over genomic regions: the sites are enumerated on the device from the resident genome (csrc/sites.hip,
# PackedGenome.scan_sites / emit_sites) instead of being read from a BED file with one row per site.  The reference has no
# counterpart: its users write that BED with scripts of their own.
# ------------------------------------------------------------------------------------------------------------------
REGION_END = 1 << 62       # "to the end of the record" (the enumeration clamps every window to the record)


def _merge_intervals(intervals):
    """Sorted disjoint [lo, hi) intervals; overlapping and touching ones merged, empty ones dropped."""
    out = []
    for lo, hi in sorted((int(a), int(b)) for a, b in intervals if b > a):
        if out and lo <= out[-1][1]:
            out[-1][1] = max(out[-1][1], hi)
        else:
            out.append([lo, hi])
    return [(lo, hi) for lo, hi in out]


def read_regions_arg(spec):
    """{chrom: [(lo, hi), ..]} -- sorted, disjoint, 0-based half-open -- of a region argument or a list of them:
    ``chr`` (the whole record: (0, REGION_END)), ``chr:start-end`` (1-based inclusive, as users write it) or the path of an existing BED-like file of regions (0-based half-open, extra columns ignored, plain or gzip:
    ``tables.read_regions``).  Overlapping or touching regions are merged, so no site is enumerated twice.  Raises ValueError naming
    the argument."""
    specs = [spec] if isinstance(spec, (str, os.PathLike)) else list(spec)
    found = {}
    for sp in specs:
        sp = os.fspath(sp)
        if os.path.isfile(sp):
            from .tables import read_regions
            try:
                table = read_regions(sp)
            except ValueError as e:
                raise ValueError(f"regions {sp!r}: {e}") from None
            if not table:
                raise ValueError(f"regions {sp!r}: the file holds no region")
            for chrom, (starts, ends) in table.items():
                for lo, hi in zip(starts, ends):
                    if lo < 0 or hi < lo:
                        raise ValueError(f"regions {sp!r}: bad interval {chrom} {lo} {hi}")
                    found.setdefault(chrom, []).append((lo, hi))
        elif ":" in sp:
            chrom, _, span = sp.rpartition(":")
            m = re.fullmatch(r"([0-9]+)-([0-9]+)", span)
            if not chrom or m is None:
                raise ValueError(f"regions {sp!r}: expected chr, chr:start-end (1-based, inclusive) or the path of a BED file")
            a, b = int(m.group(1)), int(m.group(2))
            if a < 1 or b < a:
                raise ValueError(f"regions {sp!r}: start must be at least 1 and end at least start")
            found.setdefault(chrom, []).append((a - 1, b))
        elif sp.strip():
            found.setdefault(sp, []).append((0, REGION_END))
        else:
            raise ValueError(f"regions {sp!r}: empty argument")
    return {chrom: _merge_intervals(iv) for chrom, iv in found.items()}


def _region_pieces(cum, a, b):
    """Sites [a, b) of a chromosome's enumeration -- its regions' enumerations one after the other, `cum` their running totals
    (cum[0] = 0) -- as [(region, first site within the region, sites)] in ascending order, empty pieces left out."""
    out = []
    for j in range(max(int(np.searchsorted(cum, a, "right")) - 1, 0), int(np.searchsorted(cum, b, "left"))):
        s0, s1 = max(a, int(cum[j])), min(b, int(cum[j + 1]))
        if s1 > s0:
            out.append((j, s0 - int(cum[j]), s1 - s0))
    return out


def mutations_for_regions(mutations, regions):
    """{chrom of `regions`: (its list (start, strand, label) or None, list rows inside the chromosome's merged regions)}: what a regions
    run takes from a mutation list ({chrom: (start ascending, strand, label)}, data.ingest.read_mutations).  Chromosomes that only the
    list names are left out; a chromosome that only the regions name has no list (every label 0)."""
    out = {}
    for chrom, intervals in regions.items():
        listed = mutations.get(chrom)
        if listed is None or len(listed[0]) == 0:
            out[chrom] = (None, 0)
            continue
        iv = np.asarray(intervals, np.int64).reshape(-1, 2)                        # (merged: sorted and disjoint)
        start = np.asarray(listed[0], np.int64)
        at = np.searchsorted(iv[:, 0], start, "right") - 1
        out[chrom] = (listed, int(((at >= 0) & (start < iv[np.maximum(at, 0), 1])).sum()) if len(iv) else 0)
    return out


class _RegionSites:
    """Site source of predict_regions_sharded: a chromosome's sites are its regions' enumerations one after the other.  The enumeration
    ascends, so the rows are always in the table's order and a gathered shard needs no reorder; the sites are chosen BY their base, so
    the per-(segment, strand) focal-base check of the BED path cannot fail and is skipped.

    `mutations` ({chrom: (start, strand, label)}, data.ingest.read_mutations) gives the rows their labels: a chromosome's list goes to
    the device once (open), every part's label column is a lookup in it (columns: data.genome.label_sites, this rank's slice only), and
    the two `stats` words come back once per chromosome behind its last part (done)."""
    check_focal = reorder = False
    read_key = "enumerate"

    def __init__(self, forward, regions, focal, context, dev, T, mutations=None, check_strand=False, classes=None):
        self.forward, self.regions, self.focal, self.context, self.dev, self.T = forward, regions, focal, context, dev, T
        self.classes = classes                             # focal "SET": the union of site classes that is enumerated
        self.names = sorted(regions)
        self.mutations, self.check_strand = None if mutations is None else mutations_for_regions(mutations, regions), check_strand
        self.in_regions = self.matched = 0
        if mutations is not None:
            T["label"] = 0.0
            self.in_regions = sum(inside for _, inside in self.mutations.values())

    def open(self, chrom, fetch_next):
        self.g = g = self.forward.genome(chrom)            # (KeyError for a chromosome the FASTA lacks, like the BED path)
        t0 = time.perf_counter()
        self.scans = [g.scan_sites(lo, hi, self.focal, self.context, self.classes) for lo, hi in self.regions[chrom]]
        fetch_next()                                       # right behind the enqueued scans, before the host waits for their totals
        self.muts = self.stats = None
        if self.mutations is not None:
            from .data.genome import new_label_stats
            self.stats = new_label_stats(self.dev)
            listed = self.mutations[chrom][0]
            if listed is not None:
                self.muts = tuple(torch.from_numpy(np.ascontiguousarray(a, dt)).to(self.dev)
                                  for a, dt in zip(listed, (np.int64, np.uint8, np.float32)))
        # the one read-back per chromosome: the totals size the outputs and the ranks' slices
        self.cum = np.r_[0, np.cumsum(torch.cat([sc.total_dev for sc in self.scans]).tolist() if self.scans else [])].astype(np.int64)
        self.T["enumerate"] += time.perf_counter() - t0
        return int(self.cum[-1]), True

    def columns(self, chrom, a, b):
        pos = torch.empty(b - a, dtype=torch.int64, device=self.dev)
        strand = torch.empty(b - a, dtype=torch.uint8, device=self.dev)
        o = 0
        for j, first, m in _region_pieces(self.cum, a, b):
            self.g.emit_sites(self.scans[j], first, m, pos[o:o + m], strand[o:o + m])
            o += m
        if self.mutations is None:
            return pos, pos + 1, strand, torch.zeros(b - a, dtype=torch.float32, device=self.dev)
        from .data.genome import label_sites
        t0 = time.perf_counter()
        label = label_sites(pos, strand, self.muts, self.check_strand, self.stats)
        self.T["label"] += time.perf_counter() - t0
        return pos, pos + 1, strand, label

    def done(self, chrom):
        """Behind the chromosome's last part: its `stats` words, read back once.  A listed mutation on the other strand than the site it
        lies on raises ValueError (inside the driver's frame: the sink is aborted, no table is left)."""
        if self.stats is None:
            return
        matched, wrong = self.stats.tolist()
        self.matched += matched
        if self.muts is not None and wrong < len(self.muts[0]):
            listed = self.mutations[chrom][0]
            start, st = int(listed[0][wrong]), int(listed[1][wrong])
            raise ValueError(f"mutations: {chrom}:{start} is listed on strand '{'+-'[st]}' but the site there is on strand "
                             f"'{'-+'[st]}' (the strand says which base mutated: A / C sites are '+', T / G sites '-')")

    def finish(self, group, world, emulated, strict):
        """The counts of the run -> timings['mutations']; `strict`: a listed mutation inside the regions that matched no site raises."""
        if self.mutations is None:
            return
        matched = self.matched
        if world > 1 and not emulated:
            total = torch.tensor([matched], dtype=torch.int64, device=self.dev)
            dist.all_reduce(total, group=group)
            matched = int(total.item())
        counts = {"in_regions": self.in_regions, "matched": matched, "unmatched": self.in_regions - matched}
        self.T["mutations"] = counts
        if strict and counts["unmatched"]:
            raise ValueError("mutations: %d of the %d listed mutations inside the regions lie on no enumerated site (%d matched): "
                             "another focal base or context, an N, or a wrong coordinate" % (counts["unmatched"], self.in_regions, matched))

    def layout(self, chrom, row0, n):
        return [(row0, row0 + n)], None                    # there is no input file: the rows count up in the table's order


def predict_regions_sharded(forward, regions, focal, context="all", model_type="snv", group=None, sink=None, collect=True, timings=None,
                            emulate=None, mutations=None, strict_mutations=False):
    """predict_bed_sharded for sites that are not listed in a file but selected by their base: every A/T site (focal 'A'), every C/G
    site (focal 'C'; context 'all', 'CpG' or 'nonCpG') or, for INDEL models, every A/C/G/T position (focal 'ANY') of `regions` (what
    read_regions_arg returns, or its argument).  Same forward (HipShardForward: a HIP ``device`` and ``genome(chrom)``), sinks, `timings`,
    `emulate` and return value as predict_bed_sharded; rows carry end = start + 1 and label 0 (`mutations`: below).  With `collect` the returned rows are in the
    table's order -- ascending chromosome name, then start: there is no input file whose order could be kept -- and `order` counts them.

    focal 'SET' goes with a ModelSetForward (and only with one): the sites of every class the set has a member for, in one ascending
    enumeration, every row computed by the model of its class -- one table of the rate at every selected base, its prob columns the
    substitutions of the row's own base (which strand and genome determine).  One `mutations` list serves all members.

    Chromosomes go in ascending name order, the next one is packed while this one is computed.  Per chromosome the regions are counted
    on the device (one read-back of the totals), rank i of N takes the slice shard_bounds(sites of the chromosome, i, N) of the
    enumeration and emits it in parts of at most _ALIGNED_PART_ROWS sites.  The enumeration ascends, so with a consumer of aligned
    blocks (a TsvSink, every rank's with parts=True; collect=False) a rank's rows are its slice of the table: nothing is gathered or
    sorted.  A caller that wants all rows back, or a sink on rank 0 alone, gets one all_gather per chromosome instead.

    `mutations`: the observed side -- the path of a BED of the mutated sites (data.ingest.read_mutations: chrom start end name score
    strand, score = mut_type, checked against the model's n_class) or what read_mutations returns.  A row whose position is a listed
    start carries that entry's label, every other row 0: the table is the one the BED path writes for a BED with every enumerated site
    and those scores.  The join is a lookup per site on the device in front of the forward (csrc/sites.hip: mural_sites_label), on every
    rank for its own slice; nothing is gathered for it.  Chromosomes of the list that the regions lack are ignored.  For the SNV
    selections a listed mutation on the other strand than the site it lies on raises ValueError (chromosome, start, both strands); like
    every failure it leaves no table (under a process group the rank whose slice holds the site raises; the others fail with it at
    their next collective).  Listed mutations inside the regions that lie on NO enumerated site (the other focal base, an N,
    outside the CpG selection: one list may serve several models) are counted, and raise ValueError only with `strict_mutations`.
    timings['mutations'] = {in_regions, matched, unmatched = in_regions - matched}: `in_regions` counts the list's rows inside the
    merged regions on the host, `matched` is summed over the ranks of a process group with one all_reduce at the end of the run; an
    emulated rank (`emulate=`) reports the matches of ITS slice alone, so `unmatched` means nothing there and `strict_mutations` is
    refused.  timings['label'] are the host seconds spent enqueueing the lookups (without `mutations` neither key appears)."""
    from .data.genome import site_selection
    classes = None
    if str(focal).upper() == "SET":
        if not isinstance(forward, ModelSetForward):
            raise ValueError("focal 'SET' enumerates the site classes of a ModelSetForward: this forward serves one model, name its "
                             "selection (focal 'A' / 'C' with a context, 'ANY')")
        classes = forward.classes
    elif isinstance(forward, ModelSetForward):
        raise ValueError(f"a ModelSetForward serves the union of its members' site classes: focal 'SET', not {focal!r}")
    f_code, _ = site_selection(focal, context, classes)
    if model_type not in ("snv", "indel"):
        raise ValueError(f"model_type {model_type} not supported!")
    if (f_code == 2) != (model_type == "indel"):
        raise ValueError(f"focal {focal!r} does not go with model_type {model_type!r}: 'ANY' is the INDEL models' selection, "
                         "'A' / 'C' the SNV models'")
    if not isinstance(regions, dict):
        regions = read_regions_arg(regions)
    dev = _device_of(forward)
    if dev is None or not hasattr(forward, "genome"):
        raise ValueError("predict_regions_sharded enumerates the sites on the device: the forward needs a HIP device and genome(chrom)")
    rank, world = _rank_world(group, emulate)
    T = {} if timings is None else timings
    T.update({"emulation": 0.0, "enumerate": 0.0})
    if emulate is not None and world > 1 and not _takes_aligned_blocks(sink, collect, world):
        raise ValueError("emulate=(rank, world) needs collect=False and a part-file sink: one rank cannot stand in for a gather")
    if strict_mutations and (mutations is None or (emulate is not None and world > 1)):
        raise ValueError("strict_mutations needs mutations= and every rank's matches: it does not go with emulate=(rank, world)")
    if mutations is not None and not isinstance(mutations, dict):
        from .data.ingest import read_mutations
        mutations = read_mutations(mutations, getattr(getattr(forward, "model", None), "n_class", None))
    src = _RegionSites(forward, regions, focal, context, dev, T, mutations, check_strand=f_code != 2, classes=classes)
    emulated = emulate is not None
    return _predict_shards(forward, src, 0, model_type, group, sink, collect, T, rank, world, emulated,
                           finish=lambda: src.finish(group, world, emulated, strict_mutations))
