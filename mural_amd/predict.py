"""Sharded genome-wide prediction: one process per GPU, sites split into contiguous blocks, ONE RCCL all_gather of the
per-rank probabilities per call (the reference itself is single-process and only advises to
split the BED file by hand, MuRaL/commands/predict.py:134-137).

The host logic (block partition, padded all_gather, trimming back to the reference's row order) is backend-agnostic
and covered by world_size-2 gloo tests on CPU; the compute function is the HIP model's ``forward_packed`` /
``forward_packed_reuse``.  What consumes the shards lives beside this module: the prediction table in ``sinks`` (TsvSink, TeeSink),
the summaries reduced in flight in ``summaries`` (SummarySink and its numpy twins).
"""
import contextlib
import os
import re
import threading
import time

import numpy as np
import torch
import torch.distributed as dist

from . import _lib
# the names that moved to sinks.py and summaries.py, re-exported: bench.py, the tools and the tests import them from here
from .mutagenesis import (MutagenesisMap, encode_subst_windows_host, mutagenesis_reduce_host, mutagenesis_rows_host,  # noqa: F401
                          saturation_mutagenesis, variant_footprint)
from .sinks import (TeeSink, TsvSink, _name_table, _np, _tsv_struct, format_rows_host, shard_bounds,  # noqa: F401
                    write_predictions)
from .summaries import (_MOTIF_ORD_SHIFT, _MOTIF_POS_SHIFT, SummarySink, _calib_fold, _calib_lo_cells, _kmer_collapse,  # noqa: F401
                        _kmer_fold, _kmer_merge, annot_table_from_sums, calib_bounds, calib_cells, calib_metrics_from_sums,
                        calib_rows_device, kmer_keys_host, kmer_table_from_sums, motif_table_from_sums, summary_annot_host,
                        summary_calib_host, summary_conseq_host, summary_kmer_host, summary_motif_host, summary_rows_host,
                        summary_txindel_host, summary_txstruct_host)


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
