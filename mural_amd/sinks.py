"""The consumers of the shards of a file-level prediction (mural_amd.predict: one shard = the rows of one chromosome): ``TsvSink`` writes
the prediction table, formatted by ``csrc/tsv.hip`` (device kernel or host threads), ``TeeSink`` feeds several consumers from one
shard loop; ``write_predictions`` is the table of a collected result.  ``summaries.SummarySink`` is the third consumer; the helpers
that read a shard (its name, its strand column, the host calibration) are shared with it."""
import ctypes as C
import os
import queue
import threading
import time

import numpy as np
import torch
import torch.distributed as dist

from . import _lib


def shard_bounds(n, rank, world):
    """Contiguous block [lo, hi) of `n` rows for `rank`: the first n % world ranks take one extra row.  (Here because the part-file
    sinks slice a sorted shard by it; the gather and the shard loop of mural_amd.predict split their rows the same way.)"""
    if world <= 0 or not (0 <= rank < world):
        raise ValueError(f"bad rank/world {rank}/{world}")
    base, extra = divmod(n, world)
    lo = rank * base + min(rank, extra)
    return lo, lo + base + (1 if rank < extra else 0)


def _np(a):
    return a.detach().cpu().numpy() if isinstance(a, torch.Tensor) else np.asarray(a)


def shard_name(shard):
    """The chromosome name of a shard (``chrom``: the name, or an array whose first entry is the name); None for a shard without rows."""
    c = shard["chrom"]
    if isinstance(c, str):
        return c
    return str(c[0]) if len(c) else None


def strand_u8(s):
    """A strand column as uint8 (1 = '-'): tensors and uint8 arrays as they are, '+' / '-' strings converted."""
    if isinstance(s, torch.Tensor):
        return s
    s = np.asarray(s)
    return s if s.dtype == np.uint8 else (s == "-").astype(np.uint8)


def host_calibrate(prob, poisson, dirichlet_weights):
    """The calibration chain of run_predict.py:217-225 on host probabilities: Dirichlet, then Poisson, each where asked for."""
    prob = np.asarray(prob)
    if dirichlet_weights is not None:
        from .calibration import dirichlet_calibrate
        prob = dirichlet_calibrate(prob, dirichlet_weights)
    if poisson:
        from .data.ingest import poisson_calibrate
        prob = poisson_calibrate(prob)
    return prob


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

    # -- streaming --------------------------------------------------------------------------------------------------------
    def _stream_host(self, name, shard):
        t0 = time.perf_counter()
        prob = host_calibrate(shard["prob"], self.poisson, self.dirichlet_weights)
        start = np.asarray(shard["start"])
        if shard.get("aligned"):       # this rank's own rows, already in the table's order (predict_bed_sharded: _ShardTail.aligned)
            perm = np.arange(len(start), dtype=np.int64)
        else:
            perm = np.argsort(start, kind="stable")
            if self.parts:
                s0, s1 = shard_bounds(len(perm), self.rank, self.world)
                perm = perm[s0:s1]
        text = format_rows_host([name], None, start, shard["end"], strand_u8(shard["strand"]), shard["label"], prob, perm,
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
            strand, label = to(strand_u8(shard["strand"]), torch.uint8), to(shard["label"], torch.float32)
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
        name = shard_name(shard)
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
                            "strand": cpu(strand_u8(shard["strand"])), "label": cpu(shard["label"]),
                            "prob": host_calibrate(cpu(shard["prob"])[:, :k], self.poisson, self.dirichlet_weights)})

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
    _refuse_second_calibration(res, poisson, dirichlet_weights)
    prob = host_calibrate(res["prob"], poisson, dirichlet_weights)
    chrom = np.asarray(res["chrom"], dtype=object)
    n = len(chrom)
    names = sorted(set(chrom.tolist()))
    rank = {nm: i for i, nm in enumerate(names)}
    cid = np.fromiter((rank[c] for c in chrom), np.int32, n)
    start = np.asarray(res["start"], np.int64)
    perm = np.lexsort((start, cid))                     # stable, like pandas' multi-column sort_values
    strand = strand_u8(res["strand"])
    k = prob.shape[1] if prob.ndim == 2 else 0
    with open(path, "wb") as fh:
        fh.write(_header(k))
        if n:
            fh.write(format_rows_host(names, cid, start, res["end"], strand, np.asarray(res["label"], np.float32), prob, perm))
    return n
