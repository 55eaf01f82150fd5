"""The prediction table read back on the device: ``evaluate`` (k-mer and regional correlations), ``calc_scaling_factor`` and
``scale`` on the files ``predict`` writes (columns ``chrom start end strand mut_type prob0 .. prob{n-1}``, plain or gzip).

The entry points carry the names and ``args`` contracts the reference's CLI dispatches to (MuRaL/mural_snv.py:108-124,
MuRaL/mural_indel.py:109-135): switching the imports there is the whole integration.  The reference parses the
table row by row in Python (MuRaL/scripts/calc_kmer_corr.py, calc_regional_corr.py) or loads it whole with pandas
(MuRaL/scripts/scaling.py); here a streaming reader (csrc/tables.hip) parses it chunk by chunk on the device and the per-row work is
device kernels, the existing '%.4g' row formatter (csrc/tsv.hip) and the group tables of csrc/analytics.hip included.

``chunk_bytes`` (keyword of every function) is the target size of one chunk of text.

Known deviation: pandas re-types a chromosome name that looks like a number when ``scale`` reads the table (``01`` is written back
as ``1``); here every name is kept verbatim.
"""
import concurrent.futures
import ctypes as C
import gzip
import os
import sys
import zlib

import numpy as np
import torch

from . import _lib

DEFAULT_CHUNK_BYTES = 64 << 20
MAX_KMER = 10
# the motif tables are indexed by all 4^m keys, 3 n_class cells of 8 bytes each: 50 MB at m = 9 and 805 MB at m = 11 with 8 classes (half
# of that with 4), once on the device and once on the host when it is read back; m = 13 would take 12.9 GB
MAX_MOTIF = 11
_NAME_STRIDE = 256
_GZ_THREADS = 16
_GZ_BLOCK = 4 << 20


# ------------------------------------------------------------------------------------------------------------------
# header, file names, arguments (host logic)
# ------------------------------------------------------------------------------------------------------------------
def _is_gzip(path):
    with open(path, "rb") as fh:
        return fh.read(2) == b"\x1f\x8b"


def read_header(path):
    """The first line of a prediction table (plain or gzip), without its line end."""
    opener = gzip.open if _is_gzip(path) else open
    with opener(path, "rt") as fh:
        return fh.readline().rstrip("\r\n")


def check_header(header, n_class):
    """The header check of calc_kmer_corr.py:208-218 / calc_regional_corr.py:178-188: ValueError with the reference's message."""
    if not header.startswith("chrom"):
        raise ValueError(f"Invalid file header: {header.strip()}, header should be continue with 'chrom'")
    fields = header.strip().split("\t")
    if len(fields) != n_class + 5:
        raise ValueError(f"Column count mismatch. Expected {n_class + 5} columns, got {len(fields)} in line: {fields}")
    return fields


def kmer_output_names(out_prefix, kmer_length):
    return f"{out_prefix}.{kmer_length}-mer.mut_rates.tsv", f"{out_prefix}.{kmer_length}-mer.corr.txt"


def regional_output_names(out_prefix, window_size):
    window = f"{int(int(window_size) / 1000)}Kb"
    return f"{out_prefix}.{window}.mut_rates.tsv", f"{out_prefix}.{window}.corr.txt", window


def scaled_output_name(pred_file):
    return pred_file + ".scaled.tsv.gz"


def check_kmer_length(k):
    k = int(k)
    if k < 1:
        raise ValueError(f"--kmer_length must be positive (got {k})")
    if k > MAX_KMER:
        raise ValueError(f"--kmer_length {k} is larger than {MAX_KMER}: the k-mer table has 4^k groups")
    return k


def motif_output_names(out_prefix, motif_length):
    return f"{out_prefix}.{motif_length}-motif.mut_rates.tsv", f"{out_prefix}.{motif_length}-motif.corr.txt"


def check_motif_length(m, device=False):
    """validate_motif_length of calc_motif_corr.py:83-87 (its message), and the upper bound of the tables here: ``MAX_MOTIF`` (15, the
    largest key of 32 bits, for a direct call of the device entry with `device`)."""
    m = int(m)
    if m <= 1 or m % 2 != 1:
        raise ValueError("--motif_length must be a positive odd integer >1")
    top = 15 if device else MAX_MOTIF
    if m > top:
        raise ValueError(f"--motif_length {m} is larger than {top}: the motif table has 4^m entries")
    return m


_STRAND_MODES = {"+": 1, "pos": 1, "-": 2, "neg": 2, "both": 3}


def strand_mode(model_type, strand=None):
    """0: each row's own strand (SNV); INDEL: --strand as given (pos / neg / both, or the '+' / '-' / 'both' the CLI maps it to)."""
    if model_type == "snv":
        return 0
    if model_type != "indel":
        raise ValueError(f"model_type {model_type} not supported!")
    if strand not in _STRAND_MODES:
        raise ValueError(f"Invalid strand: {strand}")
    return _STRAND_MODES[strand]


def kmer_name(key, k):
    return "".join("ACGT"[(key >> (2 * (k - 1 - j))) & 3] for j in range(k))


def pearson(x, y):
    """(r, p) of scipy.stats.pearsonr (host work on the small table); p is NaN when SciPy is not installed."""
    try:
        from scipy.stats import pearsonr
    except ImportError:
        from .evaluation import _pearson
        return _pearson(x, y), float("nan")
    res = pearsonr(x, y)
    return float(res[0]), float(res[1])


def _float_text(v):
    return repr(float(v))


def _rates_text(header, rows):
    return "\t".join(header) + "\n" + "".join("\t".join(r) + "\n" for r in rows)


def _corr_text(label, corrs):
    return "".join(f"{label}\t{c}\t{r:.5f}\t{p:.10e}\n" for c, (r, p) in corrs)


# ------------------------------------------------------------------------------------------------------------------
# the streaming reader
# ------------------------------------------------------------------------------------------------------------------
class TableReader:
    """Chunks of a prediction table parsed on the current HIP device (``for chunk in reader``: a ``MuralTableChunk`` whose device
    columns are valid until the next step)."""

    def __init__(self, path, n_class, chunk_bytes=DEFAULT_CHUNK_BYTES):
        self._h = C.c_void_p()
        if not torch.cuda.is_available():
            raise RuntimeError("mural_amd.tables needs a HIP device; there is no CPU path")
        path = os.fspath(path)
        self.header = check_header(read_header(path), n_class)
        self.n_class = int(n_class)
        self.device = torch.device("cuda", torch.cuda.current_device())
        _lib.check(_lib.lib().mural_table_open(path.encode(), self.n_class, int(chunk_bytes), C.byref(self._h)))

    def close(self):
        if self._h:
            _lib.lib().mural_table_close(self._h)
            self._h = C.c_void_p()

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    def __del__(self):
        self.close()

    def __iter__(self):
        lib = _lib.lib()
        while True:
            c = _lib.MuralTableChunk()
            _lib.check(lib.mural_table_next(self._h, C.byref(c), _lib.current_stream_ptr(self.device)))
            if c.n_rows == 0:
                return
            yield c

    def chrom_name(self, cid):
        return _lib.lib().mural_table_chrom_name(self._h, int(cid)).decode()

    def chrom_names(self, n):
        return [self.chrom_name(i) for i in range(n)]

    def stats(self):
        out = (C.c_double * 4)()
        _lib.check(_lib.lib().mural_table_stats(self._h, out))
        return dict(read_s=out[0], wait_read_s=out[1], parse_s=out[2], text_bytes=int(out[3]))


def _name_table(names):
    buf = C.create_string_buffer(max(len(names), 1) * _NAME_STRIDE)
    for i, nm in enumerate(names):
        raw = nm.encode()
        if len(raw) >= _NAME_STRIDE:
            raise ValueError(f"chromosome name longer than {_NAME_STRIDE - 1} bytes: {nm!r}")
        buf[i * _NAME_STRIDE:i * _NAME_STRIDE + len(raw)] = raw
    return buf


# ------------------------------------------------------------------------------------------------------------------
# scale
# ------------------------------------------------------------------------------------------------------------------
class _Out:
    """Text sink: a plain file, or gzip written as independent members compressed on up to 16 host threads."""

    def __init__(self, path):
        self.fh = open(path, "wb")
        self.gz = str(path).endswith(".gz")
        self.pool = concurrent.futures.ThreadPoolExecutor(_GZ_THREADS) if self.gz else None

    @staticmethod
    def _member(data):
        z = zlib.compressobj(6, zlib.DEFLATED, 31)
        return z.compress(data) + z.flush()

    def write(self, data):
        if not self.gz:
            self.fh.write(data)
            return
        mv = memoryview(data)
        parts = [mv[i:i + _GZ_BLOCK] for i in range(0, len(mv), _GZ_BLOCK)]
        for blob in self.pool.map(self._member, parts):
            self.fh.write(blob)

    def close(self):
        if self.pool is not None:
            self.pool.shutdown()
        self.fh.close()


def _scale_file(pred_file, factor, n_class, out_file, chunk_bytes, timing=None):
    lib = _lib.lib()
    with TableReader(pred_file, n_class, chunk_bytes) as rd:
        out = _Out(out_file)
        try:
            out.write(("\t".join(rd.header) + "\n").encode())
            dev = rd.device
            text = ws = host = None
            count = torch.zeros(1, dtype=torch.int64, device=dev)
            for c in rd:
                n = int(c.n_rows)
                _lib.check(lib.mural_table_scale_rows(c.prob, n, n_class, float(factor), _lib.current_stream_ptr(dev)))
                names = _name_table(rd.chrom_names(c.n_chroms))
                t = _lib.MuralTsvRows()
                t.chrom_names, t.n_chroms, t.name_stride = C.cast(names, C.c_char_p), max(c.n_chroms, 1), _NAME_STRIDE
                t.chrom_id, t.start, t.end, t.strand, t.label, t.prob = c.chrom_id, c.start, c.end, c.strand, c.label, c.prob
                t.prob_f64, t.n_class, t.prob_stride, t.perm, t.n, t.layout = 1, n_class, n_class, None, n, 0
                bound = int(lib.mural_tsv_row_bound(C.byref(t)))
                if bound < 0:
                    raise ValueError("prediction table: bad row layout")
                need = n * bound
                if text is None or text.numel() < need:
                    text = torch.empty(need, dtype=torch.uint8, device=dev)
                    host = torch.empty(need, dtype=torch.uint8).pin_memory()
                ws_need = int(lib.mural_tsv_format_workspace_bytes(n)) + max(c.n_chroms, 1) * _NAME_STRIDE + 16
                if ws is None or ws.numel() < ws_need:
                    ws = torch.empty(ws_need, dtype=torch.uint8, device=dev)
                _lib.check(lib.mural_tsv_format_device(C.byref(t), text.data_ptr(), text.numel(), count.data_ptr(), ws.data_ptr(),
                                                      ws.numel(), _lib.current_stream_ptr(dev)))
                nb = int(count.item())
                host[:nb].copy_(text[:nb])
                out.write(host[:nb].numpy().tobytes())
            if timing is not None:
                timing.update(rd.stats())
        finally:
            out.close()


def apply_scaling_file(pred_file, scale_factor, n_class, out_file, chunk_bytes=DEFAULT_CHUNK_BYTES):
    """scaling.py:10-28 (apply_scaling) on a table file: prob1.. *= scale_factor, prob0 = 1 - their sum, rows in file order, floats
    '%.4g'; an out_file ending in .gz is written as gzip.  (The in-memory rule is ``mural_amd.calibration.apply_scaling``.)"""
    _scale_file(os.fspath(pred_file), float(scale_factor), int(n_class), os.fspath(out_file), chunk_bytes)


def scaling_files(pred_files, scale_factors, n_class, out_files, chunk_bytes=DEFAULT_CHUNK_BYTES):
    """scaling.py:30-40: apply_scaling_file over parallel lists."""
    if not isinstance(pred_files, list) or not isinstance(scale_factors, list) or not isinstance(out_files, list):
        print("ERROR: pred_files, scale_factors, and out_files must be lists!", file=sys.stderr)
        sys.exit()
    for pred_file, factor, out_file in zip(pred_files, scale_factors, out_files):
        apply_scaling_file(pred_file, factor, n_class, out_file, chunk_bytes=chunk_bytes)


# ------------------------------------------------------------------------------------------------------------------
# calc_scaling_factor
# ------------------------------------------------------------------------------------------------------------------
def read_regions(path):
    """{chrom: (starts, ends)} of a BED file (the first three columns; plain or gzip; track / browser / '#' lines skipped).  The
    region list is small: host work."""
    opener = gzip.open if _is_gzip(path) else open
    out = {}
    with opener(path, "rt") as fh:
        for ln, line in enumerate(fh, 1):
            if not line.strip() or line.startswith(("#", "track", "browser")):
                continue
            f = line.rstrip("\r\n").split("\t")
            if len(f) < 3:
                raise ValueError(f"{path}:{ln}: a BED row needs chrom, start and end")
            a, b = out.setdefault(f[0], ([], []))
            a.append(int(f[1]))
            b.append(int(f[2]))
    return out


def _regions_on_device(regions, names, dev):
    """Benchmark regions per table chromosome: (offsets [n+1], each chromosome's sorted starts, its sorted ends) on `dev`."""
    b0, b1, off = [], [], [0]
    for nm in names:
        a, b = regions.get(nm, ([], []))
        b0.append(np.sort(np.asarray(a, np.int64)))
        b1.append(np.sort(np.asarray(b, np.int64)))
        off.append(off[-1] + len(a))
    cat = lambda xs: torch.from_numpy(np.concatenate(xs + [np.zeros(1, np.int64)])).to(dev)      # noqa: E731
    return torch.tensor(off, dtype=torch.int64, device=dev), cat(b0), cat(b1)


def prob_sum_file(pred_file, n_class, benchmark_regions=None, chunk_bytes=DEFAULT_CHUNK_BYTES):
    """(sum over rows of prob1 + .. + prob{n-1}, n_sites) of a table; with benchmark regions each row counts once per overlapping
    region (bedtools intersect without -u).  float64, fixed reduction order."""
    lib = _lib.lib()
    nb = int(lib.mural_table_prob_sum_blocks())
    total, n_sites = 0.0, 0
    with TableReader(pred_file, n_class, chunk_bytes) as rd:
        dev = rd.device
        part_s = torch.zeros(nb, dtype=torch.float64, device=dev)
        part_c = torch.zeros(nb, dtype=torch.int64, device=dev)
        chunks = []
        bed = read_regions(benchmark_regions) if benchmark_regions else None
        regions, reg_names = None, 0
        for c in rd:
            if bed is not None and (regions is None or reg_names < c.n_chroms):
                reg_names = c.n_chroms
                regions = _regions_on_device(bed, rd.chrom_names(reg_names), dev)
            ro, r0, r1 = (regions[0].data_ptr(), regions[1].data_ptr(), regions[2].data_ptr()) if regions else (None, None, None)
            _lib.check(lib.mural_table_prob_sum(c.prob, c.chrom_id, c.start, c.end, c.n_rows, n_class, ro, r0, r1, reg_names,
                                               part_s.data_ptr(), part_c.data_ptr(), _lib.current_stream_ptr(dev)))
            chunks.append((part_s.cpu().numpy().copy(), part_c.cpu().numpy().copy()))
        for s, k in chunks:
            for v in s:
                total += float(v)
            n_sites += int(k.sum())
    return total, n_sites


def calc_mu_scaling_factor(args, model_type, chunk_bytes=DEFAULT_CHUNK_BYTES):
    """scaling.py:45-107: per prediction file the factor genomewide_mu * n_sites * m_proportion / g_proportion / prob_sum (g = 1
    for INDEL); prints the reference's lines, writes <pred>.scaled.tsv.gz with --do_scaling, returns the factors."""
    pred_files = list(args.pred_files)
    g_props = list(args.g_proportions) if model_type == "snv" else [1] * len(pred_files)
    m_props = list(args.m_proportions)
    if len(m_props) != len(pred_files):
        print("ERROR: length of proportions does not equal to length of pred_files!", file=sys.stderr)
        sys.exit()
    factors = []
    for i, pred_file in enumerate(pred_files):
        prob_sum, n_sites = prob_sum_file(pred_file, args.n_class, getattr(args, "benchmark_regions", None) or None, chunk_bytes)
        factor = mu_scaling_factor(args.genomewide_mu, n_sites, m_props[i], g_props[i], prob_sum)
        print("\nType " + str(i + 1) + ":\n" + "pred_file:", pred_file)
        print_scaling_factor(args.genomewide_mu, n_sites, g_props[i], m_props[i], prob_sum, factor)
        if args.do_scaling:
            apply_scaling_file(pred_file, factor, args.n_class, scaled_output_name(pred_file), chunk_bytes=chunk_bytes)
        factors.append(factor)
    return factors


# ------------------------------------------------------------------------------------------------------------------
# evaluate: k-mer
# ------------------------------------------------------------------------------------------------------------------
def _group(keys, c, n_class, n_groups, table, status, dev):
    _lib.check(_lib.lib().mural_eval_group_obs_pred(keys.data_ptr(), c.mut_type, c.prob, 1, c.n_rows, n_class, n_groups,
                                                   table.data_ptr(), status.data_ptr(), _lib.current_stream_ptr(dev)))


def _check_status(status, what):
    s = int(status.item())
    if s & 2:
        raise ValueError(f"{what}: a mut_type outside 0 .. n_class - 1")
    if s & 1:
        raise ValueError(f"{what}: a negative start")


def kmer_table(pred_file, ref_genome, kmer_length, n_class, model_type, strand=None, chunk_bytes=DEFAULT_CHUNK_BYTES):
    """(k-mer names, table [groups][1 + 2 n_class] of rows / per-class counts / per-class prob sums) in the reference's dict order."""
    from .data.ingest import read_fasta, scan_fasta
    k = check_kmer_length(kmer_length)
    mode = strand_mode(model_type, strand)
    lib = _lib.lib()
    n_groups = 4 ** k
    fasta_names = {r.name for r in scan_fasta(ref_genome)}
    genomes = {}
    with TableReader(pred_file, n_class, chunk_bytes) as rd:
        dev = rd.device
        stream = lambda: _lib.current_stream_ptr(dev)      # noqa: E731
        table = torch.zeros((n_groups, 1 + 2 * n_class), dtype=torch.float64, device=dev)
        first = torch.full((n_groups,), -1, dtype=torch.int64, device=dev)      # (all ones = the largest unsigned value)
        status = torch.zeros(1, dtype=torch.int32, device=dev)
        for c in rd:
            n = int(c.n_rows)
            key_a = torch.empty(n, dtype=torch.int32, device=dev)
            key_b = torch.empty(n, dtype=torch.int32, device=dev) if mode == 3 else None
            rows = list(c.run_row[:c.n_runs]) + [n]
            for r in range(c.n_runs):
                name = rd.chrom_name(c.run_chrom[r])
                if name not in genomes:
                    if name not in fasta_names:
                        raise ValueError(f"Chromosome {name} not found in {ref_genome} (prediction table line {c.row0 + rows[r] + 2})")
                    genomes[name] = read_fasta(ref_genome, dev, names={name})[name]
                g = genomes[name].as_struct()
                a, b = rows[r], rows[r + 1]
                _lib.check(lib.mural_table_kmer_keys(C.byref(g), c.start + 8 * a, c.end + 8 * a, c.strand + a, b - a, k,
                                                    int(model_type == "indel"), mode, key_a[a:].data_ptr(),
                                                    key_b[a:].data_ptr() if key_b is not None else None, stream()))
            for sub, keys in enumerate((key_a, key_b)):
                if keys is None:
                    continue
                _group(keys, c, n_class, n_groups, table, status, dev)
                _lib.check(lib.mural_table_first_row(keys.data_ptr(), n, c.row0, sub, n_groups, first.data_ptr(), stream()))
        _check_status(status, pred_file)
        table, first = table.cpu().numpy(), first.cpu().numpy().view(np.uint64)
    live = np.nonzero(table[:, 0] > 0)[0]
    order = live[np.argsort(first[live], kind="stable")]
    return [kmer_name(int(g), k) for g in order], table[order]


def _rates(table, n_class):
    tot = table[:, 1:1 + n_class].sum(axis=1)
    obs = table[:, 2:1 + n_class] / tot[:, None]
    pred = table[:, 2 + n_class:] / tot[:, None]
    return obs, pred, table[:, 2:1 + n_class].astype(np.int64), tot.astype(np.int64)


def run_kmer_corr_calc(args, model_type, chunk_bytes=DEFAULT_CHUNK_BYTES):
    """calc_kmer_corr.py:195-270: per k-mer observed / predicted rates and their Pearson r per class; writes
    {out_prefix}.{k}-mer.mut_rates.tsv and .corr.txt."""
    assert args.ref_genome is not None, "--ref_genome is required for k-mer correlation calculation"
    n_class = args.n_class
    names, table = kmer_table(os.fspath(args.pred_file), os.fspath(args.ref_genome), args.kmer_length, n_class, model_type,
                              getattr(args, "strand", None), chunk_bytes)
    return write_kmer_outputs(names, table, n_class, args.kmer_length, args.out_prefix)


def write_kmer_outputs(names, table, n_class, kmer_length, out_prefix):
    """The two files of calc_kmer_corr.py:252-270 from a k-mer table (``kmer_table``'s pair, or the one a ``predict.SummarySink``
    reduced in flight): per k-mer observed / predicted rates and counts, Pearson r per class.  Returns [(class, (r, p))]."""
    return _write_type_outputs(names, table, n_class, kmer_output_names(out_prefix, kmer_length), f"{kmer_length}-mer")


def _write_type_outputs(names, table, n_class, paths, label):
    obs, pred, cnt, tot = _rates(table, n_class)
    cls = range(1, n_class)
    header = (["type"] + [f"avg_obs_rate{i}" for i in cls] + [f"avg_pred_rate{i}" for i in cls] + [f"number_of_mut{i}" for i in cls]
              + ["number_of_all"])
    rows = [[nm] + [_float_text(v) for v in obs[j]] + [_float_text(v) for v in pred[j]] + [str(int(v)) for v in cnt[j]] + [str(int(tot[j]))]
            for j, nm in enumerate(names)]
    rates_path, corr_path = paths
    corrs = [(c, pearson(obs[:, c - 1], pred[:, c - 1])) for c in cls]
    with open(rates_path, "w") as fh:
        fh.write(_rates_text(header, rows))
    with open(corr_path, "w") as fh:
        fh.write(_corr_text(label, corrs))
    return corrs


# ------------------------------------------------------------------------------------------------------------------
# evaluate: motif
# ------------------------------------------------------------------------------------------------------------------
def motif_table(pred_file, ref_genome, motif_length, n_class, model_type, chunk_bytes=DEFAULT_CHUNK_BYTES):
    """(motif names, table [entries][1 + 2 n_class] of windows / per-class counts / per-class prob sums) in the reference's dict order
    (calc_motif_corr.py:191-254): every window of motif_length bases that holds a row's site, on the reference strand, a motif and its
    reverse complement in one entry named after the orientation seen first.  The chunks of the table go through the entry point of the
    in-flight reduction (``mural_summary_motif_rows``; ``predict.SummarySink(motifs=...)``), the rows' order being their line numbers."""
    from .data.ingest import read_fasta, scan_fasta
    from .summaries import _SUMMARY_STATUS, motif_table_from_sums      # (summaries imports this module: not at the top)
    m = check_motif_length(motif_length)
    if model_type not in ("snv", "indel"):
        raise ValueError(f"model_type {model_type} not supported!")
    if not 1 <= int(n_class) <= 8:
        raise ValueError("the motif tables take 1 .. 8 classes")
    lib = _lib.lib()
    fasta_names = {r.name for r in scan_fasta(ref_genome)}
    genomes = {}
    with TableReader(pred_file, n_class, chunk_bytes) as rd:
        dev = rd.device
        table = torch.zeros(4 ** m * 3 * n_class, dtype=torch.int64, device=dev)
        first = torch.full((4 ** m,), -1, dtype=torch.int64, device=dev)      # (all ones = the largest unsigned value)
        status = torch.zeros(1, dtype=torch.int32, device=dev)
        for c in rd:
            rows = list(c.run_row[:c.n_runs]) + [int(c.n_rows)]
            for r in range(c.n_runs):
                name = rd.chrom_name(c.run_chrom[r])
                if name not in genomes:
                    if name not in fasta_names:
                        raise ValueError(f"Chromosome {name} not found in {ref_genome} (prediction table line {c.row0 + rows[r] + 2})")
                    genomes[name] = read_fasta(ref_genome, dev, names={name})[name]
                g = genomes[name].as_struct()
                a, b = rows[r], rows[r + 1]
                s = _lib.MuralSummaryMotifRows()
                s.genome = C.pointer(g)
                s.prob, s.prob_f64, s.prob_stride = c.prob + 8 * n_class * a, 1, n_class
                s.start, s.end, s.label, s.label_kind = c.start + 8 * a, c.end + 8 * a, c.mut_type + 4 * a, 1
                s.n, s.n_class, s.n_m, s.indel, s.order_by_row = b - a, n_class, 1, int(model_type == "indel"), 1
                s.m[0], s.table[0], s.first[0] = m, table.data_ptr(), first.data_ptr()
                s.order_base, s.status = c.row0 + a, status.data_ptr()
                _lib.check(lib.mural_summary_motif_rows(C.byref(s), _lib.current_stream_ptr(dev)))
        bits = int(status.item())
        for bit, what in _SUMMARY_STATUS:
            if bits & bit:
                raise ValueError(f"{pred_file}: {what}")
        table, first = table.cpu().numpy().view(np.uint64).reshape(4 ** m, 3, n_class), first.cpu().numpy().view(np.uint64)
    return motif_table_from_sums(table, first, m, n_class)


def run_motif_corr_calc(args, model_type, chunk_bytes=DEFAULT_CHUNK_BYTES):
    """calc_motif_corr.py:191-261 (`evaluate --motif_only`): per motif observed / predicted rates and their Pearson r per class; writes
    {out_prefix}.{m}-motif.mut_rates.tsv and .corr.txt.  As in the reference no strand is read: ``args.strand`` is ignored."""
    assert args.ref_genome is not None, "--ref_genome is required for motif correlation calculation"
    names, table = motif_table(os.fspath(args.pred_file), os.fspath(args.ref_genome), args.motif_length, args.n_class, model_type, chunk_bytes)
    return write_motif_outputs(names, table, args.n_class, args.motif_length, args.out_prefix)


def write_motif_outputs(names, table, n_class, motif_length, out_prefix):
    """The two files of calc_motif_corr.py:256-261 from a motif table (``motif_table``'s pair, or the one a ``predict.SummarySink``
    reduced in flight); the correlation lines keep the reference's label ``{m}-moitf``.  Returns [(class, (r, p))]."""
    return _write_type_outputs(names, table, n_class, motif_output_names(out_prefix, motif_length), f"{motif_length}-moitf")


# ------------------------------------------------------------------------------------------------------------------
# annotations: expected and observed mutations per named interval set (the exons of a gene, an enhancer set)
# ------------------------------------------------------------------------------------------------------------------
def annotation_output_names(out_prefix):
    return f"{out_prefix}.annotation.mut_rates.tsv", f"{out_prefix}.annotation.corr.txt"


def _annotation_rows(source):
    """(chrom, start, end, name or None, where) of a BED file (plain or gzip; the lines ``read_regions`` skips are skipped) or of a dict
    {chrom: [(start, end[, name])]}."""
    if isinstance(source, dict):
        for chrom, items in source.items():
            for j, item in enumerate(items):
                yield str(chrom), int(item[0]), int(item[1]), (str(item[2]) if len(item) > 2 else None), f"annotations[{chrom!r}][{j}]"
        return
    path = os.fspath(source)
    opener = gzip.open if _is_gzip(path) else open
    with opener(path, "rt") as fh:
        for ln, line in enumerate(fh, 1):
            if not line.strip() or line.startswith(("#", "track", "browser")):
                continue
            f = line.rstrip("\r\n").split("\t")
            if len(f) < 3:
                raise ValueError(f"{path}:{ln}: a BED row needs chrom, start and end")
            yield f[0], int(f[1]), int(f[2]), (f[3] if len(f) > 3 and f[3] else None), f"{path}:{ln}"


def read_annotations(source):
    """(names, meta, pieces) of an annotation BED (a path, plain or gzip; a dict {chrom: [(start, end[, name])]}; or this function's own
    result, returned as it is).  Columns 1-3 are required, column 4 is the NAME of the row's interval set (``chrom:start-end`` where
    there is none); rows may be unsorted, overlap and nest, many rows may share a name (the exons of a gene), and a name may occur on
    several chromosomes.  ``start < 0`` or ``end <= start`` raises ValueError with file and line.
      names: in order of first appearance;
      meta[name] = (n_intervals, length): the input rows of the name, and the bases of the union of its intervals summed over chromosomes;
      pieces[chrom] = (b0 int64, b1 int64, group int32), sorted by (b0, b1, group): each name's intervals on that chromosome merged into
        disjoint pieces that do not touch, `group` the name's index in `names`; pieces of different names overlap freely.
    A prediction row belongs to a piece when b0 <= row.start < b1 (BED half-open on the row's own position): at most once per name, and
    once for every name that covers it.  The list is small: host work."""
    if isinstance(source, tuple) and len(source) == 3 and isinstance(source[2], dict):
        return source
    index, counts, per_chrom = {}, [], {}
    for chrom, a, b, name, where in _annotation_rows(source):
        if a < 0:
            raise ValueError(f"{where}: a negative start ({a})")
        if b <= a:
            raise ValueError(f"{where}: end {b} is not above start {a}")
        name = f"{chrom}:{a}-{b}" if name is None else name
        g = index.setdefault(name, len(index))
        if g == len(counts):
            counts.append(0)
        counts[g] += 1
        per_chrom.setdefault(chrom, []).append((g, a, b))
    names = list(index)
    length = [0] * len(names)
    pieces = {}
    for chrom, rows in per_chrom.items():
        rows.sort()
        merged = []
        for g, a, b in rows:
            if merged and merged[-1][2] == g and a <= merged[-1][1]:      # overlaps or touches the name's piece before it
                merged[-1][1] = max(merged[-1][1], b)
            else:
                merged.append([a, b, g])
        merged.sort()
        arr = np.asarray(merged, np.int64).reshape(-1, 3)
        for a, b, g in merged:
            length[g] += b - a
        pieces[chrom] = (arr[:, 0].copy(), arr[:, 1].copy(), arr[:, 2].astype(np.int32))
    return names, {nm: (counts[g], length[g]) for g, nm in enumerate(names)}, pieces


def annotation_meta(names, meta):
    """int64 [n][2] of (n_intervals, length) in `names` order."""
    return np.asarray([meta[nm] for nm in names], np.int64).reshape(-1, 2)


def annotation_table(pred_file, annotations, n_class, chunk_bytes=DEFAULT_CHUNK_BYTES):
    """(names, meta int64 [n][2], table float64 [n][1 + 2 n_class] of rows / per-class counts / per-class probability sums) per name of
    `annotations` (a BED path or ``read_annotations``' result) from a written prediction table: what ``SummarySink(annotations=...)``
    reduces in flight, through the same entry point (``mural_summary_annot_rows``), chromosome run by chromosome run of each chunk.
    The rows of a chromosome must ascend in start, as ``predict`` writes them; no genome is read."""
    from .summaries import _SUMMARY_STATUS, annot_table_from_sums      # (summaries imports this module: not at the top)
    names, meta, pieces = read_annotations(annotations)
    if not 1 <= int(n_class) <= 8:
        raise ValueError("the annotation tables take 1 .. 8 classes")
    lib = _lib.lib()
    n_groups = len(names)
    with TableReader(pred_file, n_class, chunk_bytes) as rd:
        dev = rd.device
        table = torch.zeros(max(n_groups, 1) * 3 * n_class, dtype=torch.int64, device=dev)
        status = torch.zeros(1, dtype=torch.int32, device=dev)
        on_dev, ws = {}, None
        for c in rd:
            rows = list(c.run_row[:c.n_runs]) + [int(c.n_rows)]
            for r in range(c.n_runs):
                name = rd.chrom_name(c.run_chrom[r])
                a, b = rows[r], rows[r + 1]
                if name not in pieces or b == a:
                    continue
                if name not in on_dev:
                    on_dev[name] = tuple(torch.from_numpy(np.ascontiguousarray(x)).to(dev) for x in pieces[name])
                b0, b1, grp = on_dev[name]
                need = int(lib.mural_summary_annot_workspace_bytes(b - a, n_class))
                if ws is None or ws.numel() * 8 < need:
                    ws = torch.empty(need // 8 + 1, dtype=torch.int64, device=dev)
                s = _lib.MuralSummaryAnnotRows()
                s.prob, s.prob_f64, s.prob_stride = c.prob + 8 * n_class * a, 1, n_class
                s.start, s.label, s.label_kind = c.start + 8 * a, c.mut_type + 4 * a, 1
                s.n, s.n_class, s.n_groups = b - a, n_class, n_groups
                s.piece_b0, s.piece_b1, s.piece_group, s.n_pieces = b0.data_ptr(), b1.data_ptr(), grp.data_ptr(), b0.shape[0]
                s.table, s.status = table.data_ptr(), status.data_ptr()
                _lib.check(lib.mural_summary_annot_rows(C.byref(s), ws.data_ptr(), ws.numel() * 8, _lib.current_stream_ptr(dev)))
        bits = int(status.item())
        for bit, what in _SUMMARY_STATUS:
            if bits & bit:
                raise ValueError(f"{pred_file}: {what}")
        sums = table.cpu().numpy().view(np.uint64)[:n_groups * 3 * n_class].reshape(n_groups, 3, n_class)
    return names, annotation_meta(names, meta), annot_table_from_sums(sums, n_class)


def write_annotation_outputs(names, meta, table, n_class, out_prefix):
    """The two files of an annotation summary (``annotation_table``'s triple, or the one a ``SummarySink`` reduced in flight):
    ``{out_prefix}.annotation.mut_rates.tsv`` -- name, n_intervals, length, number_of_all, the observed number_of_mut{c} and the
    expected_mut{c} (the probability sums) per class c >= 1, a row per name in `names` order -- and ``.annotation.corr.txt``, the Pearson
    r of observed against expected over the names with a row.  Returns [(class, (r, p))]."""
    cls = range(1, n_class)
    table = np.asarray(table, np.float64).reshape(len(names), 1 + 2 * n_class)
    header = (["name", "n_intervals", "length", "number_of_all"] + [f"number_of_mut{c}" for c in cls] + [f"expected_mut{c}" for c in cls])
    rows = [[nm, str(int(meta[j][0])), str(int(meta[j][1])), str(int(table[j, 0]))] + [str(int(table[j, 1 + c])) for c in cls]
            + [_float_text(table[j, 1 + n_class + c]) for c in cls] for j, nm in enumerate(names)]
    used = table[:, 0] > 0
    corrs = []
    for c in cls:
        obs, exp = table[used, 1 + c], table[used, 1 + n_class + c]
        if len(obs) < 2 or np.ptp(obs) == 0 or np.ptp(exp) == 0:      # (no labels: every observed column is zero)
            corrs.append((c, (float("nan"), float("nan"))))
        else:
            corrs.append((c, pearson(obs, exp)))
    rates_path, corr_path = annotation_output_names(out_prefix)
    with open(rates_path, "w") as fh:
        fh.write(_rates_text(header, rows))
    with open(corr_path, "w") as fh:
        fh.write(_corr_text("annotation", corrs))
    return corrs


def run_annotation_calc(args, chunk_bytes=DEFAULT_CHUNK_BYTES):
    """For an `evaluate`-style caller (args.pred_file, args.annotations, args.n_class, args.out_prefix): per name of the annotation BED
    the observed and expected mutations of the table's rows inside its intervals; writes {out_prefix}.annotation.mut_rates.tsv and
    .corr.txt."""
    assert getattr(args, "annotations", None) is not None, "--annotations is required for the annotation table"
    names, meta, table = annotation_table(os.fspath(args.pred_file), args.annotations, args.n_class, chunk_bytes)
    return write_annotation_outputs(names, meta, table, args.n_class, args.out_prefix)


# ------------------------------------------------------------------------------------------------------------------
# consequences: expected and observed mutations per transcript, split by what a substitution does to its codon
# ------------------------------------------------------------------------------------------------------------------
STANDARD_CODON_TABLE = "KNKNTTTTRSRSIIMIQHQHPPPPRRRRLLLLEDEDAAAAGGGGVVVV*Y*YSSSS*CWCLFLF"      # index 16 b0 + 4 b1 + b2, A0 C1 G2 T3
CONSEQUENCES = ("syn", "mis", "stop_gained", "stop_lost")      # bins 0 .. 3 of the consequence table; bin 4 is `unresolved`
_SEG_FIELDS = ("seg_b0", "seg_b1", "seg_cds0", "seg_tx", "seg_prev", "seg_next")


def consequence_output_name(out_prefix):
    return f"{out_prefix}.consequence.mut_rates.tsv"


def check_codon_table(codon_table=None):
    """uint8 [64] of a codon table: 64 characters indexed by 16 b0 + 4 b1 + b2 (A0 C1 G2 T3), '*' a stop; None: the standard code."""
    if codon_table is None:
        codon_table = STANDARD_CODON_TABLE
    if isinstance(codon_table, np.ndarray):
        codon_table = bytes(np.asarray(codon_table, np.uint8)).decode("latin-1")
    text = codon_table.decode("ascii") if isinstance(codon_table, bytes) else str(codon_table)
    if len(text) != 64 or not text.isascii() or any(ch.isspace() for ch in text):
        raise ValueError("codon_table: 64 ASCII characters are required, indexed by 16 b0 + 4 b1 + b2 with A0 C1 G2 T3 ('*' marks a stop)")
    return np.frombuffer(text.encode("ascii"), np.uint8).copy()


def check_alt_order(alt_order=None):
    """uint8 [4][3]: the alternative base of class c = 1 .. 3 of a row whose own base is r (A0 C1 G2 T3), on the row's strand.  None:
    the three other bases in A < C < G < T order (A>C, A>G, A>T; ...).  A text spec names the 12 alternatives row by row
    ("CGT,AGT,ACT,ACG" is the default; commas and blanks are optional).  A row that names r itself or repeats a base is refused."""
    if alt_order is None:
        out = np.array([[b for b in range(4) if b != r] for r in range(4)], np.uint8)
    elif isinstance(alt_order, str):
        text = "".join(ch for ch in alt_order.upper() if ch not in ", ;/")
        if len(text) != 12 or set(text) - set("ACGT"):
            raise ValueError(f"alt_order: 12 letters of ACGT are required, three per own base A, C, G, T (got {alt_order!r})")
        out = np.array(["ACGT".index(ch) for ch in text], np.uint8).reshape(4, 3)
    else:
        out = np.asarray(alt_order)
        if out.shape != (4, 3) or not np.issubdtype(out.dtype, np.integer) or (out < 0).any() or (out > 3).any():
            raise ValueError("alt_order: an integer array [4][3] of base codes 0 .. 3 is required")
        out = out.astype(np.uint8)
    for r in range(4):
        if sorted(out[r].tolist() + [r]) != [0, 1, 2, 3]:
            raise ValueError(f"alt_order: the row of own base {'ACGT'[r]} must name the three other bases once each")
    return out


def _bed12_lines(source):
    """(text line, where) of a BED12 source: a path (plain or gzip) or an open handle (text or bytes)."""
    if hasattr(source, "read"):
        name = getattr(source, "name", "<transcripts>")
        for ln, line in enumerate(source, 1):
            yield (line.decode() if isinstance(line, bytes) else line), f"{name}:{ln}"
        return
    path = os.fspath(source)
    opener = gzip.open if _is_gzip(path) else open
    with opener(path, "rt") as fh:
        for ln, line in enumerate(fh, 1):
            yield line, f"{path}:{ln}"


def read_transcripts(source, codon_table=None):
    """(names, meta, segments) of a BED12 transcript file (a path, plain or gzip; an open handle; or this function's own result, returned
    as it is): chrom start end name score strand thickStart thickEnd rgb blockCount blockSizes blockStarts, trailing commas tolerated; the
    lines ``read_regions`` skips are skipped.  A transcript's CDS segments are its blocks clipped to [thickStart, thickEnd), empty ones
    dropped; a transcript without CDS (thickStart == thickEnd) stays, with zeros.  BED12 carries no frame: CDS offset 0 is the 5'-most
    CDS base in transcript orientation (for strand '-' the last base of the last segment), and the trailing cds_length % 3 bases at the
    3' end belong to no complete codon.  ValueError with file and line: a duplicate name, a strand other than + / -, blocks that overlap
    or do not ascend, blocks that leave [start, end).
      names: in file order;
      meta: dict(chrom [n] list, strand uint8 [n] (1: '-'), cds_length int64 [n], n_segments int32 [n], aa uint8 [64] -- `codon_table`,
        ``check_codon_table``);
      segments[chrom]: dict of flat arrays sorted by (seg_b0, seg_b1, seg_tx): seg_b0, seg_b1 int64 (genomic, half-open), seg_cds0 int64
        (the CDS offset of the segment's first base in transcript orientation), seg_tx int32 (the transcript's index in `names`),
        seg_prev / seg_next int32 (the indices, in the same arrays, of the same transcript's neighbouring segments in transcript
        orientation, -1 at the ends), and tx_strand uint8 / tx_cds_len int64 (meta's arrays: indexed by the global transcript id).
    Transcripts overlap and nest freely, across strands too.  GTF / GFF input and explicit frames are out of scope."""
    if isinstance(source, tuple) and len(source) == 3 and isinstance(source[1], dict) and "aa" in source[1]:
        if codon_table is not None:
            source = (source[0], dict(source[1], aa=check_codon_table(codon_table)), source[2])
        return source
    return _parse_transcripts(source, codon_table)[:3]


def _parse_transcripts(source, codon_table=None):
    """``read_transcripts``' result from a path or a handle, and a fourth item for ``read_transcript_structure``: per transcript
    (chromStart, chromEnd, thickStart, thickEnd, [(block start, block end)])."""
    aa = check_codon_table(codon_table)
    names, index, chroms, strands, cds_len, n_segs, per_chrom, spans = [], set(), [], [], [], [], {}, []
    for line, where in _bed12_lines(source):
        if not line.strip() or line.startswith(("#", "track", "browser")):
            continue
        f = line.rstrip("\r\n").split("\t")
        if len(f) < 12:
            raise ValueError(f"{where}: a BED12 row needs 12 columns (got {len(f)})")
        try:
            start, end, thick0, thick1, n_blocks = int(f[1]), int(f[2]), int(f[6]), int(f[7]), int(f[9])
            sizes = [int(v) for v in f[10].rstrip(",").split(",")] if f[10].strip(",") else []
            offs = [int(v) for v in f[11].rstrip(",").split(",")] if f[11].strip(",") else []
        except ValueError:
            raise ValueError(f"{where}: a BED12 column that should be a number is not") from None
        name = f[3]
        if name in index:
            raise ValueError(f"{where}: duplicate transcript name {name!r}")
        if f[5] not in ("+", "-"):
            raise ValueError(f"{where}: strand {f[5]!r} is neither + nor -")
        if start < 0 or end < start:
            raise ValueError(f"{where}: start {start} / end {end} out of order")
        if len(sizes) != n_blocks or len(offs) != n_blocks:
            raise ValueError(f"{where}: blockCount {n_blocks} against {len(sizes)} blockSizes and {len(offs)} blockStarts")
        if not (thick0 == thick1 or (start <= thick0 < thick1 <= end)):
            raise ValueError(f"{where}: thickStart {thick0} / thickEnd {thick1} outside [{start}, {end})")
        at, segs, blocks = start, [], []
        for size, off in zip(sizes, offs):
            a, b = start + off, start + off + size
            if size <= 0 or a < start or b > end:
                raise ValueError(f"{where}: block [{a}, {b}) leaves [{start}, {end})")
            if a < at:
                raise ValueError(f"{where}: blocks overlap or do not ascend at [{a}, {b})")
            at = b
            blocks.append((a, b))
            a, b = max(a, thick0), min(b, thick1)
            if a < b:
                segs.append((a, b))
        t = len(names)
        index.add(name)
        names.append(name)
        minus = f[5] == "-"
        total = sum(b - a for a, b in segs)
        chroms.append(f[0])
        strands.append(int(minus))
        cds_len.append(total)
        n_segs.append(len(segs))
        spans.append((start, end, thick0, thick1, blocks))
        done = 0                          # CDS bases 5' of the segment, in transcript orientation
        for j, (a, b) in (reversed(list(enumerate(segs))) if minus else enumerate(segs)):
            per_chrom.setdefault(f[0], []).append((a, b, t, done, j))
            done += b - a
    if len(names) >= 2 ** 31:
        raise ValueError("transcripts: 2^31 names or more")
    meta = dict(chrom=chroms, strand=np.asarray(strands, np.uint8), cds_length=np.asarray(cds_len, np.int64),
                n_segments=np.asarray(n_segs, np.int32), aa=aa)
    segments = {}
    for chrom, rows in per_chrom.items():
        rows.sort()
        arr = np.asarray(rows, np.int64).reshape(-1, 5)
        tx, rank = arr[:, 2], arr[:, 4]
        where = {(int(t), int(j)): i for i, (t, j) in enumerate(zip(tx, rank))}
        lower = np.array([where.get((int(t), int(j) - 1), -1) for t, j in zip(tx, rank)], np.int32)      # the neighbour at lower coordinates
        upper = np.array([where.get((int(t), int(j) + 1), -1) for t, j in zip(tx, rank)], np.int32)
        minus = meta["strand"][tx] != 0
        segments[chrom] = dict(seg_b0=arr[:, 0].copy(), seg_b1=arr[:, 1].copy(), seg_cds0=arr[:, 3].copy(), seg_tx=tx.astype(np.int32),
                               seg_prev=np.where(minus, upper, lower).astype(np.int32), seg_next=np.where(minus, lower, upper).astype(np.int32),
                               tx_strand=meta["strand"], tx_cds_len=meta["cds_length"])
    return names, meta, segments, spans


def read_transcript_structure(source, codon_table=None):
    """(names, meta, segments, features) of a BED12 transcript file: ``read_transcripts``' three (the same line parser and refusals) and
    the transcripts' STRUCTURE for ``summary_txstruct_host`` / ``mural_summary_txstruct_rows``.  `source`: a path (plain or gzip), an
    open handle, or this function's own result, returned as it is; a ``read_transcripts`` triple holds no blocks any more and is refused.
      features[chrom]: dict of flat arrays sorted by (feat_b0, feat_b1, feat_tx): feat_b0, feat_b1 int64 (genomic, half-open), feat_tx
        int32, feat_kind uint8, feat_seg int32 (kind 5: the index in segments[chrom] of the CDS segment that equals the item; else -1),
        and tx_strand / tx_cds_len as `segments` has them.
    A transcript's items TILE [chromStart, chromEnd) without overlap: its blocks, cut at thickStart / thickEnd, and the gaps between
    them (an empty gap between abutting blocks is dropped; where the blocks do not reach an end of the span, the rest is a gap too).
    Kinds: 0 a 5'UTR exon part, 1 a 3'UTR exon part -- in transcript orientation: on '-' the part at or above thickEnd is the 5'UTR --, 2
    an exon of a transcript without CDS (thickStart == thickEnd), 3 a coding intron -- a gap [a, b) with thickStart < a and b <
    thickEnd: a CDS base on both sides --, 4 any other gap, 5 a CDS part."""
    if isinstance(source, tuple) and len(source) == 4 and isinstance(source[1], dict) and "aa" in source[1]:
        return source
    if isinstance(source, tuple):
        raise ValueError("read_transcript_structure: a read_transcripts result holds no UTR exons and introns; pass the BED12 path")
    names, meta, segments, spans = _parse_transcripts(source, codon_table)
    per_chrom = {}
    for t, (start, end, thick0, thick1, blocks) in enumerate(spans):
        items, minus, at = per_chrom.setdefault(meta["chrom"][t], []), bool(meta["strand"][t]), start
        for a, b in blocks + [(end, end)]:
            if at < a:
                items.append((at, a, t, 3 if thick0 < at and a < thick1 else 4))
            at = b
            if thick0 == thick1:
                cuts = [(a, b, 2)]
            else:
                cuts = [(a, min(b, thick0), 1 if minus else 0), (max(a, thick0), min(b, thick1), 5), (max(a, thick1), b, 0 if minus else 1)]
            items += [(lo, hi, t, kind) for lo, hi, kind in cuts if lo < hi]
    features = {}
    for chrom, items in per_chrom.items():
        if not items:
            continue
        items.sort()
        arr = np.asarray(items, np.int64).reshape(-1, 4)
        seg = segments.get(chrom)
        where = {} if seg is None else {key: j for j, key in enumerate(zip(seg["seg_b0"].tolist(), seg["seg_b1"].tolist(), seg["seg_tx"].tolist()))}
        feat_seg = np.array([where[(a, b, t)] if kind == 5 else -1 for a, b, t, kind in arr.tolist()], np.int32)
        features[chrom] = dict(feat_b0=arr[:, 0].copy(), feat_b1=arr[:, 1].copy(), feat_tx=arr[:, 2].astype(np.int32),
                               feat_kind=arr[:, 3].astype(np.uint8), feat_seg=feat_seg, tx_strand=meta["strand"], tx_cds_len=meta["cds_length"])
    return names, meta, segments, features


def consequence_table_from_sums(table, rows):
    """float64 [n][3 + 2 * 4 + 1] per transcript from the integer sums of ``summary_conseq_host`` / ``mural_summary_conseq_rows``: n_rows,
    n_nonmut, n_unresolved (the mutated rows of bin 4), then expected, observed per consequence of ``CONSEQUENCES`` and the expected
    value of bin 4.  A probability sum is (hi * 2^40 + lo) / 2^71, formed from Python integers (true division rounds correctly)."""
    table, rows = np.asarray(table, np.uint64).reshape(-1, 5, 3), np.asarray(rows, np.uint64).reshape(-1, 2)
    out = np.zeros((table.shape[0], 12))
    out[:, 0], out[:, 1], out[:, 2] = rows[:, 0], rows[:, 1], table[:, 4, 0]
    den = 1 << 71
    hi, lo = table[:, :, 1].ravel().tolist(), table[:, :, 2].ravel().tolist()
    exp = np.array([((h << 40) + l) / den for h, l in zip(hi, lo)], np.float64).reshape(-1, 5)
    out[:, 3:11:2], out[:, 4:11:2], out[:, 11] = exp[:, :4], table[:, :4, 0], exp[:, 4]
    return out


def write_consequence_outputs(names, meta, table, out_prefix, labels=True):
    """``{out_prefix}.consequence.mut_rates.tsv`` from a consequence table (``consequence_table``'s triple, or the one a ``SummarySink``
    reduced in flight): a line per transcript in file order -- name, chrom, strand, cds_length, n_rows (the rows inside the CDS), n_nonmut
    (those of label 0), n_unresolved (the mutated rows in incomplete or masked codons), then expected_* and observed_* for syn, mis,
    stop_gained and stop_lost.  `labels=False`: the rows carried no labels, the observed_* columns are NA.  Returns the path."""
    table = np.asarray(table, np.float64).reshape(len(names), 12)
    header = ["name", "chrom", "strand", "cds_length", "n_rows", "n_nonmut", "n_unresolved"]
    for what in CONSEQUENCES:
        header += [f"expected_{what}", f"observed_{what}"]
    rows = []
    for j, nm in enumerate(names):
        row = [nm, meta["chrom"][j], "-" if meta["strand"][j] else "+", str(int(meta["cds_length"][j]))] + [str(int(v)) for v in table[j, :3]]
        for b in range(4):
            row += [_float_text(table[j, 3 + 2 * b]), str(int(table[j, 4 + 2 * b])) if labels else "NA"]
        rows.append(row)
    path = consequence_output_name(out_prefix)
    with open(path, "w") as fh:
        fh.write(_rates_text(header, rows))
    return path


def consequence_table(pred_file, transcripts, ref_genome, codon_table=None, alt_order=None, chunk_bytes=DEFAULT_CHUNK_BYTES):
    """(names, meta, table float64 [n][12] -- ``consequence_table_from_sums``) per transcript of `transcripts` (a BED12 path or
    ``read_transcripts``' result) from a written SNV prediction table (4 classes): what ``SummarySink(transcripts=...)`` reduces in
    flight, through the same entry point (``mural_summary_conseq_rows``), chromosome run by chromosome run of each chunk.  The rows of a
    chromosome must ascend in start, as ``predict`` writes them; the codons are read from `ref_genome` (a FASTA path)."""
    from .data.ingest import read_fasta, scan_fasta
    from .summaries import _SUMMARY_STATUS, conseq_rows_device      # (summaries imports this module: not at the top)
    names, meta, segments = read_transcripts(transcripts, codon_table)
    alt = check_alt_order(alt_order)
    n_tx = len(names)
    fasta_names = {r.name for r in scan_fasta(ref_genome)}
    with TableReader(pred_file, 4, chunk_bytes) as rd:
        dev = rd.device
        acc = dict(table=torch.zeros(max(n_tx, 1) * 15, dtype=torch.int64, device=dev), rows=torch.zeros(max(n_tx, 1) * 2, dtype=torch.int64, device=dev),
                   status=torch.zeros(1, dtype=torch.int32, device=dev), segments={}, ws=None)
        genomes = {}
        for c in rd:
            rows = list(c.run_row[:c.n_runs]) + [int(c.n_rows)]
            for r in range(c.n_runs):
                name = rd.chrom_name(c.run_chrom[r])
                a, b = rows[r], rows[r + 1]
                if name not in segments or b == a:
                    continue
                if name not in genomes:
                    if name not in fasta_names:
                        raise ValueError(f"Chromosome {name} not found in {ref_genome} (prediction table line {c.row0 + a + 2})")
                    genomes[name] = read_fasta(ref_genome, dev, names={name})[name]
                conseq_rows_device(acc, name, segments[name], n_tx, meta["aa"], alt, genomes[name].as_struct(), dev,
                                   prob=c.prob + 8 * 4 * a, prob_f64=1, prob_stride=4, start=c.start + 8 * a, strand=c.strand + a,
                                   label=c.mut_type + 4 * a, label_kind=1, n=b - a)
        bits = int(acc["status"].item())
        for bit, what in _SUMMARY_STATUS:
            if bits & bit:
                raise ValueError(f"{pred_file}: {what}")
        table = acc["table"].cpu().numpy().view(np.uint64)[:n_tx * 15].reshape(n_tx, 5, 3)
        counts = acc["rows"].cpu().numpy().view(np.uint64)[:n_tx * 2].reshape(n_tx, 2)
    return names, meta, consequence_table_from_sums(table, counts)


def run_consequence_calc(args, chunk_bytes=DEFAULT_CHUNK_BYTES):
    """For an `evaluate`-style caller (args.pred_file, args.transcripts, args.ref_genome, args.out_prefix; optional args.codon_table,
    args.alt_order): per transcript of the BED12 file the expected and observed mutations of the table's rows inside its CDS by
    consequence; writes {out_prefix}.consequence.mut_rates.tsv."""
    assert getattr(args, "transcripts", None) is not None, "--transcripts is required for the consequence table"
    assert getattr(args, "ref_genome", None) is not None, "--ref_genome is required for the consequence table"
    names, meta, table = consequence_table(os.fspath(args.pred_file), args.transcripts, os.fspath(args.ref_genome),
                                           getattr(args, "codon_table", None), getattr(args, "alt_order", None), chunk_bytes)
    return write_consequence_outputs(names, meta, table, args.out_prefix)


# the structure table: where a row lies in the transcript, beside the consequence table (``summaries.summary_txstruct_host`` is the rule)
STRUCTURE_BINS = ("utr5", "utr3", "noncoding_exon", "splice_donor", "splice_acceptor", "splice_utr", "intron", "start_lost", "cds")


def structure_output_name(out_prefix):
    return f"{out_prefix}.consequence.structure.tsv"


def _structure_acc(n_tx, dev):
    """The device accumulators of ``summaries.txstruct_rows_device`` and, in `conseq`, of ``summaries.conseq_rows_device``."""
    zeros = lambda n, dt=torch.int64: torch.zeros(n, dtype=dt, device=dev)      # noqa: E731
    return dict(table=zeros(max(n_tx, 1) * 27), rows=zeros(max(n_tx, 1) * 2), status=zeros(1, torch.int32), features={}, ws=None,
                conseq=dict(table=zeros(max(n_tx, 1) * 15), rows=zeros(max(n_tx, 1) * 2), status=zeros(1, torch.int32), segments={}, ws=None))


def _structure_cells(cells, stop_gained):
    """The ten [count, hi, lo] cells of a transcript as Python integers: its nine bins and LoF = stop gained + splice donor + splice
    acceptor + start lost, added word by word."""
    return cells + [[sum(c[w] for c in (stop_gained, cells[3], cells[4], cells[7])) for w in range(3)]]


def structure_cells_from_sums(table, stop_gained):
    """(expected float64 [n][10], observed int64 [n][10]) of the nine bins of ``STRUCTURE_BINS`` and LoF from the integer sums
    ``write_structure_outputs`` takes: the numbers of its expected_* and observed_* columns.  Where every limb is below 2^51 -- any
    real run -- the LoF words are added as uint64 without overflow, hi and lo are exact in float64 and hi * 2^40 + lo is ONE float64
    addition of two exact terms: rounded correctly, as the writer's true division of Python integers is, and the scaling by 2^-71 is
    exact; the same numbers without a walk over the cells.  Otherwise the writer's own arithmetic, cell by cell."""
    table = np.asarray(table, np.uint64).reshape(-1, 9, 3)
    stop_gained = np.asarray(stop_gained, np.uint64).reshape(len(table), 3)
    limit = np.uint64(1 << 51)
    if (table < limit).all() and (stop_gained < limit).all():
        full = np.concatenate([table, (stop_gained + table[:, 3] + table[:, 4] + table[:, 7])[:, None, :]], axis=1)
        expected = (full[:, :, 1].astype(np.float64) * 2.0 ** 40 + full[:, :, 2].astype(np.float64)) * 2.0 ** -71
        return expected, full[:, :, 0].astype(np.int64)
    den = 1 << 71
    cells = [_structure_cells(c, s) for c, s in zip(table.tolist(), stop_gained.tolist())]
    expected = np.array([[((hi << 40) + lo) / den for _, hi, lo in c] for c in cells], np.float64).reshape(len(table), 10)
    observed = np.array([[count for count, _, _ in c] for c in cells], np.int64).reshape(len(table), 10)
    return expected, observed


def write_structure_outputs(names, meta, table, rows, stop_gained, out_prefix, labels=True):
    """``{out_prefix}.consequence.structure.tsv`` from the integer sums of ``summary_txstruct_host`` / ``mural_summary_txstruct_rows``
    (table uint64 [n][9][3], rows uint64 [n][2]) and `stop_gained` uint64 [n][3], bin 2 of the consequence table's own integers: a line
    per transcript in file order -- name, chrom, strand, n_rows (the rows inside the span), n_nonmut (those of label 0), expected_* and
    observed_* for the nine bins of ``STRUCTURE_BINS``, and expected_lof / observed_lof = stop gained + splice donor + splice acceptor +
    start lost.  An expected value is (hi * 2^40 + lo) / 2^71, formed from Python integers by true division (the LoF sum is added as
    integers first).  `labels=False`: the rows carried no labels, the observed_* columns are NA.  Returns the path."""
    table = np.asarray(table, np.uint64).reshape(len(names), 9, 3).tolist()
    rows = np.asarray(rows, np.uint64).reshape(len(names), 2).tolist()
    stop_gained = np.asarray(stop_gained, np.uint64).reshape(len(names), 3).tolist()
    header = ["name", "chrom", "strand", "n_rows", "n_nonmut"]
    for what in STRUCTURE_BINS + ("lof",):
        header += [f"expected_{what}", f"observed_{what}"]
    den, lines = 1 << 71, []
    for j, nm in enumerate(names):
        cells = _structure_cells(table[j], stop_gained[j])
        line =[nm, meta["chrom"][j], "-" if meta["strand"][j] else "+", str(rows[j][0]), str(rows[j][1])]
        for count, hi, lo in cells:
            line += [_float_text(((hi << 40) + lo) / den), str(count) if labels else "NA"]
        lines.append(line)
    path = structure_output_name(out_prefix)
    with open(path, "w") as fh:
        fh.write(_rates_text(header, lines))
    return path


def structure_table(pred_file, transcripts, ref_genome, codon_table=None, alt_order=None, chunk_bytes=DEFAULT_CHUNK_BYTES):
    """(names, meta, table uint64 [n][9][3], rows uint64 [n][2], stop_gained uint64 [n][3]) per transcript of `transcripts` (a BED12
    path or ``read_transcript_structure``'s result) from a written SNV prediction table (4 classes): what ``SummarySink(transcripts=...,
    transcript_structure=True)`` reduces in flight, through the same entry points (``mural_summary_txstruct_rows``, and
    ``mural_summary_conseq_rows`` for the stop-gained integers of the LoF column), chromosome run by chromosome run of each chunk.  The
    rows of a chromosome must ascend in start, as ``predict`` writes them; the codons are read from `ref_genome` (a FASTA path)."""
    from .data.ingest import read_fasta, scan_fasta
    from .summaries import _SUMMARY_STATUS, conseq_rows_device, txstruct_rows_device      # (summaries imports this module: not at the top)
    names, meta, segments, features = read_transcript_structure(transcripts, codon_table)
    alt = check_alt_order(alt_order)
    n_tx = len(names)
    fasta_names = {r.name for r in scan_fasta(ref_genome)}
    with TableReader(pred_file, 4, chunk_bytes) as rd:
        dev = rd.device
        acc = _structure_acc(n_tx, dev)
        genomes = {}
        for c in rd:
            rows = list(c.run_row[:c.n_runs]) + [int(c.n_rows)]
            for r in range(c.n_runs):
                name = rd.chrom_name(c.run_chrom[r])
                a, b = rows[r], rows[r + 1]
                if name not in features or b == a:
                    continue
                if name not in genomes:
                    if name not in fasta_names:
                        raise ValueError(f"Chromosome {name} not found in {ref_genome} (prediction table line {c.row0 + a + 2})")
                    genomes[name] = read_fasta(ref_genome, dev, names={name})[name]
                cols = dict(prob=c.prob + 8 * 4 * a, prob_f64=1, prob_stride=4, start=c.start + 8 * a, strand=c.strand + a,
                            label=c.mut_type + 4 * a, label_kind=1, n=b - a)
                if name in segments:
                    conseq_rows_device(acc["conseq"], name, segments[name], n_tx, meta["aa"], alt, genomes[name].as_struct(), dev, **cols)
                txstruct_rows_device(acc, acc["conseq"], name, segments.get(name), features[name], n_tx, meta["aa"], alt,
                                     genomes[name].as_struct(), dev, **cols)
        bits = int(acc["status"].item()) | int(acc["conseq"]["status"].item())
        for bit, what in _SUMMARY_STATUS:
            if bits & bit:
                raise ValueError(f"{pred_file}: {what}")
        table = acc["table"].cpu().numpy().view(np.uint64)[:n_tx * 27].reshape(n_tx, 9, 3)
        counts = acc["rows"].cpu().numpy().view(np.uint64)[:n_tx * 2].reshape(n_tx, 2)
        stop_gained = acc["conseq"]["table"].cpu().numpy().view(np.uint64)[:n_tx * 15].reshape(n_tx, 5, 3)[:, 2].copy()
    return names, meta, table, counts, stop_gained


def run_structure_calc(args, chunk_bytes=DEFAULT_CHUNK_BYTES):
    """For an `evaluate`-style caller (args.pred_file, args.transcripts, args.ref_genome, args.out_prefix; optional args.codon_table,
    args.alt_order): per transcript of the BED12 file the expected and observed mutations of the table's rows inside its span by where
    they lie in its structure; writes {out_prefix}.consequence.structure.tsv."""
    assert getattr(args, "transcripts", None) is not None, "--transcripts is required for the structure table"
    assert getattr(args, "ref_genome", None) is not None, "--ref_genome is required for the structure table"
    result = structure_table(os.fspath(args.pred_file), args.transcripts, os.fspath(args.ref_genome), getattr(args, "codon_table", None),
                             getattr(args, "alt_order", None), chunk_bytes)
    return write_structure_outputs(*result, args.out_prefix)


# the INDEL structure table: what an INDEL event does to the transcript (``summaries.summary_txindel_host`` is the rule)
INDEL_STRUCTURE_BINS = ("utr5", "utr3", "noncoding_exon", "splice", "splice_utr", "intron", "start_lost", "frameshift", "inframe", "cds_mixed")
INDEL_KINDS = ("insertion", "deletion_start", "deletion_end")      # the models the reference ships: `kind` 0, 1, 2
INDEL_DEFAULT_LENGTHS = "1,2,3,4,5,6,7-20"                          # the reference's labelling of its 8 classes
INDEL_MAX_LENGTH = 64


def indel_structure_output_name(out_prefix):
    return f"{out_prefix}.indel_structure.tsv"


def check_indel_kind(kind):
    """0, 1 or 2 from a kind's number or its name in ``INDEL_KINDS``; ValueError otherwise."""
    if isinstance(kind, str) and kind in INDEL_KINDS:
        return INDEL_KINDS.index(kind)
    if isinstance(kind, (int, np.integer)) and not isinstance(kind, bool) and 0 <= int(kind) <= 2:
        return int(kind)
    raise ValueError(f"indel_kind: one of {', '.join(INDEL_KINDS)} (or 0, 1, 2) is required, got {kind!r}")


def check_breakpoint_offset(offset):
    if isinstance(offset, (int, np.integer)) and not isinstance(offset, bool) and int(offset) in (0, 1):
        return int(offset)
    raise ValueError(f"breakpoint_offset: 0 or 1 is required, got {offset!r}")


def check_indel_lengths(lengths=None, n_class=None):
    """int32 [n_class][2]: the inclusive (lo, hi) of the lengths that class c >= 1 stands for, row 0 zeros.  `lengths`: a text spec, one
    entry per class >= 1 ("1,2,3,4-6": a number or lo-hi), a sequence or array of numbers or (lo, hi) pairs, this function's own result
    (an array whose row 0 is (0, 0): no class has lo = 0), or None -- ``INDEL_DEFAULT_LENGTHS``, which serves 8 classes only.  1 <= lo <= hi <= 64, and with `n_class` one entry per class
    >= 1; ValueError otherwise."""
    if lengths is None:
        if n_class is not None and int(n_class) != 8:
            raise ValueError(f"indel_lengths: the default {INDEL_DEFAULT_LENGTHS} serves 8 classes; {n_class} classes need their own")
        lengths = INDEL_DEFAULT_LENGTHS
    if isinstance(lengths, np.ndarray) and lengths.ndim == 2 and lengths.shape[1] == 2 and len(lengths) and not lengths[0].any():
        pairs = [tuple(int(v) for v in row) for row in lengths[1:].tolist()]      # this function's own result: row 0 is (0, 0), no class's
    elif isinstance(lengths, str):
        pairs = []
        for item in lengths.replace(" ", "").strip(",").split(","):
            lo, dash, hi = item.partition("-")
            if not lo.isdigit() or (dash and not hi.isdigit()):
                raise ValueError(f"indel_lengths: {item!r} is neither a length nor lo-hi (got {lengths!r})")
            pairs.append((int(lo), int(hi) if dash else int(lo)))
    else:
        try:
            pairs = [(int(v), int(v)) if np.ndim(v) == 0 else (int(v[0]), int(v[1])) for v in lengths]
        except (TypeError, ValueError, IndexError):
            raise ValueError("indel_lengths: a text spec or a sequence of lengths / (lo, hi) pairs is required") from None
    if not 1 <= len(pairs) <= 15:
        raise ValueError(f"indel_lengths: 1 .. 15 classes above class 0 (got {len(pairs)})")
    if n_class is not None and len(pairs) != int(n_class) - 1:
        raise ValueError(f"indel_lengths: {len(pairs)} entries for {int(n_class) - 1} classes above class 0")
    for c, (lo, hi) in enumerate(pairs, 1):
        if not 1 <= lo <= hi <= INDEL_MAX_LENGTH:
            raise ValueError(f"indel_lengths: class {c} needs 1 <= lo <= hi <= {INDEL_MAX_LENGTH} (got {lo}-{hi})")
    return np.asarray([(0, 0)] + pairs, np.int32)


def structure_links(features):
    """(feat_prev, feat_next) int32 of a chromosome's dict of ``read_transcript_structure``'s features: per item the index, in the same
    arrays, of the same transcript's neighbouring item at lower / higher coordinates (genomic order), -1 at the ends of the span.  A
    transcript's items tile its span, so the neighbour at higher coordinates starts where the item ends."""
    tx, b0 = np.asarray(features["feat_tx"], np.int64), np.asarray(features["feat_b0"], np.int64)
    order = np.lexsort((b0, tx))      # by transcript, then by position
    prev, nxt = np.full(len(tx), -1, np.int32), np.full(len(tx), -1, np.int32)
    if len(order) > 1:
        same = tx[order[1:]] == tx[order[:-1]]
        prev[order[1:][same]] = order[:-1][same]
        nxt[order[:-1][same]] = order[1:][same]
    return prev, nxt


def _indel_lof_cells(cells):
    """The twelve [count, hi, lo] cells of a transcript as Python integers: its ten bins, LoF = splice + start lost + frameshift and the
    upper LoF = that + cds_mixed, added word by word."""
    lof = [cells[3][w] + cells[6][w] + cells[7][w] for w in range(3)]
    return cells + [lof, [lof[w] + cells[9][w] for w in range(3)]]


def indel_structure_cells_from_sums(table):
    """(expected, observed) of the INDEL structure file from the integer sums [n][10][3] (an array or nested lists): per transcript
    twelve Python floats and twelve Python integers -- the ten bins of ``INDEL_STRUCTURE_BINS``, then lof and lof_upper
    (``_indel_lof_cells``).  The integers are added as integers; an expected value is (hi * 2^40 + lo) / 2^71, formed from Python
    integers by true division.  The one place where ``write_indel_structure_outputs`` and
    ``write_indel_structure_simulation_outputs`` take their numbers from."""
    table = table.tolist() if isinstance(table, np.ndarray) else table
    den, expected, observed = 1 << 71, [], []
    for cells in table:
        cells = _indel_lof_cells([[int(w) for w in cell] for cell in cells])
        expected.append([((hi << 40) + lo) / den for _, hi, lo in cells])
        observed.append([count for count, _, _ in cells])
    return expected, observed


def write_indel_structure_outputs(names, meta, table, rows, kind, out_prefix, labels=True):
    """``{out_prefix}.indel_structure.tsv`` from the integer sums of ``summary_txindel_host`` / ``mural_summary_txindel_rows`` (table
    uint64 [n][10][3], rows uint64 [n][2]) of a run of `kind` (``check_indel_kind``): a line per transcript in file order -- name, chrom,
    strand, kind, n_rows (the rows counted), n_nonmut (those of label 0), expected_* and observed_* for the ten bins of
    ``INDEL_STRUCTURE_BINS``, expected_lof / observed_lof = splice + start lost + frameshift and expected_lof_upper / observed_lof_upper =
    that + cds_mixed.  The integers are added as integers; an expected value is (hi * 2^40 + lo) / 2^71, formed from Python integers by
    true division.  `labels=False`: the rows carried no labels, the observed_* columns are NA.  Returns the path."""
    kind = INDEL_KINDS[check_indel_kind(kind)]
    table = np.asarray(table, np.uint64).reshape(len(names), 10, 3).tolist()
    rows = np.asarray(rows, np.uint64).reshape(len(names), 2).tolist()
    header = ["name", "chrom", "strand", "kind", "n_rows", "n_nonmut"]
    for what in INDEL_STRUCTURE_BINS + ("lof", "lof_upper"):
        header += [f"expected_{what}", f"observed_{what}"]
    expected, observed = indel_structure_cells_from_sums(table)
    lines = []
    for j, nm in enumerate(names):
        line = [nm, meta["chrom"][j], "-" if meta["strand"][j] else "+", kind, str(rows[j][0]), str(rows[j][1])]
        for value, count in zip(expected[j], observed[j]):
            line += [_float_text(value), str(count) if labels else "NA"]
        lines.append(line)
    path = indel_structure_output_name(out_prefix)
    with open(path, "w") as fh:
        fh.write(_rates_text(header, lines))
    return path


def _indel_structure_acc(n_tx, dev):
    """The device accumulators of ``summaries.txindel_rows_device``."""
    zeros = lambda n, dt=torch.int64: torch.zeros(n, dtype=dt, device=dev)      # noqa: E731
    return dict(table=zeros(max(n_tx, 1) * 30), rows=zeros(max(n_tx, 1) * 2), status=zeros(1, torch.int32), features={}, segments={}, ws=None)


def indel_structure_table(pred_file, transcripts, n_class, kind, lengths=None, breakpoint_offset=1, chrom_lengths=None,
                          chunk_bytes=DEFAULT_CHUNK_BYTES):
    """(names, meta, table uint64 [n][10][3], rows uint64 [n][2]) per transcript of `transcripts` (a BED12 path or
    ``read_transcript_structure``'s result) from a written INDEL prediction table of `n_class` classes: what
    ``SummarySink(indel_transcripts=...)`` reduces in flight, through the same entry point (``mural_summary_txindel_rows``), chromosome
    run by chromosome run of each chunk.  `kind`, `lengths`, `breakpoint_offset`: ``summary_txindel_host``'s; `chrom_lengths`: {name:
    length} or None -- a deletion is then clipped to the transcript's span alone.  The rows of a chromosome must ascend in start, as
    ``predict`` writes them; no genome is read."""
    from .summaries import _SUMMARY_STATUS, txindel_rows_device      # (summaries imports this module: not at the top)
    names, meta, segments, features = read_transcript_structure(transcripts)
    k, kind, off = int(n_class), check_indel_kind(kind), check_breakpoint_offset(breakpoint_offset)
    class_len = check_indel_lengths(lengths, k)
    n_tx = len(names)
    links = {}
    with TableReader(pred_file, k, chunk_bytes) as rd:
        dev = rd.device
        acc = _indel_structure_acc(n_tx, dev)
        for c in rd:
            rows = list(c.run_row[:c.n_runs]) + [int(c.n_rows)]
            for r in range(c.n_runs):
                name = rd.chrom_name(c.run_chrom[r])
                a, b = rows[r], rows[r + 1]
                if name not in features or b == a:
                    continue
                if name not in links:
                    links[name] = structure_links(features[name])
                txindel_rows_device(acc, name, segments.get(name), features[name], links[name], n_tx, kind, off, class_len,
                                    None if chrom_lengths is None else chrom_lengths.get(name), dev, prob=c.prob + 8 * k * a, prob_f64=1,
                                    prob_stride=k, start=c.start + 8 * a, label=c.mut_type + 4 * a, label_kind=1, n=b - a, n_class=k)
        bits = int(acc["status"].item())
        for bit, what in _SUMMARY_STATUS:
            if bits & bit:
                raise ValueError(f"{pred_file}: {what}")
        table = acc["table"].cpu().numpy().view(np.uint64)[:n_tx * 30].reshape(n_tx, 10, 3)
        counts = acc["rows"].cpu().numpy().view(np.uint64)[:n_tx * 2].reshape(n_tx, 2)
    return names, meta, table, counts


def read_chrom_lengths(source):
    """{name: length} from a dict (returned as it is), or from a FASTA index (.fai) or any tab-separated file of name and length."""
    if isinstance(source, dict):
        return source
    out = {}
    with open(os.fspath(source)) as fh:
        for ln, line in enumerate(fh, 1):
            f = line.rstrip("\r\n").split("\t")
            if not line.strip() or line.startswith("#"):
                continue
            if len(f) < 2 or not f[1].isdigit():
                raise ValueError(f"{source}:{ln}: a chromosome name and its length are required")
            out[f[0]] = int(f[1])
    return out


def run_indel_structure_calc(args, chunk_bytes=DEFAULT_CHUNK_BYTES):
    """For an `evaluate`-style caller (args.pred_file, args.indel_transcripts, args.n_class, args.indel_kind, args.out_prefix; optional
    args.indel_lengths, args.breakpoint_offset, args.chrom_lengths): per transcript of the BED12 file the expected and observed INDEL
    events of the table's rows by what they do to its structure; writes {out_prefix}.indel_structure.tsv.  args.chrom_lengths: {name:
    length}, or a FASTA index (.fai) -- ``read_chrom_lengths``.  ``SummarySink(indel_transcripts=, genome=)`` clips a deletion to the
    chromosome; this route gives the same table for a transcript that runs past the chromosome's end only with the lengths."""
    assert getattr(args, "indel_transcripts", None) is not None, "--indel_transcripts is required for the INDEL structure table"
    assert getattr(args, "indel_kind", None) is not None, "--indel_kind is required for the INDEL structure table"
    lengths = getattr(args, "chrom_lengths", None)
    names, meta, table, rows = indel_structure_table(os.fspath(args.pred_file), args.indel_transcripts, args.n_class, args.indel_kind,
                                                     getattr(args, "indel_lengths", None), getattr(args, "breakpoint_offset", 1),
                                                     None if lengths is None else read_chrom_lengths(lengths), chunk_bytes)
    return write_indel_structure_outputs(names, meta, table, rows, args.indel_kind, args.out_prefix)


# ------------------------------------------------------------------------------------------------------------------
# simulation: mutation sets drawn from the rates, per-name empirical p-values
# ------------------------------------------------------------------------------------------------------------------
def simulation_output_name(out_prefix):
    return f"{out_prefix}.annotation.sim.tsv"


def simulation_bed_name(out_prefix, replicate):
    return f"{out_prefix}.sim{int(replicate)}.mutations.bed"


def simulation_bed_text(chrom, start, strand, label):
    """The rows of a simulated mutation list as BED text: chrom start end name score strand, score = class (``data.read_mutations``)."""
    return "".join(f"{chrom}\t{s}\t{s + 1}\t.\t{c}\t{'-' if m else '+'}\n"
                   for s, m, c in zip(np.asarray(start).tolist(), np.asarray(strand).tolist(), np.asarray(label).tolist()))


def write_simulation_outputs(names, counts, observed, expected, n_class, out_prefix):
    """``{out_prefix}.annotation.sim.tsv``: one line per name and class c >= 1 -- name, class, observed, expected, sim_mean, sim_min,
    sim_max, n_ge, n_le, p_upper, p_lower (``summaries.simulate_pvalues``) -- from counts [names][n_class - 1][R], observed
    [names][n_class - 1] (None: no labels, 'NA' in the observed column and the last four) and expected [names][n_class - 1]."""
    from .summaries import simulate_pvalues      # (summaries imports this module: not at the top)
    header = ["name", "class", "observed", "expected", "sim_mean", "sim_min", "sim_max", "n_ge", "n_le", "p_upper", "p_lower"]
    counts = np.asarray(counts)
    rows = []
    stats = {c: simulate_pvalues(counts[:, c - 1], None if observed is None else np.asarray(observed)[:, c - 1]) for c in range(1, n_class)}
    for j, nm in enumerate(names):
        for c in range(1, n_class):
            mean, lo, hi, n_ge, n_le, p_up, p_lo = stats[c][j]
            obs = "NA" if observed is None else str(int(observed[j][c - 1]))
            tail = ["NA"] * 4 if observed is None else [str(n_ge), str(n_le), _float_text(p_up), _float_text(p_lo)]
            rows.append([nm, str(c), obs, _float_text(expected[j][c - 1]), _float_text(mean), str(lo), str(hi)] + tail)
    path = simulation_output_name(out_prefix)
    with open(path, "w") as fh:
        fh.write(_rates_text(header, rows))
    return path


def simulate_table(pred_file, annotations, n_rep, seed, n_class, write=(), out_prefix=None, labels=True, chunk_bytes=DEFAULT_CHUNK_BYTES):
    """(names, counts uint32 [names][n_class - 1][n_rep], observed or None, expected) from a written prediction table: what
    ``SummarySink(simulate=n_rep, simulate_seed=seed, annotations=...)`` reduces in flight, through the same entries
    (``mural_simulate_annot_rows`` beside ``mural_summary_annot_rows``), chromosome run by chromosome run of each chunk; the draws are
    made from the table's four-digit probabilities.  `write`: replicates whose mutation lists go to
    ``{out_prefix}.sim{r}.mutations.bed`` (``mural_simulate_rows``).  `annotations` may be None when only lists are asked for."""
    from .summaries import _SUMMARY_STATUS, SIMULATE_MAX_REPLICATES, annot_table_from_sums, simulate_chrom_key
    n_class, n_rep, seed, write = int(n_class), int(n_rep), int(seed), tuple(int(r) for r in write)
    if not 2 <= n_class <= 8:
        raise ValueError("the simulation takes 2 .. 8 classes")
    if not 1 <= n_rep <= SIMULATE_MAX_REPLICATES or not 0 <= seed < 1 << 64:
        raise ValueError("simulate_table: 1 .. 2^20 replicates and an unsigned 64-bit seed")
    if any(not 0 <= r < n_rep for r in write) or (write and out_prefix is None):
        raise ValueError("simulate_table: `write` holds replicates below n_rep and needs an out_prefix")
    if annotations is None and not write:
        raise ValueError("simulate_table needs annotations or a replicate to write")
    names, meta, pieces = read_annotations(annotations) if annotations is not None else ([], {}, {})
    lib = _lib.lib()
    n_groups = len(names)
    files = {r: open(simulation_bed_name(out_prefix, r), "w") for r in write}
    try:
        with TableReader(pred_file, n_class, chunk_bytes) as rd:
            dev = rd.device
            sums = torch.zeros(max(n_groups, 1) * 3 * n_class, dtype=torch.int64, device=dev)
            table = torch.zeros(max(n_groups * (n_class - 1) * n_rep, 1), dtype=torch.int32, device=dev)
            status = torch.zeros(1, dtype=torch.int32, device=dev)
            on_dev, ws = {}, None
            stream = _lib.current_stream_ptr(dev)

            def workspace(need):
                nonlocal ws
                if ws is None or ws.numel() * 8 < need:
                    ws = torch.empty(need // 8 + 1, dtype=torch.int64, device=dev)
                return ws

            for c in rd:
                rows = list(c.run_row[:c.n_runs]) + [int(c.n_rows)]
                for r in range(c.n_runs):
                    name = rd.chrom_name(c.run_chrom[r])
                    a, b = rows[r], rows[r + 1]
                    if b == a:
                        continue
                    key = simulate_chrom_key(name)
                    if name in pieces:
                        if name not in on_dev:
                            on_dev[name] = tuple(torch.from_numpy(np.ascontiguousarray(x)).to(dev) for x in pieces[name])
                        b0, b1, grp = on_dev[name]
                        s = _lib.MuralSummaryAnnotRows()
                        s.prob, s.prob_f64, s.prob_stride = c.prob + 8 * n_class * a, 1, n_class
                        s.start, s.label, s.label_kind = c.start + 8 * a, c.mut_type + 4 * a, 1
                        s.n, s.n_class, s.n_groups = b - a, n_class, n_groups
                        s.piece_b0, s.piece_b1, s.piece_group, s.n_pieces = b0.data_ptr(), b1.data_ptr(), grp.data_ptr(), b0.shape[0]
                        s.table, s.status = sums.data_ptr(), status.data_ptr()
                        w = workspace(int(lib.mural_summary_annot_workspace_bytes(b - a, n_class)))
                        _lib.check(lib.mural_summary_annot_rows(C.byref(s), w.data_ptr(), w.numel() * 8, stream))
                        m = _lib.MuralSimulateAnnotRows()
                        m.prob, m.prob_f64, m.prob_stride, m.n_class = c.prob + 8 * n_class * a, 1, n_class, n_class
                        m.start, m.strand, m.n = c.start + 8 * a, c.strand + a, b - a
                        m.chrom_key, m.n_rep, m.seed = key, n_rep, seed
                        m.piece_b0, m.piece_b1, m.piece_group, m.n_pieces = b0.data_ptr(), b1.data_ptr(), grp.data_ptr(), b0.shape[0]
                        m.n_groups, m.table, m.status = n_groups, table.data_ptr(), status.data_ptr()
                        w = workspace(int(lib.mural_simulate_annot_workspace_bytes(b0.shape[0])))
                        _lib.check(lib.mural_simulate_annot_rows(C.byref(m), w.data_ptr(), w.numel() * 8, stream))
                    for rep in write:      # (a table is read at the host's pace: the list is read back part by part)
                        out = (torch.empty(b - a, dtype=torch.int64, device=dev), torch.empty(b - a, dtype=torch.uint8, device=dev),
                               torch.empty(b - a, dtype=torch.uint8, device=dev), torch.zeros(1, dtype=torch.int64, device=dev))
                        m = _lib.MuralSimulateRows()
                        m.prob, m.prob_f64, m.prob_stride, m.n_class = c.prob + 8 * n_class * a, 1, n_class, n_class
                        m.start, m.strand, m.n = c.start + 8 * a, c.strand + a, b - a
                        m.chrom_key, m.replicate, m.seed = key, rep, seed
                        m.out_start, m.out_strand, m.out_label, m.count = (out[0].data_ptr(), out[1].data_ptr(), out[2].data_ptr(),
                                                                           out[3].data_ptr())
                        m.status = status.data_ptr()
                        w = workspace(int(lib.mural_simulate_rows_workspace_bytes(b - a)))
                        _lib.check(lib.mural_simulate_rows(C.byref(m), w.data_ptr(), w.numel() * 8, stream))
                        hits = int(out[3].item())
                        files[rep].write(simulation_bed_text(name, *(x[:hits].cpu().numpy() for x in out[:3])))
            bits = int(status.item())
            for bit, what in _SUMMARY_STATUS:
                if bits & bit:
                    raise ValueError(f"{pred_file}: {what}")
            annot = annot_table_from_sums(sums.cpu().numpy().view(np.uint64)[:n_groups * 3 * n_class].reshape(n_groups, 3, n_class), n_class)
            counts = table.cpu().numpy().view(np.uint32)[:n_groups * (n_class - 1) * n_rep].reshape(n_groups, n_class - 1, n_rep)
    finally:
        for fh in files.values():
            fh.close()
    return names, counts, (annot[:, 2:1 + n_class] if labels else None), annot[:, 2 + n_class:1 + 2 * n_class]


def run_simulate_calc(args, chunk_bytes=DEFAULT_CHUNK_BYTES):
    """For an `evaluate`-style caller (args.pred_file, args.annotations, args.simulate, args.seed, args.n_class, args.out_prefix,
    optionally args.write_simulated): the simulated counts per name of the annotation BED from the table's rows; writes
    {out_prefix}.annotation.sim.tsv and the mutation lists asked for."""
    assert getattr(args, "seed", None) is not None, "--seed is required with --simulate: there is no default randomness"
    write = tuple(getattr(args, "write_simulated", None) or ())
    names, counts, observed, expected = simulate_table(os.fspath(args.pred_file), getattr(args, "annotations", None), args.simulate, args.seed,
                                                       args.n_class, write, args.out_prefix, True, chunk_bytes)
    if getattr(args, "annotations", None) is None:
        return None
    return write_simulation_outputs(names, counts, observed, expected, args.n_class, args.out_prefix)


def consequence_simulation_output_name(out_prefix):
    return f"{out_prefix}.consequence.sim.tsv"


def write_consequence_simulation_outputs(names, counts, observed, expected, out_prefix):
    """``{out_prefix}.consequence.sim.tsv``: one line per transcript and consequence of ``CONSEQUENCES`` -- name, consequence, observed,
    expected, sim_mean, sim_min, sim_max, n_ge, n_le, p_upper, p_lower (``summaries.simulate_pvalues``) -- from counts
    [transcripts][5][R] (bin 4, unresolved, stays in the counts and gets no line), observed [transcripts][4] (None: no labels, 'NA' in
    the observed column and the last four) and expected [transcripts][4]: the consequence table's own columns.  Returns the path."""
    from .summaries import simulate_pvalues      # (summaries imports this module: not at the top)
    header = ["name", "consequence", "observed", "expected", "sim_mean", "sim_min", "sim_max", "n_ge", "n_le", "p_upper", "p_lower"]
    counts = np.asarray(counts).reshape(len(names), 5, -1)
    stats = [simulate_pvalues(counts[:, b], None if observed is None else np.asarray(observed)[:, b]) for b in range(len(CONSEQUENCES))]
    rows = []
    for j, nm in enumerate(names):
        for b, what in enumerate(CONSEQUENCES):
            mean, lo, hi, n_ge, n_le, p_up, p_lo = stats[b][j]
            obs = "NA" if observed is None else str(int(observed[j][b]))
            tail = ["NA"] * 4 if observed is None else [str(n_ge), str(n_le), _float_text(p_up), _float_text(p_lo)]
            rows.append([nm, what, obs, _float_text(expected[j][b]), _float_text(mean), str(lo), str(hi)] + tail)
    path = consequence_simulation_output_name(out_prefix)
    with open(path, "w") as fh:
        fh.write(_rates_text(header, rows))
    return path


def simulate_consequence_table(pred_file, transcripts, ref_genome, n_rep, seed, codon_table=None, alt_order=None, labels=True,
                               chunk_bytes=DEFAULT_CHUNK_BYTES):
    """(names, counts uint32 [transcripts][5][n_rep], observed or None, expected) from a written SNV prediction table (4 classes): what
    ``SummarySink(simulate=n_rep, simulate_seed=seed, transcripts=..., simulate_transcripts=True)`` reduces in flight, through the same
    entries (``mural_simulate_conseq_rows`` beside ``mural_summary_conseq_rows``), chromosome run by chromosome run of each chunk; the
    draws are made from the table's four-digit probabilities.  observed and expected [transcripts][4] are the consequence table's
    columns (``consequence_table``); `labels=False`: observed is None."""
    from .data.ingest import read_fasta, scan_fasta
    from .summaries import (_SUMMARY_STATUS, SIMULATE_MAX_REPLICATES, conseq_rows_device,      # (summaries imports this module)
                            simulate_conseq_rows_device)
    n_rep, seed = int(n_rep), int(seed)
    if not 1 <= n_rep <= SIMULATE_MAX_REPLICATES or not 0 <= seed < 1 << 64:
        raise ValueError("simulate_consequence_table: 1 .. 2^20 replicates and an unsigned 64-bit seed")
    names, meta, segments = read_transcripts(transcripts, codon_table)
    alt = check_alt_order(alt_order)
    n_tx = len(names)
    fasta_names = {r.name for r in scan_fasta(ref_genome)}
    with TableReader(pred_file, 4, chunk_bytes) as rd:
        dev = rd.device
        acc = dict(table=torch.zeros(max(n_tx, 1) * 15, dtype=torch.int64, device=dev), rows=torch.zeros(max(n_tx, 1) * 2, dtype=torch.int64, device=dev),
                   status=torch.zeros(1, dtype=torch.int32, device=dev), segments={}, ws=None)
        sim = torch.zeros(max(n_tx * 5 * n_rep, 1), dtype=torch.int32, device=dev)
        genomes = {}
        for c in rd:
            rows = list(c.run_row[:c.n_runs]) + [int(c.n_rows)]
            for r in range(c.n_runs):
                name = rd.chrom_name(c.run_chrom[r])
                a, b = rows[r], rows[r + 1]
                if name not in segments or b == a:
                    continue
                if name not in genomes:
                    if name not in fasta_names:
                        raise ValueError(f"Chromosome {name} not found in {ref_genome} (prediction table line {c.row0 + a + 2})")
                    genomes[name] = read_fasta(ref_genome, dev, names={name})[name]
                part = dict(prob=c.prob + 8 * 4 * a, prob_f64=1, prob_stride=4, start=c.start + 8 * a, strand=c.strand + a, n=b - a)
                conseq_rows_device(acc, name, segments[name], n_tx, meta["aa"], alt, genomes[name].as_struct(), dev,
                                   label=c.mut_type + 4 * a, label_kind=1, **part)
                simulate_conseq_rows_device(sim, acc["status"], acc, name, n_tx, meta["aa"], alt, genomes[name].as_struct(), dev, n_rep, seed,
                                            **part)
        bits = int(acc["status"].item())
        for bit, what in _SUMMARY_STATUS:
            if bits & bit:
                raise ValueError(f"{pred_file}: {what}")
        table = acc["table"].cpu().numpy().view(np.uint64)[:n_tx * 15].reshape(n_tx, 5, 3)
        counts = acc["rows"].cpu().numpy().view(np.uint64)[:n_tx * 2].reshape(n_tx, 2)
        sim = sim.cpu().numpy().view(np.uint32)[:n_tx * 5 * n_rep].reshape(n_tx, 5, n_rep)
    conseq = consequence_table_from_sums(table, counts)
    return names, sim, (conseq[:, 4:11:2] if labels else None), conseq[:, 3:11:2]


def run_simulate_consequence_calc(args, chunk_bytes=DEFAULT_CHUNK_BYTES):
    """For an `evaluate`-style caller (args.pred_file, args.transcripts, args.ref_genome, args.simulate, args.seed, args.out_prefix;
    optional args.codon_table, args.alt_order): the simulated counts per transcript and consequence from the table's rows; writes
    {out_prefix}.consequence.sim.tsv."""
    assert getattr(args, "transcripts", None) is not None, "--transcripts is required for the consequence simulation"
    assert getattr(args, "ref_genome", None) is not None, "--ref_genome is required for the consequence simulation"
    assert getattr(args, "seed", None) is not None, "--seed is required with --simulate: there is no default randomness"
    names, counts, observed, expected = simulate_consequence_table(os.fspath(args.pred_file), args.transcripts, os.fspath(args.ref_genome),
                                                                   args.simulate, args.seed, getattr(args, "codon_table", None),
                                                                   getattr(args, "alt_order", None), True, chunk_bytes)
    return write_consequence_simulation_outputs(names, counts, observed, expected, args.out_prefix)


def structure_simulation_output_name(out_prefix):
    return f"{out_prefix}.consequence.structure.sim.tsv"


def write_structure_simulation_outputs(names, counts, lof, observed, expected, out_prefix):
    """``{out_prefix}.consequence.structure.sim.tsv``: one line per transcript and row of ``STRUCTURE_BINS`` + ("lof",) -- name, bin,
    observed, expected, sim_mean, sim_min, sim_max, n_ge, n_le, p_upper, p_lower (``summaries.simulate_pvalues``) -- from counts
    [transcripts][9][R], lof [transcripts][R] (``summaries.simulate_lof_counts``), observed [transcripts][10] (None: no labels, 'NA' in
    the observed column and the last four) and expected [transcripts][10]: the structure file's own numbers
    (``structure_cells_from_sums``), LoF last.  Returns the path."""
    from .summaries import simulate_pvalues      # (summaries imports this module: not at the top)
    header = ["name", "bin", "observed", "expected", "sim_mean", "sim_min", "sim_max", "n_ge", "n_le", "p_upper", "p_lower"]
    counts = np.asarray(counts).reshape(len(names), 9, -1)
    lof = np.asarray(lof).reshape(len(names), -1)
    what_all = STRUCTURE_BINS + ("lof",)
    stats = [simulate_pvalues(counts[:, b] if b < 9 else lof, None if observed is None else np.asarray(observed)[:, b])
             for b in range(len(what_all))]
    rows = []
    for j, nm in enumerate(names):
        for b, what in enumerate(what_all):
            mean, lo, hi, n_ge, n_le, p_up, p_lo = stats[b][j]
            obs = "NA" if observed is None else str(int(observed[j][b]))
            tail = ["NA"] * 4 if observed is None else [str(n_ge), str(n_le), _float_text(p_up), _float_text(p_lo)]
            rows.append([nm, what, obs, _float_text(expected[j][b]), _float_text(mean), str(lo), str(hi)] + tail)
    path = structure_simulation_output_name(out_prefix)
    with open(path, "w") as fh:
        fh.write(_rates_text(header, rows))
    return path


def simulate_structure_table(pred_file, transcripts, ref_genome, n_rep, seed, codon_table=None, alt_order=None, labels=True,
                             chunk_bytes=DEFAULT_CHUNK_BYTES):
    """(names, counts uint32 [transcripts][9][n_rep], lof int64 [transcripts][n_rep], observed [transcripts][10] or None, expected
    [transcripts][10]) from a written SNV prediction table (4 classes): what ``SummarySink(simulate=n_rep, simulate_seed=seed,
    transcripts=..., transcript_structure=True, simulate_transcripts=True, simulate_structure=True)`` reduces in flight, through the
    same entries (``mural_simulate_txstruct_rows`` beside ``mural_summary_conseq_rows``, ``mural_simulate_conseq_rows`` and
    ``mural_summary_txstruct_rows``), chromosome run by chromosome run of each chunk; the draws are made from the table's four-digit
    probabilities.  observed and expected are the structure table's numbers, LoF last; `labels=False`: observed is None."""
    from .data.ingest import read_fasta, scan_fasta
    from .summaries import (_SUMMARY_STATUS, SIMULATE_MAX_REPLICATES, conseq_rows_device,      # (summaries imports this module)
                            simulate_conseq_rows_device, simulate_lof_counts, simulate_txstruct_rows_device, txstruct_rows_device)
    n_rep, seed = int(n_rep), int(seed)
    if not 1 <= n_rep <= SIMULATE_MAX_REPLICATES or not 0 <= seed < 1 << 64:
        raise ValueError("simulate_structure_table: 1 .. 2^20 replicates and an unsigned 64-bit seed")
    names, meta, segments, features = read_transcript_structure(transcripts, codon_table)
    alt = check_alt_order(alt_order)
    n_tx = len(names)
    fasta_names = {r.name for r in scan_fasta(ref_genome)}
    with TableReader(pred_file, 4, chunk_bytes) as rd:
        dev = rd.device
        acc = _structure_acc(n_tx, dev)
        sim_conseq = torch.zeros(max(n_tx * 5 * n_rep, 1), dtype=torch.int32, device=dev)
        sim = torch.zeros(max(n_tx * 9 * n_rep, 1), dtype=torch.int32, device=dev)
        genomes = {}
        for c in rd:
            rows = list(c.run_row[:c.n_runs]) + [int(c.n_rows)]
            for r in range(c.n_runs):
                name = rd.chrom_name(c.run_chrom[r])
                a, b = rows[r], rows[r + 1]
                if name not in features or b == a:
                    continue
                if name not in genomes:
                    if name not in fasta_names:
                        raise ValueError(f"Chromosome {name} not found in {ref_genome} (prediction table line {c.row0 + a + 2})")
                    genomes[name] = read_fasta(ref_genome, dev, names={name})[name]
                genome = genomes[name].as_struct()
                part = dict(prob=c.prob + 8 * 4 * a, prob_f64=1, prob_stride=4, start=c.start + 8 * a, strand=c.strand + a, n=b - a)
                labelled = dict(label=c.mut_type + 4 * a, label_kind=1, **part)
                if name in segments:
                    conseq_rows_device(acc["conseq"], name, segments[name], n_tx, meta["aa"], alt, genome, dev, **labelled)
                    simulate_conseq_rows_device(sim_conseq, acc["status"], acc["conseq"], name, n_tx, meta["aa"], alt, genome, dev, n_rep,
                                                seed, **part)
                txstruct_rows_device(acc, acc["conseq"], name, segments.get(name), features[name], n_tx, meta["aa"], alt, genome, dev,
                                     **labelled)
                simulate_txstruct_rows_device(sim, acc["status"], acc, acc["conseq"], name, n_tx, meta["aa"], alt, genome, dev, n_rep, seed,
                                              **part)
        bits = int(acc["status"].item()) | int(acc["conseq"]["status"].item())
        for bit, what in _SUMMARY_STATUS:
            if bits & bit:
                raise ValueError(f"{pred_file}: {what}")
        table = acc["table"].cpu().numpy().view(np.uint64)[:n_tx * 27].reshape(n_tx, 9, 3)
        stop_gained = acc["conseq"]["table"].cpu().numpy().view(np.uint64)[:n_tx * 15].reshape(n_tx, 5, 3)[:, 2].copy()
        sim_conseq = sim_conseq.cpu().numpy().view(np.uint32)[:n_tx * 5 * n_rep].reshape(n_tx, 5, n_rep)
        sim = sim.cpu().numpy().view(np.uint32)[:n_tx * 9 * n_rep].reshape(n_tx, 9, n_rep)
    expected, observed = structure_cells_from_sums(table, stop_gained)
    return names, sim, simulate_lof_counts(sim_conseq, sim), (observed if labels else None), expected


def run_simulate_structure_calc(args, chunk_bytes=DEFAULT_CHUNK_BYTES):
    """For an `evaluate`-style caller (args.pred_file, args.transcripts, args.ref_genome, args.simulate, args.seed, args.out_prefix;
    optional args.codon_table, args.alt_order): the simulated counts per transcript, structure bin and LoF from the table's rows;
    writes {out_prefix}.consequence.structure.sim.tsv."""
    assert getattr(args, "transcripts", None) is not None, "--transcripts is required for the structure simulation"
    assert getattr(args, "ref_genome", None) is not None, "--ref_genome is required for the structure simulation"
    assert getattr(args, "seed", None) is not None, "--seed is required with --simulate: there is no default randomness"
    result = simulate_structure_table(os.fspath(args.pred_file), args.transcripts, os.fspath(args.ref_genome), args.simulate, args.seed,
                                      getattr(args, "codon_table", None), getattr(args, "alt_order", None), True, chunk_bytes)
    return write_structure_simulation_outputs(*result, args.out_prefix)


def indel_structure_simulation_output_name(out_prefix):
    return f"{out_prefix}.indel_structure.sim.tsv"


def write_indel_structure_simulation_outputs(names, counts, lof, lof_upper, observed, expected, out_prefix):
    """``{out_prefix}.indel_structure.sim.tsv``: one line per transcript and row of ``INDEL_STRUCTURE_BINS`` + ("lof", "lof_upper") --
    name, bin, observed, expected, sim_mean, sim_min, sim_max, n_ge, n_le, p_upper, p_lower (``summaries.simulate_pvalues``) -- from
    counts [transcripts][10][R], lof and lof_upper [transcripts][R] (``summaries.simulate_indel_lof_counts``), observed
    [transcripts][12] (None: no labels, 'NA' in the observed column and the last four) and expected [transcripts][12]: the numbers
    ``write_indel_structure_outputs`` writes (``indel_structure_cells_from_sums``), lof and lof_upper last.  Returns the path."""
    from .summaries import simulate_pvalues      # (summaries imports this module: not at the top)
    header = ["name", "bin", "observed", "expected", "sim_mean", "sim_min", "sim_max", "n_ge", "n_le", "p_upper", "p_lower"]
    counts = np.asarray(counts).reshape(len(names), 10, -1)
    extra = (np.asarray(lof).reshape(len(names), -1), np.asarray(lof_upper).reshape(len(names), -1))
    what_all = INDEL_STRUCTURE_BINS + ("lof", "lof_upper")
    stats = [simulate_pvalues(counts[:, b] if b < 10 else extra[b - 10], None if observed is None else [row[b] for row in observed])
             for b in range(len(what_all))]
    rows = []
    for j, nm in enumerate(names):
        for b, what in enumerate(what_all):
            mean, lo, hi, n_ge, n_le, p_up, p_lo = stats[b][j]
            obs = "NA" if observed is None else str(int(observed[j][b]))
            tail = ["NA"] * 4 if observed is None else [str(n_ge), str(n_le), _float_text(p_up), _float_text(p_lo)]
            rows.append([nm, what, obs, _float_text(expected[j][b]), _float_text(mean), str(lo), str(hi)] + tail)
    path = indel_structure_simulation_output_name(out_prefix)
    with open(path, "w") as fh:
        fh.write(_rates_text(header, rows))
    return path


def simulate_indel_structure_table(pred_file, transcripts, n_class, kind, n_rep, seed, lengths=None, breakpoint_offset=1,
                                   chrom_lengths=None, labels=True, chunk_bytes=DEFAULT_CHUNK_BYTES):
    """(names, counts uint32 [transcripts][10][n_rep], lof int64 [transcripts][n_rep], lof_upper the same, observed [transcripts][12]
    or None, expected [transcripts][12]) from a written INDEL prediction table of `n_class` classes (2 .. 8): what
    ``SummarySink(simulate=n_rep, simulate_seed=seed, indel_transcripts=..., indel_kind=kind, simulate_indel_structure=True)`` reduces
    in flight, through the same entries (``mural_simulate_txindel_rows`` beside ``mural_summary_txindel_rows``), chromosome run by
    chromosome run of each chunk.  The draws are made from the table's four-digit probabilities, not from the model's: as DESIGN.md
    section 3.20 says of every table route, the counts differ from the in-flight ones of the same seed wherever the rounding moves a
    class bound across a draw.  observed and expected are the INDEL structure file's numbers, lof and lof_upper last;
    `labels=False`: observed is None.  `kind`, `lengths`, `breakpoint_offset`, `chrom_lengths`: ``indel_structure_table``'s."""
    from .summaries import (_SUMMARY_STATUS, SIMULATE_MAX_REPLICATES, simulate_indel_lof_counts,      # (summaries imports this module)
                            simulate_txindel_rows_device, txindel_rows_device)
    n_rep, seed, k = int(n_rep), int(seed), int(n_class)
    if not 1 <= n_rep <= SIMULATE_MAX_REPLICATES or not 0 <= seed < 1 << 64:
        raise ValueError("simulate_indel_structure_table: 1 .. 2^20 replicates and an unsigned 64-bit seed")
    if not 2 <= k <= 8:
        raise ValueError(f"simulate_indel_structure_table: 2 .. 8 classes, the bound of the simulation's draw (got {k})")
    names, meta, segments, features = read_transcript_structure(transcripts)
    kind, off = check_indel_kind(kind), check_breakpoint_offset(breakpoint_offset)
    class_len = check_indel_lengths(lengths, k)
    n_tx = len(names)
    links = {}
    with TableReader(pred_file, k, chunk_bytes) as rd:
        dev = rd.device
        acc = _indel_structure_acc(n_tx, dev)
        sim = torch.zeros(max(n_tx * 10 * n_rep, 1), dtype=torch.int32, device=dev)
        for c in rd:
            rows = list(c.run_row[:c.n_runs]) + [int(c.n_rows)]
            for r in range(c.n_runs):
                name = rd.chrom_name(c.run_chrom[r])
                a, b = rows[r], rows[r + 1]
                if name not in features or b == a:
                    continue
                if name not in links:
                    links[name] = structure_links(features[name])
                length = None if chrom_lengths is None else chrom_lengths.get(name)
                part = dict(prob=c.prob + 8 * k * a, prob_f64=1, prob_stride=k, start=c.start + 8 * a, n=b - a, n_class=k)
                txindel_rows_device(acc, name, segments.get(name), features[name], links[name], n_tx, kind, off, class_len, length, dev,
                                    label=c.mut_type + 4 * a, label_kind=1, **part)
                simulate_txindel_rows_device(sim, acc["status"], acc, name, n_tx, kind, off, class_len, length, dev, n_rep, seed,
                                             strand=c.strand + a, **part)
        bits = int(acc["status"].item())
        for bit, what in _SUMMARY_STATUS:
            if bits & bit:
                raise ValueError(f"{pred_file}: {what}")
        table = acc["table"].cpu().numpy().view(np.uint64)[:n_tx * 30].reshape(n_tx, 10, 3)
        sim = sim.cpu().numpy().view(np.uint32)[:n_tx * 10 * n_rep].reshape(n_tx, 10, n_rep)
    expected, observed = indel_structure_cells_from_sums(table)
    lof, lof_upper = simulate_indel_lof_counts(sim)
    return names, sim, lof, lof_upper, (observed if labels else None), expected


def run_simulate_indel_structure_calc(args, chunk_bytes=DEFAULT_CHUNK_BYTES):
    """For an `evaluate`-style caller (args.pred_file, args.indel_transcripts, args.n_class, args.indel_kind, args.simulate, args.seed,
    args.out_prefix; optional args.indel_lengths, args.breakpoint_offset, args.chrom_lengths): the simulated counts per transcript,
    INDEL structure bin, lof and lof_upper from the table's rows; writes {out_prefix}.indel_structure.sim.tsv."""
    assert getattr(args, "indel_transcripts", None) is not None, "--indel_transcripts is required for the INDEL structure simulation"
    assert getattr(args, "indel_kind", None) is not None, "--indel_kind is required for the INDEL structure simulation"
    assert getattr(args, "seed", None) is not None, "--seed is required with --simulate: there is no default randomness"
    lengths = getattr(args, "chrom_lengths", None)
    result = simulate_indel_structure_table(os.fspath(args.pred_file), args.indel_transcripts, args.n_class, args.indel_kind, args.simulate,
                                            args.seed, getattr(args, "indel_lengths", None), getattr(args, "breakpoint_offset", 1),
                                            None if lengths is None else read_chrom_lengths(lengths), True, chunk_bytes)
    return write_indel_structure_simulation_outputs(*result, args.out_prefix)


# ------------------------------------------------------------------------------------------------------------------
# evaluate: regional
# ------------------------------------------------------------------------------------------------------------------
_MAX_CHUNK_WINDOWS = 1 << 24


def regional_table(pred_file, window_size, n_class, chunk_bytes=DEFAULT_CHUNK_BYTES):
    """([(chrom, window_end)], table [windows][1 + 2 n_class]) in the reference's dict order (first row of each window)."""
    lib = _lib.lib()
    W = int(window_size)
    if W <= 0:
        raise ValueError(f"--window_size must be positive (got {W})")
    stride = 1 + 2 * n_class
    index, first_row, acc = {}, [], []
    with TableReader(pred_file, n_class, chunk_bytes) as rd:
        dev = rd.device
        stream = lambda: _lib.current_stream_ptr(dev)      # noqa: E731
        status = torch.zeros(1, dtype=torch.int32, device=dev)
        keys = None
        for c in rd:
            n, nch = int(c.n_rows), int(c.n_chroms)
            mn = torch.full((nch,), 2 ** 63 - 1, dtype=torch.int64, device=dev)
            mx = torch.full((nch,), -2 ** 63, dtype=torch.int64, device=dev)
            _lib.check(lib.mural_table_start_range(c.chrom_id, c.start, n, nch, mn.data_ptr(), mx.data_ptr(), stream()))
            mn_h, mx_h = mn.cpu().numpy(), mx.cpu().numpy()
            present = np.nonzero(mx_h >= mn_h)[0]
            if (mn_h[present] < 0).any():
                raise ValueError(f"{pred_file}: a negative start near line {c.row0 + 2}")
            w0 = np.zeros(nch, np.int64)
            base = np.zeros(nch, np.int64)
            n_groups = 0
            for cid in present:
                w0[cid] = mn_h[cid] // W
                base[cid] = n_groups - w0[cid]
                n_groups += int(mx_h[cid] // W - w0[cid] + 1)
            if n_groups * stride >= 2 ** 31 or n_groups > _MAX_CHUNK_WINDOWS:
                raise ValueError(f"{pred_file}: the rows of one chunk span {n_groups} windows of {W} bp; use a smaller chunk_bytes")
            if keys is None or keys.numel() < n:
                keys = torch.empty(n, dtype=torch.int32, device=dev)
            table = torch.zeros((n_groups, stride), dtype=torch.float64, device=dev)
            first = torch.full((n_groups,), -1, dtype=torch.int64, device=dev)
            base_d = torch.from_numpy(base).to(dev)
            _lib.check(lib.mural_eval_window_keys(c.chrom_id, c.start, n, W, base_d.data_ptr(), nch, keys.data_ptr(), status.data_ptr(),
                                                 stream()))
            _group(keys, c, n_class, n_groups, table, status, dev)
            _lib.check(lib.mural_table_first_row(keys.data_ptr(), n, c.row0, 0, n_groups, first.data_ptr(), stream()))
            table, first = table.cpu().numpy(), first.cpu().numpy().view(np.uint64)
            for cid in present:
                g0 = int(base[cid] + w0[cid])
                g1 = int(base[cid] + mx_h[cid] // W) + 1
                for g in np.nonzero(table[g0:g1, 0] > 0)[0] + g0:
                    key = (rd.chrom_name(int(cid)), int((g - base[cid]) * W + W))
                    j = index.get(key)
                    if j is None:
                        index[key] = len(acc)
                        acc.append(table[g].copy())
                        first_row.append(int(first[g]))
                    else:
                        acc[j] += table[g]
        _check_status(status, pred_file)
    keys_out = list(index)
    order = np.argsort(np.asarray(first_row, np.uint64), kind="stable")
    tab = np.asarray(acc, np.float64).reshape(-1, stride)
    return [keys_out[j] for j in order], tab[order]


def write_regional_outputs(keys, table, n_class, window_size, out_prefix, ratio_cutoff):
    """The two files of calc_regional_corr.py:190-212 from a window table (``regional_table``'s pair, or the one a
    ``predict.SummarySink`` reduced in flight): per window observed / predicted rates (float32), used_or_deprecated by
    ratio_cutoff * median(number_of_all), Pearson r over the used windows.  Returns [(class, (r, p))]."""
    W = int(window_size)
    obs, pred, cnt, tot = _rates(table, n_class)
    obs32, pred32 = obs.astype(np.float32), pred.astype(np.float32)
    cutoff = float(ratio_cutoff) * np.median(tot.astype(np.uint64))
    used = tot >= cutoff
    cls = range(1, n_class)
    header = (["chrom", "window_end"] + [f"avg_obs_rate{i}" for i in cls] + [f"avg_pred_rate{i}" for i in cls]
              + [f"number_of_mut{i}" for i in cls] + ["number_of_all", "used_or_deprecated"])
    rows = [[ch, str(we)] + [str(v) for v in obs32[j]] + [str(v) for v in pred32[j]] + [str(int(v)) for v in cnt[j]]
            + [str(int(tot[j])), "used" if used[j] else "deprecated"] for j, (ch, we) in enumerate(keys)]
    rates_path, corr_path, window = regional_output_names(out_prefix, W)
    corrs = [(c, pearson(obs32[used, c - 1], pred32[used, c - 1])) for c in cls]
    with open(rates_path, "w") as fh:
        fh.write(_rates_text(header, rows))
    with open(corr_path, "w") as fh:
        fh.write(_corr_text(window, corrs))
    return corrs


def run_regional_corr_calc(args, chunk_bytes=DEFAULT_CHUNK_BYTES):
    """calc_regional_corr.py:164-212: per window observed / predicted rates (float32), used_or_deprecated by ratio_cutoff *
    median(number_of_all), Pearson r over the used windows; writes {out_prefix}.{W/1000}Kb.mut_rates.tsv and .corr.txt."""
    W = int(args.window_size)
    keys, table = regional_table(os.fspath(args.pred_file), W, args.n_class, chunk_bytes)
    return write_regional_outputs(keys, table, args.n_class, W, args.out_prefix, args.ratio_cutoff)


def mu_scaling_factor(genomewide_mu, n_sites, m_proportion, g_proportion, prob_sum):
    """scaling.py:92: the factor that makes the mean predicted rate of the table genomewide_mu * m_proportion / g_proportion."""
    return (genomewide_mu * n_sites * m_proportion / g_proportion) / prob_sum


def print_scaling_factor(genomewide_mu, n_sites, g_proportion, m_proportion, prob_sum, factor):
    """The lines calc_mu_scaling_factor prints below a prediction file's name (scaling.py:94-100)."""
    print("genomewide_mu:", genomewide_mu)
    print("n_sites:", n_sites)
    print("g_proportion:", g_proportion)
    print("m_proportion:", m_proportion)
    print("prob_sum: %.3e" % prob_sum)
    print("scaling factor: %.3e" % factor)


# the reference's module-level name of the file-to-file scaling (scaling.py:10); mural_amd.calibration.apply_scaling is the
# in-memory rule and stays as it is
apply_scaling = apply_scaling_file

__all__ = ["TableReader", "apply_scaling_file", "scaling_files", "calc_mu_scaling_factor", "run_kmer_corr_calc", "run_regional_corr_calc", "write_regional_outputs", "write_kmer_outputs",
           "prob_sum_file", "read_regions", "kmer_table", "regional_table", "motif_table", "run_motif_corr_calc", "write_motif_outputs", "MAX_MOTIF", "check_header", "read_header", "DEFAULT_CHUNK_BYTES", "MAX_KMER"]
