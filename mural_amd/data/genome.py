"""Packed genome (2 bits per base + 1-bit non-ACGT mask) and the GPU window encoders.

Replaces the per-character Python encoders of the reference (MuRaL/data/preprocessing.py:636-723 seq_digit_encoder,
:756-816 seq_ohe_encoder) for sites given as (position, strand): the chromosome is packed once on the host and kept
resident in HBM; windows are decoded inside the kernels.

Format (also documented in include/mural_hip.h): ``packed2`` holds 16 bases per uint32, base i in bits
[2*(i%16), +2) with A0 C1 G2 T3; ``nmask`` holds 32 bases per uint32, bit (i%32) set when the base is not ACGT.
IUPAC ambiguity codes other than N (fractional one-hot columns in the reference, :762-772) are rare: their mask bit is set
(the k-mer encoder treats them like N, :655-666) and a sparse side table ``(amb_pos ascending, amb_sym)`` travels with the
genome; the one-hot encoder and the fused forward resolve them through it.
"""
import ctypes as C

import numpy as np
import torch

from .. import _lib

SYMBOLS = "ACGTNRYMSWKBDHV"          # MURAL_SYM_* of include/mural_hip.h = index in this string
_CODE = np.full(256, 255, dtype=np.uint8)
for _i, _ch in enumerate(SYMBOLS):
    _CODE[ord(_ch)] = _i
    _CODE[ord(_ch.lower())] = _i


def pack_sequence(seq):
    """str/bytes -> (packed2 uint32[], nmask uint32[], length, (positions, symbols) of non-N ambiguity codes)."""
    raw = np.frombuffer(seq.encode("ascii") if isinstance(seq, str) else bytes(seq), dtype=np.uint8)
    codes = _CODE[raw]
    if (codes == 255).any():
        bad = chr(int(raw[int(np.argmax(codes == 255))]))
        raise KeyError(bad)  # the reference's dict lookup raises KeyError on an unknown character
    n = len(codes)
    two = np.where(codes < 4, codes, 0).astype(np.uint32)
    two = np.concatenate([two, np.zeros((-n) % 16, np.uint32)]).reshape(-1, 16)
    packed = np.bitwise_or.reduce(two << (2 * np.arange(16, dtype=np.uint32))[None, :], axis=1).astype(np.uint32)
    m = (codes >= 4).astype(np.uint32)
    m = np.concatenate([m, np.zeros((-n) % 32, np.uint32)]).reshape(-1, 32)
    mask = np.bitwise_or.reduce(m << np.arange(32, dtype=np.uint32)[None, :], axis=1).astype(np.uint32)
    amb = np.nonzero(codes > 4)[0].astype(np.int64)
    return packed, mask, n, (amb, codes[amb].astype(np.uint8))


_FOCAL = {"A": 0, "C": 1, "ANY": 2}                    # MURAL_FOCAL_* of include/mural_hip.h
_CONTEXT = {"all": 0, "cpg": 1, "noncpg": 2}           # MURAL_CONTEXT_*


FOCAL_SET = 3                                          # MURAL_FOCAL_SET: the second selector is a union of MURAL_CLASS_* bits
SITE_CLASSES = {"A": 1, "nonCpG": 2, "CpG": 4, "C": 6}     # MURAL_CLASS_*; 'C' = nonCpG | CpG
ROW_CLASSES = ("A", "nonCpG", "CpG")                   # MURAL_ROW_CLASS_*: what classify_sites writes (255: none of them)


def class_mask(classes):
    """The MURAL_CLASS_* mask (1..7) of a union of site classes: names of SITE_CLASSES (one, or an iterable of them) or the mask itself.
    Raises ValueError for an unknown name and for an empty union."""
    if isinstance(classes, (int, np.integer)) and not isinstance(classes, bool):
        mask = int(classes)
        if not 1 <= mask <= 7:
            raise ValueError(f"classes: a mask is a non-empty union of A = 1, nonCpG = 2, CpG = 4 (1..7), got {mask}")
        return mask
    if classes is None or isinstance(classes, bool) or not (isinstance(classes, str) or hasattr(classes, "__iter__")):
        raise ValueError(f"focal 'SET' needs classes=: names of 'A', 'C', 'nonCpG', 'CpG' or their mask (1..7), got {classes!r}")
    mask = 0
    for name in ([classes] if isinstance(classes, str) else list(classes)):
        if not isinstance(name, str) or name not in SITE_CLASSES:
            raise ValueError(f"classes: unknown site class {name!r} (one of 'A', 'C', 'nonCpG', 'CpG')")
        mask |= SITE_CLASSES[name]
    if mask == 0:
        raise ValueError("classes: an empty union selects no site")
    return mask


def site_selection(focal, context="all", classes=None):
    """(MURAL_FOCAL_*, MURAL_CONTEXT_*) of a site selection: focal 'A' (A/T sites), 'C' (C/G sites) or 'ANY' (every A/C/G/T position,
    INDEL models); context 'all', 'CpG' or 'nonCpG' (any case; focal 'C' only).  focal 'SET': the union of the site classes `classes`
    names (``class_mask``), as (MURAL_FOCAL_SET, the mask); it takes no context.  Raises ValueError."""
    if str(focal).upper() == "SET":
        if str(context).lower() != "all":
            raise ValueError(f"focal 'SET' takes classes=, not a context (got context {context!r})")
        return FOCAL_SET, class_mask(classes)
    if classes is not None:
        raise ValueError(f"classes= goes with focal 'SET' (got focal {focal!r})")
    f, c = _FOCAL.get(str(focal).upper()), _CONTEXT.get(str(context).lower())
    if f is None:
        raise ValueError(f"focal must be 'A', 'C', 'ANY' or 'SET', got {focal!r}")
    if c is None:
        raise ValueError(f"context must be 'all', 'CpG' or 'nonCpG', got {context!r}")
    if c != 0 and f != 1:
        raise ValueError(f"context {context!r} needs focal 'C' (got focal {focal!r})")
    return f, c


STATS_INIT = (0, np.iinfo(np.int64).max)      # the `stats` words of label_sites before the first call


def new_label_stats(device=None):
    """The `stats` pair of ``label_sites`` (a device tensor) / ``label_sites_host`` (device=None: a numpy array) before the first call."""
    if device is None:
        return np.array(STATS_INIT, np.int64)
    return torch.tensor(STATS_INIT, dtype=torch.int64, device=device)


def label_sites_host(pos, strand, muts, check_strand, stats):
    """The specification of ``label_sites`` in numpy: `pos` / `strand` are enumerated sites (pos ascending), `muts` one chromosome's
    (start int64 strictly ascending, strand uint8, label float32) or None.  Returns float32 labels: the label of the list entry whose
    start is the site's position, 0 where there is none.  `stats` (int64[2], started at STATS_INIT) accumulates in place: stats[0] += the
    rows that found an entry, stats[1] = min(stats[1], list index) over matched entries on the other strand than their site -- only
    with `check_strand`."""
    pos, strand = np.asarray(pos, np.int64), np.asarray(strand, np.uint8)
    label = np.zeros(len(pos), np.float32)
    if muts is None or len(muts[0]) == 0 or len(pos) == 0:
        return label
    m_start, m_strand, m_label = muts
    j = np.minimum(np.searchsorted(m_start, pos, "left"), len(m_start) - 1)
    hit = m_start[j] == pos
    label[hit] = np.asarray(m_label, np.float32)[j[hit]]
    stats[0] += int(hit.sum())
    if check_strand:
        wrong = j[hit & (np.asarray(m_strand, np.uint8)[j] != strand)]
        if len(wrong):
            stats[1] = min(int(stats[1]), int(wrong.min()))
    return label


def label_sites(pos, strand, muts, check_strand, stats, out=None):
    """The label column of enumerated sites on the device (``mural_sites_label``: one binary search per site): `pos` int64 / `strand`
    uint8 contiguous device tensors as ``emit_sites`` wrote them, `muts` one chromosome's (start, strand, label) as contiguous device
    tensors (int64 strictly ascending, uint8, float32) or None, `stats` an int64[2] device tensor from ``new_label_stats`` that
    accumulates over calls.  Returns float32 labels (`out` if given).  Same contract as ``label_sites_host``; nothing is read back."""
    n = pos.shape[0]
    if out is None:
        out = torch.empty(n, dtype=torch.float32, device=pos.device)
    tensors = (pos, strand, out, stats) + (tuple(muts) if muts is not None else ())
    want = (torch.int64, torch.uint8, torch.float32, torch.int64, torch.int64, torch.uint8, torch.float32)
    if any(not t.is_cuda or t.device != pos.device or not t.is_contiguous() or t.dtype != dt or t.dim() != 1 for t, dt in zip(tensors, want)):
        raise ValueError("label_sites: pos / strand / out / stats / the mutation list must be contiguous 1-D int64 / uint8 / float32 / "
                         "int64 / (int64, uint8, float32) tensors on one HIP device")
    m = 0 if muts is None else muts[0].shape[0]
    if strand.shape[0] != n or out.shape[0] != n or stats.shape[0] != 2 or (m and (muts[1].shape[0] != m or muts[2].shape[0] != m)):
        raise ValueError("label_sites: pos / strand / out must have one length, stats two entries, the list's columns one length")
    list_ptrs = [t.data_ptr() for t in muts] if m else [None, None, None]
    with torch.cuda.device(pos.device):
        _lib.check(_lib.lib().mural_sites_label(pos.data_ptr(), strand.data_ptr(), n, *list_ptrs,
                                                m, int(bool(check_strand)), out.data_ptr(), stats.data_ptr(),
                                                _lib.current_stream_ptr(pos.device)))
    return out


class SiteScan:
    """The counting pass of a site enumeration (``PackedGenome.scan_sites``): the window, the selection, the per-tile offsets and
    the total, all on the device; ``total`` reads the count back (one synchronisation, cached)."""

    __slots__ = ("lo", "hi", "focal", "context", "offsets", "total_dev", "_total")

    def __init__(self, lo, hi, focal, context, offsets, total_dev):
        self.lo, self.hi, self.focal, self.context, self.offsets, self.total_dev = lo, hi, focal, context, offsets, total_dev
        self._total = None

    @property
    def total(self):
        if self._total is None:
            self._total = int(self.total_dev.item())
        return self._total


class SymbolWindows:
    """Sequence windows as one symbol per column (``PackedGenome.encode_symbols``): ``sym`` is a uint8 (n, W) device tensor of
    MURAL_SYM_* codes (0..14).  Only the encoder makes these -- the kernels index tables with the bytes unchecked."""

    __slots__ = ("sym",)

    def __init__(self, sym):
        self.sym = sym

    @property
    def shape(self):
        return self.sym.shape

    def to(self, *args, **kwargs):
        """The windows on another device (``train_epoch`` moves every member of a batch with ``.to(device)``); self where nothing moves."""
        sym = self.sym.to(*args, **kwargs)
        if sym.dtype != torch.uint8:
            raise TypeError("SymbolWindows hold uint8 symbols: .to() moves them, it does not convert them")
        return self if sym is self.sym else SymbolWindows(sym)


class PackedGenome:
    """One chromosome resident on a HIP device."""

    def __init__(self, packed2, nmask, length, device, ambiguous=None):
        self.length = int(length)
        self.device = torch.device(device)
        # int32 views: torch has no uint32 arithmetic, the kernels reinterpret the bits
        self.packed2 = torch.from_numpy(np.ascontiguousarray(packed2).view(np.int32)).to(self.device)
        self.nmask = torch.from_numpy(np.ascontiguousarray(nmask).view(np.int32)).to(self.device)
        # side table of IUPAC codes other than N: (ascending positions int64, MURAL_SYM_* uint8)
        amb_pos, amb_sym = (np.zeros(0, np.int64), np.zeros(0, np.uint8)) if ambiguous is None else ambiguous
        amb_pos, amb_sym = np.asarray(amb_pos, np.int64), np.asarray(amb_sym, np.uint8)
        if amb_pos.shape != amb_sym.shape or (len(amb_pos) > 1 and (np.diff(amb_pos) <= 0).any()):
            raise ValueError("ambiguity table: positions must ascend strictly and match the symbols in length")
        if len(amb_sym) and (amb_sym.min() < 5 or amb_sym.max() > 14):
            raise ValueError("ambiguity table: symbols must be MURAL_SYM_R .. MURAL_SYM_V (5..14)")
        self.ambiguous = (amb_pos, amb_sym)
        self.amb_pos = torch.from_numpy(amb_pos).to(self.device) if len(amb_pos) else None
        self.amb_sym = torch.from_numpy(amb_sym).to(self.device) if len(amb_pos) else None

    @classmethod
    def from_sequence(cls, seq, device="cuda"):
        packed, mask, n, amb = pack_sequence(seq)
        return cls(packed, mask, n, device, amb)

    def as_struct(self, device=None):
        if device is not None and torch.device(device) != self.packed2.device:
            raise RuntimeError(f"genome lives on {self.packed2.device}, model on {device}")
        if self.amb_pos is None:
            return _lib.MuralGenome(self.packed2.data_ptr(), self.nmask.data_ptr(), self.length, None, None, 0)
        return _lib.MuralGenome(self.packed2.data_ptr(), self.nmask.data_ptr(), self.length, self.amb_pos.data_ptr(),
                                self.amb_sym.data_ptr(), self.amb_pos.shape[0])

    # ------------------------------------------------------------------------------------------------
    def _prep(self, pos, strand):
        pos = torch.as_tensor(pos, dtype=torch.int64, device=self.device).contiguous()
        strand = torch.as_tensor(strand, dtype=torch.uint8, device=self.device).contiguous()
        if pos.shape != strand.shape or pos.dim() != 1:
            raise ValueError("pos and strand must be 1-D and of equal length")
        return pos, strand

    def encode_kmer(self, pos, strand, radius, order, model_type="snv"):
        """int64 (n, 2r+1-(k-1)) [snv] / (n, 2r-(k-1)) [indel] k-mer indices, bit-exact with seq_digit_encoder."""
        if model_type not in ("snv", "indel"):
            raise ValueError(f"model_type {model_type} not supported!")
        pos, strand = self._prep(pos, strand)
        width = 2 * radius + (1 if model_type == "snv" else 0)
        out = torch.empty((pos.shape[0], width - (order - 1)), dtype=torch.int64, device=self.device)
        g = self.as_struct()
        with torch.cuda.device(self.device):
            _lib.check(_lib.lib().mural_encode_kmer(C.byref(g), pos.data_ptr(), strand.data_ptr(), pos.shape[0], int(radius),
                                                   int(order), int(model_type == "indel"), out.data_ptr(),
                                                   _lib.current_stream_ptr(self.device)))
        return out

    def encode_symbols(self, pos, strand, radius, model_type="snv"):
        """The windows of ``encode_onehot`` as one symbol per column (uint8 (n, W), wrapped as ``SymbolWindows``): the training-mode
        forward of the SNV models takes them in place of the dense ``distal_input`` -- its first layer works from symbols anyway, the
        one-hot tensor (16 bytes per column) and its conversion back are skipped.  Same values as the dense route, bit for bit."""
        if model_type not in ("snv", "indel"):
            raise ValueError(f"model_type {model_type} not supported!")
        pos, strand = self._prep(pos, strand)
        width = 2 * radius + (1 if model_type == "snv" else 0)
        out = torch.empty((pos.shape[0], width), dtype=torch.uint8, device=self.device)
        g = self.as_struct()
        with torch.cuda.device(self.device):
            _lib.check(_lib.lib().mural_encode_symbols(C.byref(g), pos.data_ptr(), strand.data_ptr(), pos.shape[0], int(radius),
                                                      int(model_type == "indel"), out.data_ptr(),
                                                      _lib.current_stream_ptr(self.device)))
        return SymbolWindows(out)

    def encode_subst_windows(self, pos, strand, sub_pos, sub_base, radius, local_radius=None, local_order=None, model_type="snv"):
        """One row per (site, substitution): ``(symbols uint8 (n, 2 * radius + 1), cat_x int64 (n, 2 * local_radius + 1 - (local_order - 1)))``,
        bit for bit ``encode_symbols`` / ``encode_kmer`` of (pos, strand) on this genome with the base at the '+'-strand position `sub_pos`
        replaced by the '+'-strand base `sub_base` (0..3; 255: none).  ``model_type="indel"``: ``(symbols uint8 (n, 2 * radius), None)`` of
        the INDEL window, the local arguments are not read.  The genome itself is only read (``mural_amd.mutagenesis``)."""
        from ..mutagenesis import encode_subst_windows
        return encode_subst_windows(self, pos, strand, sub_pos, sub_base, int(radius), None if local_radius is None else int(local_radius),
                                    None if local_order is None else int(local_order), model_type)

    def encode_allele_windows(self, pos, strand, allele, alleles, radius, local_radius=None, local_order=None, model_type="snv"):
        """One row per (site, allele): ``(symbols, cat_x)`` shaped as ``encode_subst_windows`` gives them, bit for bit ``encode_symbols`` /
        ``encode_kmer`` of (pos, strand) on the alternate haplotype of allele ``allele[i]`` of the ``mural_amd.mutagenesis.Alleles`` table
        (an insertion, deletion or multi-base replacement; -1: none).  `pos` is in the coordinates of THAT haplotype.  The genome itself is
        only read."""
        from ..mutagenesis import encode_allele_windows
        return encode_allele_windows(self, pos, strand, allele, alleles, int(radius), None if local_radius is None else int(local_radius),
                                     None if local_order is None else int(local_order), model_type)

    def encode_onehot(self, pos, strand, radius, model_type="snv"):
        """float32 (n, 4, W) one-hot windows (N -> 0.25 each, other IUPAC codes -> their fractional columns), exact w.r.t.
        seq_ohe_encoder."""
        if model_type not in ("snv", "indel"):
            raise ValueError(f"model_type {model_type} not supported!")
        pos, strand = self._prep(pos, strand)
        width = 2 * radius + (1 if model_type == "snv" else 0)
        out = torch.empty((pos.shape[0], 4, width), dtype=torch.float32, device=self.device)
        g = self.as_struct()
        with torch.cuda.device(self.device):
            _lib.check(_lib.lib().mural_encode_onehot(C.byref(g), pos.data_ptr(), strand.data_ptr(), pos.shape[0], int(radius),
                                                     int(model_type == "indel"), out.data_ptr(),
                                                     _lib.current_stream_ptr(self.device)))
        return out

    # ------------------------------------------------------------------------------------------------
    # site enumeration (csrc/sites.hip): the sites of a window straight from the resident genome, no BED file
    def scan_sites(self, lo, hi, focal, context="all", classes=None):
        """Count the sites of the window [lo, hi) (0-based half-open, clamped to the record) on the device: a ``SiteScan`` for
        ``emit_sites``.  Nothing is read back."""
        f, c = site_selection(focal, context, classes)
        lo, hi = int(lo), int(hi)
        lib = _lib.lib()
        tiles = int(lib.mural_sites_tiles(self.length, lo, hi))
        offsets = torch.empty(tiles + 1, dtype=torch.int64, device=self.device)
        total = torch.empty(1, dtype=torch.int64, device=self.device)
        g = self.as_struct()
        with torch.cuda.device(self.device):
            _lib.check(lib.mural_sites_count(C.byref(g), lo, hi, f, c, offsets.data_ptr(), total.data_ptr(),
                                             _lib.current_stream_ptr(self.device)))
        return SiteScan(lo, hi, f, c, offsets, total)

    def emit_sites(self, scan, first, n, pos=None, strand=None):
        """Sites number first .. first + n - 1 of a scan (the caller keeps first + n <= scan.total) as (pos int64, strand uint8)
        device tensors -- freshly allocated, or the given n-entry contiguous ones."""
        first, n = int(first), int(n)
        if pos is None:
            pos = torch.empty(n, dtype=torch.int64, device=self.device)
            strand = torch.empty(n, dtype=torch.uint8, device=self.device)
        elif (pos.shape != (n,) or strand.shape != (n,) or pos.dtype != torch.int64 or strand.dtype != torch.uint8
              or not pos.is_contiguous() or not strand.is_contiguous() or pos.device != self.device or strand.device != self.device):
            raise ValueError("emit_sites: pos / strand must be contiguous int64 / uint8 device tensors of n entries")
        g = self.as_struct()
        with torch.cuda.device(self.device):
            _lib.check(_lib.lib().mural_sites_emit(C.byref(g), scan.lo, scan.hi, scan.focal, scan.context, scan.offsets.data_ptr(),
                                                  first, n, pos.data_ptr(), strand.data_ptr(), _lib.current_stream_ptr(self.device)))
        return pos, strand

    def count_sites(self, lo, hi, focal, context="all", classes=None):
        """Number of sites ``enumerate_sites`` yields for the window."""
        return self.scan_sites(lo, hi, focal, context, classes).total

    def enumerate_sites(self, lo, hi, focal, context="all", first=0, n=None, classes=None):
        """The sites of the window [lo, hi) of the record (0-based half-open like a BED row, clamped to the record) in ascending
        position order: (pos int64, strand uint8) device tensors in the coordinate the encoders and the packed forwards take for a
        BED row (p, p + 1).  focal 'A': A ('+', 0) and T ('-', 1); 'C': C ('+') and G ('-'), with context 'CpG' / 'nonCpG' decided by
        the next ('+') or previous ('-') base of the record; 'ANY': every A/C/G/T position on '+'; 'SET': the sites of every class that
        `classes` names ('A', 'C', 'nonCpG', 'CpG', or their mask), each on its own strand, in one ascending enumeration.  N and IUPAC
        codes are never sites.  `first` / `n`: a contiguous slice of the enumeration (clamped to it; n=None: to its end)."""
        scan = self.scan_sites(lo, hi, focal, context, classes)
        first = max(int(first), 0)
        left = max(scan.total - first, 0)
        n = left if n is None else min(max(int(n), 0), left)
        return self.emit_sites(scan, first, n)

    def classify_sites(self, pos, strand):
        """uint8 device tensor, one entry per (pos, strand) row: the index in ROW_CLASSES of the site's class (0 'A', 1 'nonCpG', 2
        'CpG', by the rules of ``enumerate_sites``), 255 for a position outside the record, an N or IUPAC base, or a strand that is
        not the base's.  Nothing is read back."""
        pos, strand = self._prep(pos, strand)
        cls = torch.empty(pos.shape[0], dtype=torch.uint8, device=self.device)
        g = self.as_struct()
        with torch.cuda.device(self.device):
            _lib.check(_lib.lib().mural_sites_classify(C.byref(g), pos.data_ptr(), strand.data_ptr(), pos.shape[0], cls.data_ptr(),
                                                      _lib.current_stream_ptr(self.device)))
        return cls


def split_rows(cls, n_classes):
    """Stable partition of the rows 0 .. n-1 by a uint8 class column on the device (``mural_rows_split``): (perm int64 [n], counts
    int64 [n_classes + 1]) device tensors.  perm lists the rows of class 0 in ascending order, then class 1, ..; counts[c] are the
    class sizes, counts[n_classes] the rows of a class >= n_classes, which perm leaves out (its last counts[n_classes] entries are
    not written).  No atomics: the same bytes for the same column.  Nothing is read back."""
    if not cls.is_cuda or cls.dtype != torch.uint8 or cls.dim() != 1 or not cls.is_contiguous():
        raise ValueError("split_rows: cls must be a contiguous 1-D uint8 tensor on a HIP device")
    n, k = cls.shape[0], int(n_classes)
    lib = _lib.lib()
    perm = torch.empty(n, dtype=torch.int64, device=cls.device)
    counts = torch.empty(k + 1, dtype=torch.int64, device=cls.device)
    ws_bytes = int(lib.mural_rows_split_workspace_bytes(n, k))
    ws = torch.empty(max(ws_bytes // 8, 1), dtype=torch.int64, device=cls.device)
    with torch.cuda.device(cls.device):
        _lib.check(lib.mural_rows_split(cls.data_ptr(), n, k, perm.data_ptr(), counts.data_ptr(), ws.data_ptr(), ws_bytes,
                                        _lib.current_stream_ptr(cls.device)))
    return perm, counts


def scatter_rows(src, perm, dst):
    """dst[perm[j], :] = src[j, :] on the device (``mural_rows_scatter``): `src` (m, cols) and `dst` (rows, cols) contiguous float32 or
    float64 tensors of one dtype, `perm` m distinct int64 row numbers of dst (a contiguous slice of ``split_rows``' perm).  Returns dst."""
    if (not src.is_cuda or src.device != dst.device or perm.device != src.device or src.dtype != dst.dtype
            or src.dtype not in (torch.float32, torch.float64) or perm.dtype != torch.int64 or src.dim() != 2 or dst.dim() != 2
            or perm.dim() != 1 or src.shape[1] != dst.shape[1] or src.shape[1] < 1 or perm.shape[0] != src.shape[0]
            or not (src.is_contiguous() and dst.is_contiguous() and perm.is_contiguous())):
        raise ValueError("scatter_rows: src (m, cols) / dst (rows, cols) must be contiguous float32 or float64 tensors of one dtype on "
                         "one HIP device, perm m contiguous int64 entries")
    with torch.cuda.device(src.device):
        _lib.check(_lib.lib().mural_rows_scatter(src.data_ptr(), perm.data_ptr(), src.shape[0], src.shape[1], src.element_size(),
                                                dst.data_ptr(), dst.shape[0], _lib.current_stream_ptr(src.device)))
    return dst
