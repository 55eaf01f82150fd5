"""In-silico saturation mutagenesis and variant footprints on top of the SNV and INDEL forwards (csrc/mutagenesis.hip; DESIGN.md
sections 3.27 to 3.30).

``saturation_mutagenesis`` answers "which bases of the +-distal_radius window make this site's rate what it is": every column of the
window is replaced by each of its three alternatives, the window re-predicted, and the change in log-probability reported as a map
``delta[site, column, alternative base, class]``.  ``variant_footprint`` is the transposed question: what one variant does to the rate of
every site around it.  Both encode "the window as if one base were different" on the device (``mural_encode_subst_windows``) and run the
models' ``forward_symbols``; nothing patches a FASTA and no dense one-hot tensor is assembled.  For the INDEL model (``UNet_Small``)
the window is [pos - R + 1, pos + R] (W = 2 R) and the log-probabilities are the log-softmax of the forward's Softplus scores
(``mural_scores_log_softmax``), which is what predict writes.

The numpy twins (``encode_subst_windows_host``, ``mutagenesis_rows_host``, ``mutagenesis_reduce_host``) are the specification the CPU
tests pin against brute force (patch the sequence string, encode with the oracle); ``log_softmax_host`` is the float64 twin of the
log-softmax.

``allele_footprint`` is the footprint of an allele that may change the sequence's length -- an insertion, a deletion, a multi-base
replacement (``Alleles``) -- on the sites it can reach; its windows come from ``mural_encode_allele_windows``, which reads the
alternate haplotype in its own coordinates.  Twins: ``encode_allele_windows_host``, ``allele_rows_host``; ``alternate_sequence`` is the
string patch they are pinned against.

``mutagenesis_profile`` is the map reduced over sites in flight (section 3.30): the same chunk loop with an accumulating kernel
(``mural_mutagenesis_profile_window``) in the place of the reduce, exact integer sums per [group, column, reference base, alternative,
class] in a ``MutagenesisProfile`` whose tables add across chunks, calls and ranks.  Twin: ``mutagenesis_profile_host``.
"""
import ctypes as C

import numpy as np
import torch

from . import _lib
from .data.genome import _CODE, PackedGenome, SymbolWindows  # noqa: F401

NO_SUBST = 255                      # sub_base of "no substitution"
_COMPLEMENT = np.array([3, 2, 1, 0, 4, 6, 5, 10, 8, 9, 7, 14, 13, 12, 11, 15], np.uint8)      # csrc/common.h: sym_complement


# ----------------------------------------------------------------------------------------------------------------------------------
# host twins
# ----------------------------------------------------------------------------------------------------------------------------------
def _codes(genome):
    """uint8 MURAL_SYM_* codes of a sequence (str / bytes) or of such a code array."""
    if isinstance(genome, (str, bytes)):
        raw = np.frombuffer(genome.encode("ascii") if isinstance(genome, str) else bytes(genome), np.uint8)
        codes = _CODE[raw]
        if (codes == 255).any():
            raise KeyError(chr(int(raw[int(np.argmax(codes == 255))])))
        return codes
    return np.asarray(genome, np.uint8)


def _window(radius, model_type="snv"):
    """(offset of the window's first base from the site, W): csrc/common.h window_geometry"""
    if model_type not in ("snv", "indel"):
        raise ValueError(f"model_type {model_type} not supported!")
    return (-radius, 2 * radius + 1) if model_type == "snv" else (-radius + 1, 2 * radius)


def _window_symbols_host(codes, pos, strand, radius, sub_pos=None, sub_base=None, model_type="snv"):
    """(n, W) strand-oriented symbols of the sites' windows ('-': reversed and complemented; outside the record: N), with the base at
    sub_pos replaced by sub_base where the row has a substitution."""
    pos, neg = np.asarray(pos, np.int64), np.asarray(strand) != 0
    (off0, W), L = _window(radius, model_type), len(codes)
    j = np.arange(W, dtype=np.int64)
    gp = pos[:, None] + off0 + np.where(neg[:, None], W - 1 - j[None, :], j[None, :])  # genome position of column j
    inside = (gp >= 0) & (gp < L)
    sym = np.full(gp.shape, 4, np.uint8)
    sym[inside] = codes[gp[inside]]
    if sub_pos is not None:
        sp, sb = np.asarray(sub_pos, np.int64), np.asarray(sub_base, np.uint8)
        live = (sb < 4) & (sp >= 0) & (sp < L)
        hit = live[:, None] & (gp == sp[:, None])
        sym = np.where(hit, sb[:, None], sym)
    return np.where(neg[:, None], _COMPLEMENT[sym], sym).astype(np.uint8), gp


def encode_subst_windows_host(genome, pos, strand, sub_pos, sub_base, radius, local_radius=None, local_order=None, model_type="snv"):
    """The numpy twin of ``mural_encode_subst_windows``: (symbols uint8 (n, 2 * radius + 1), cat_x int64 (n, 2 * local_radius + 1 -
    (local_order - 1))) of the rows' windows on the genome with the base at sub_pos replaced by sub_base ('+'-strand base 0..3; above 3:
    no substitution; a position outside the record or the window changes nothing).  ``model_type="indel"``: the twin of
    ``mural_encode_subst_symbols(.., indel = 1)``, (symbols uint8 (n, 2 * radius), None)."""
    codes = _codes(genome)
    symbols, _ = _window_symbols_host(codes, pos, strand, radius, sub_pos, sub_base, model_type)
    if model_type == "indel":
        return symbols, None
    local, _ = _window_symbols_host(codes, pos, strand, local_radius, sub_pos, sub_base)
    ncol = 2 * local_radius + 1 - (local_order - 1)
    digit = local.astype(np.int64)
    val = np.zeros((len(digit), ncol), np.int64)
    bad = np.zeros((len(digit), ncol), bool)
    for d in range(local_order):
        col = digit[:, d:d + ncol]
        bad |= col > 3                                   # N and the IUPAC codes alike (preprocessing.py:655-666)
        val = val * 4 + np.where(col > 3, 0, col)
    return symbols, np.where(bad, 4 ** local_order, val)


def _ids(first, count, W):
    v = first + np.arange(count, dtype=np.int64)
    cell, a = v // 3, v % 3
    return cell // W, cell % W, a


def mutagenesis_ids_host(first, count, radius, model_type="snv"):
    """(site, column, a) of the variant ids [first, first + count): v = (site * W + column) * 3 + a."""
    return _ids(first, count, _window(radius, model_type)[1])


def mutagenesis_rows_host(genome, pos, strand, radius, first, count, model_type="snv"):
    """The numpy twin of ``mural_mutagenesis_rows`` (``.._window``): (row_pos int64, row_strand uint8, sub_pos int64, sub_base uint8) of
    the ids [first, first + count).  In window orientation the alternative is the a-th of {A, C, G, T} without the column's reference
    symbol, ascending; sub_base is that alternative on the '+' strand; a column that is not A/C/G/T gives 255."""
    codes = _codes(genome)
    pos, strand = np.asarray(pos, np.int64), (np.asarray(strand) != 0).astype(np.uint8)
    W = _window(radius, model_type)[1]
    if first < 0 or count < 0 or first + count > len(pos) * W * 3:
        raise ValueError("mutagenesis_rows: ids [first, first + count) must lie in [0, n_sites * W * 3)")
    site, j, a = _ids(first, count, W)
    sym, gp = _window_symbols_host(codes, pos, strand, radius, model_type=model_type)
    ref = sym[site, j].astype(np.int64)
    alt = a + (a >= ref)
    neg = strand[site] != 0
    sub_base = np.where(ref < 4, np.where(neg, 3 - alt, alt), NO_SUBST).astype(np.uint8)
    return pos[site], strand[site], gp[site, j], sub_base


def mutagenesis_reduce_host(ref_logp, var_logp, ref_symbols, first, delta, logp_map=None):
    """The numpy twin of ``mural_mutagenesis_reduce`` (``.._window``: any W >= 1): scatters var_logp (count, n_class) of the ids [first, first + count) into `delta`
    (n_sites, W, 4, n_class) float32 in place (and var_logp itself into `logp_map`).  Id a of an A/C/G/T column writes its alternative's
    entry, id a = 0 the reference base's (+0.0; ref_logp in the second map) too; in any other column id a writes NaN to entry a, id a = 2
    to entry 3 as well."""
    ref_logp, var_logp = np.asarray(ref_logp, np.float32), np.asarray(var_logp, np.float32)
    ref_symbols = np.asarray(ref_symbols, np.uint8)
    n, W = ref_symbols.shape
    site, j, a = _ids(first, len(var_logp), W)
    ref = ref_symbols[site, j].astype(np.int64)
    plain = ref < 4
    alt = a + (a >= ref)
    nan = np.float32(np.nan)
    s, c, b = site[plain], j[plain], alt[plain]
    delta[s, c, b] = var_logp[plain] - ref_logp[s]
    if logp_map is not None:
        logp_map[s, c, b] = var_logp[plain]
    z = plain & (a == 0)
    delta[site[z], j[z], ref[z]] = np.float32(0.0)
    if logp_map is not None:
        logp_map[site[z], j[z], ref[z]] = ref_logp[site[z]]
    for maps in (delta, logp_map):
        if maps is None:
            continue
        maps[site[~plain], j[~plain], a[~plain]] = nan
        last = ~plain & (a == 2)
        maps[site[last], j[last], 3] = nan
    return delta


PROFILE_WORDS = 5                   # n, sum, abs, sq_lo, sq_hi of a cell (csrc/mutagenesis.hip: PW_*)
PROFILE_SCALE = 30                  # q = rne(delta * 2^30)
PROFILE_LIMIT = 256.0               # a term is valid when delta is finite and |delta| < 256
PROFILE_MAX_SITES = 1 << 24         # per call: |q| < 2^38 and at most 2^24 terms per cell keep every word below 2^63
PROFILE_NONFINITE, PROFILE_RANGE = 1, 2     # bits of status[0]; status[1] / status[2] count the terms of either kind


def mutagenesis_profile_host(ref_logp, var_logp, ref_symbols, group, first, table, status=None):
    """The numpy twin of ``mural_mutagenesis_profile_window``: adds the terms of the ids [first, first + count) into `table`, uint64
    (n_groups, W, 4, 3, n_class, 5) indexed [group, column, reference symbol, a, class, word] in place (and the invalid terms into
    `status`, uint64 (3,)).  `group`: int32 (n_sites,) or None for group 0 everywhere."""
    ref_logp, var_logp = np.asarray(ref_logp, np.float32), np.asarray(var_logp, np.float32)
    ref_symbols = np.asarray(ref_symbols, np.uint8)
    n, W = ref_symbols.shape
    n_groups, n_class = table.shape[0], ref_logp.shape[1]
    if table.dtype != np.uint64 or table.shape != (n_groups, W, 4, 3, n_class, PROFILE_WORDS) or not table.flags.c_contiguous:
        raise ValueError(f"mutagenesis_profile: table must be uint64 (n_groups, {W}, 4, 3, {n_class}, {PROFILE_WORDS})")
    if n > PROFILE_MAX_SITES:
        raise ValueError("mutagenesis_profile: at most 2^24 sites per call")
    if first < 0 or first + len(var_logp) > n * W * 3:
        raise ValueError("mutagenesis_profile: ids [first, first + count) must lie in [0, n_sites * W * 3)")
    site, j, a = _ids(first, len(var_logp), W)
    ref = ref_symbols[site, j].astype(np.int64)
    grp = np.zeros(n, np.int64) if group is None else np.asarray(group, np.int32).astype(np.int64)
    g = grp[site]
    row = (ref < 4) & (g >= 0) & (g < n_groups)
    with np.errstate(invalid="ignore", over="ignore"):
        delta = var_logp - ref_logp[site]                                 # (count, n_class): the reduce's float32 subtraction
        finite = np.isfinite(delta)
        small = finite & (np.abs(delta) < np.float32(PROFILE_LIMIT))
    term = row[:, None] & small
    if status is not None:
        nonfinite, out_of_range = int((row[:, None] & ~finite).sum()), int((row[:, None] & finite & ~small).sum())
        status[0] |= np.uint64((PROFILE_NONFINITE if nonfinite else 0) | (PROFILE_RANGE if out_of_range else 0))
        status[1] += np.uint64(nonfinite)
        status[2] += np.uint64(out_of_range)
    k, c = np.nonzero(term)
    # float32 -> float64 is exact; times 2^30 only moves the exponent (|delta| < 2^8 and the smallest float32 is 2^-149: no overflow, no
    # underflow in float64), so the product is delta * 2^30 itself and rint (to nearest, ties to even) is the one rounding of q
    q = np.rint(delta[k, c].astype(np.float64) * float(1 << PROFILE_SCALE)).astype(np.int64)
    mag = np.abs(q).astype(np.uint64)                                     # < 2^38: mag = hi * 2^20 + lo, mag^2 = hi^2 2^40 + (2 hi lo 2^20 + lo^2)
    hi, lo = mag >> np.uint64(20), mag & np.uint64((1 << 20) - 1)
    low = ((hi * lo) << np.uint64(21)) + lo * lo                          # < 2^60
    cell = ((((g[k] * W + j[k]) * 4 + ref[k]) * 3 + a[k]) * n_class + c) * PROFILE_WORDS
    flat = table.reshape(-1)
    words = (np.ones(len(q), np.uint64), q.view(np.uint64), mag, low & np.uint64((1 << 40) - 1), hi * hi + (low >> np.uint64(40)))
    for w, x in enumerate(words):
        np.add.at(flat, cell + w, x)
    return table


def log_softmax_host(scores):
    """The float64 twin of ``mural_scores_log_softmax``: s - (max + log sum exp(s - max)) per row."""
    s = np.asarray(scores, np.float64)
    mx = s.max(axis=1, keepdims=True)
    return s - (mx + np.log(np.exp(s - mx).sum(axis=1, keepdims=True)))


# ----------------------------------------------------------------------------------------------------------------------------------
# device entry points
# ----------------------------------------------------------------------------------------------------------------------------------
def _encode_subst_into(genome, pos, strand, sub_pos, sub_base, radius, local_radius, local_order, symbols, cat_x):
    g = genome.as_struct()
    with torch.cuda.device(genome.device):
        _lib.check(_lib.lib().mural_encode_subst_windows(
            C.byref(g), pos.data_ptr(), strand.data_ptr(), sub_pos.data_ptr(), sub_base.data_ptr(), pos.shape[0], int(radius),
            int(local_radius), int(local_order), None if symbols is None else symbols.data_ptr(),
            None if cat_x is None else cat_x.data_ptr(), _lib.current_stream_ptr(genome.device)))


def _encode_subst_symbols_into(genome, pos, strand, sub_pos, sub_base, radius, indel, symbols):
    g = genome.as_struct()
    with torch.cuda.device(genome.device):
        _lib.check(_lib.lib().mural_encode_subst_symbols(
            C.byref(g), pos.data_ptr(), strand.data_ptr(), sub_pos.data_ptr(), sub_base.data_ptr(), pos.shape[0], int(radius), int(indel),
            symbols.data_ptr(), _lib.current_stream_ptr(genome.device)))


def encode_subst_windows(genome, pos, strand, sub_pos, sub_base, radius, local_radius=None, local_order=None, model_type="snv"):
    """``PackedGenome.encode_subst_windows``: (symbols uint8 (n, 2 * radius + 1), cat_x int64 (n, 2 * local_radius + 1 - (local_order - 1)))
    of one row per (site, substitution), bit for bit ``encode_symbols`` / ``encode_kmer`` on the genome with that base replaced.  `sub_pos`
    is a '+'-strand position, `sub_base` a '+'-strand base 0..3 or 255 for none.  ``model_type="indel"``: (symbols uint8 (n, 2 * radius),
    None) of the INDEL window; the local arguments are not read."""
    if model_type not in ("snv", "indel"):
        raise ValueError(f"model_type {model_type} not supported!")
    pos, strand = genome._prep(pos, strand)
    sub_pos = torch.as_tensor(sub_pos, dtype=torch.int64, device=genome.device).contiguous()
    sub_base = torch.as_tensor(sub_base, dtype=torch.uint8, device=genome.device).contiguous()
    if sub_pos.shape != pos.shape or sub_base.shape != pos.shape:
        raise ValueError("sub_pos and sub_base must be 1-D and as long as pos")
    n = pos.shape[0]
    if model_type == "indel":
        symbols = torch.empty((n, 2 * radius), dtype=torch.uint8, device=genome.device)
        _encode_subst_symbols_into(genome, pos, strand, sub_pos, sub_base, radius, 1, symbols)
        return symbols, None
    if local_radius is None or local_order is None:
        raise ValueError("encode_subst_windows: the SNV windows need local_radius and local_order")
    symbols = torch.empty((n, 2 * radius + 1), dtype=torch.uint8, device=genome.device)
    cat_x = torch.empty((n, 2 * local_radius + 1 - (local_order - 1)), dtype=torch.int64, device=genome.device)
    _encode_subst_into(genome, pos, strand, sub_pos, sub_base, radius, local_radius, local_order, symbols, cat_x)
    return symbols, cat_x


def mutagenesis_rows(genome, pos, strand, radius, first, count, model_type="snv"):
    """``mural_mutagenesis_rows`` (``.._window`` for ``model_type="indel"``) on the device: (row_pos, row_strand, sub_pos, sub_base) of the
    variant ids [first, first + count)."""
    if model_type not in ("snv", "indel"):
        raise ValueError(f"model_type {model_type} not supported!")
    pos, strand = genome._prep(pos, strand)
    dev = genome.device
    out = (torch.empty(count, dtype=torch.int64, device=dev), torch.empty(count, dtype=torch.uint8, device=dev),
           torch.empty(count, dtype=torch.int64, device=dev), torch.empty(count, dtype=torch.uint8, device=dev))
    g = genome.as_struct()
    with torch.cuda.device(dev):
        if model_type == "indel":
            _lib.check(_lib.lib().mural_mutagenesis_rows_window(C.byref(g), pos.data_ptr(), strand.data_ptr(), pos.shape[0], int(radius), 1,
                                                               int(first), int(count), *[t.data_ptr() for t in out],
                                                               _lib.current_stream_ptr(dev)))
        else:
            _lib.check(_lib.lib().mural_mutagenesis_rows(C.byref(g), pos.data_ptr(), strand.data_ptr(), pos.shape[0], int(radius), int(first),
                                                        int(count), *[t.data_ptr() for t in out], _lib.current_stream_ptr(dev)))
    return out


def mutagenesis_reduce(ref_logp, var_logp, ref_symbols, first, delta, logp_map=None):
    """``mural_mutagenesis_reduce`` on the device: var_logp (count, n_class) of the ids [first, first + count) into `delta` (n_sites, W, 4,
    n_class) in place (and into `logp_map`).  Contiguous float32 / uint8 device tensors.  An odd W is the SNV entry (W = 2 * radius + 1),
    an even one ``mural_mutagenesis_reduce_window``: the same kernel."""
    n, W = ref_symbols.shape
    n_class = ref_logp.shape[1]
    tensors = [(ref_logp, torch.float32, (n, n_class)), (var_logp, torch.float32, (var_logp.shape[0], n_class)),
               (ref_symbols, torch.uint8, (n, W)), (delta, torch.float32, (n, W, 4, n_class))]
    if logp_map is not None:
        tensors.append((logp_map, torch.float32, (n, W, 4, n_class)))
    for t, dt, shape in tensors:
        _lib.require_cuda(t, "mutagenesis_reduce input")
        if t.dtype != dt or tuple(t.shape) != shape or not t.is_contiguous():
            raise ValueError(f"mutagenesis_reduce: expected a contiguous {dt} tensor of shape {shape}, got {t.dtype} {tuple(t.shape)}")
    if W < 1:
        raise ValueError("mutagenesis_reduce: ref_symbols must be (n_sites, W) with W >= 1")
    dev = delta.device
    with torch.cuda.device(dev):
        if W % 2 == 0:
            _lib.check(_lib.lib().mural_mutagenesis_reduce_window(ref_logp.data_ptr(), var_logp.data_ptr(), ref_symbols.data_ptr(), n, W, n_class,
                                                                 int(first), var_logp.shape[0], delta.data_ptr(),
                                                                 None if logp_map is None else logp_map.data_ptr(),
                                                                 _lib.current_stream_ptr(dev)))
            return delta
        _lib.check(_lib.lib().mural_mutagenesis_reduce(ref_logp.data_ptr(), var_logp.data_ptr(), ref_symbols.data_ptr(), n, (W - 1) // 2,
                                                      n_class, int(first), var_logp.shape[0], delta.data_ptr(),
                                                      None if logp_map is None else logp_map.data_ptr(), _lib.current_stream_ptr(dev)))
    return delta


def scores_log_softmax(scores):
    """``mural_scores_log_softmax`` on the device: float32 (n, n_class) scores -> the log-probabilities of softmax(scores), a new tensor.
    One thread per row: a row's bits do not depend on the rows it shares the call with."""
    _lib.require_cuda(scores, "scores")
    if scores.dtype != torch.float32 or scores.dim() != 2 or scores.shape[1] < 1 or not scores.is_contiguous():
        raise ValueError(f"scores_log_softmax: expected a contiguous float32 (n, n_class) tensor, got {scores.dtype} {tuple(scores.shape)}")
    out = torch.empty_like(scores)
    with torch.cuda.device(scores.device):
        _lib.check(_lib.lib().mural_scores_log_softmax(scores.data_ptr(), scores.shape[0], scores.shape[1], out.data_ptr(),
                                                      _lib.current_stream_ptr(scores.device)))
    return out


def _is_indel(model):
    from .model.model_indel import UNet_Small
    return isinstance(model, UNet_Small)


def _require_indel(model, radius):
    """distal radius of a UNet_Small the symbols entry serves; RuntimeError that names the reason otherwise."""
    if model.training:
        raise RuntimeError("internal: the fused inference kernels serve eval mode only")
    if next(model.parameters()).device.type != "cuda":
        raise RuntimeError("mural_amd models run on a HIP device only: call model.to('cuda') first")
    if radius is None:
        radius = getattr(model, "distal_radius", None)
    if radius is None or int(radius) < 1:
        raise ValueError("mutagenesis of the INDEL model needs distal_radius >= 1 (UNet_Small does not carry its window length)")
    return int(radius)


def _require_model(model, local_radius, local_order):
    """(distal radius, local radius) of a model the symbols entry serves; RuntimeError that names the reason otherwise."""
    model_no = getattr(model, "model_no", -1)
    if model_no == 0:
        raise RuntimeError("mutagenesis needs a model with a distal window: Network0 has none (it reads the local k-mers only)")
    if model_no not in (1, 2):
        raise RuntimeError(f"mutagenesis serves the SNV models Network1 / Network2, not {type(model).__name__}")
    if model.training:
        raise RuntimeError("internal: the fused inference kernels serve eval mode only")
    if next(model.parameters()).device.type != "cuda":
        raise RuntimeError("mural_amd models run on a HIP device only: call model.to('cuda') first")
    if not model.symbols_entry_ok():
        if model._front_ok():
            raise RuntimeError("mutagenesis runs through forward_symbols, which this model does not have: its window is so long that only "
                               "the front of the large tower is fused (front-only long windows)")
        raise RuntimeError("mutagenesis runs through forward_symbols, which this model does not have: its shape evaluates through the "
                           "per-layer path (CNN_out_channels != 32, CNN_kernel_size != 3 or a window too long for LDS)")
    if local_radius is None:
        local_radius = (getattr(model, "no_of_cat", 1) + local_order - 2) // 2
    return (model.seq_len - 1) // 2, int(local_radius)


def _sites(genome, model, pos, strand):
    pos = _lib.require_cuda(torch.as_tensor(pos), "pos").to(torch.int64).contiguous()
    strand = _lib.require_cuda(torch.as_tensor(strand), "strand").to(torch.uint8).contiguous()
    if pos.dim() != 1 or pos.shape != strand.shape:
        raise ValueError("pos and strand must be 1-D and of equal length")
    dev = next(model.parameters()).device
    if genome.packed2.device != dev or pos.device != dev or strand.device != dev:
        raise RuntimeError(f"genome ({genome.packed2.device}), sites ({pos.device}) and model ({dev}) must live on one HIP device")
    return pos, strand


class MutagenesisMap:
    """The result of ``saturation_mutagenesis``.  Device tensors: ``delta`` float32 (n, W, 4, n_class), indexed [site, window column,
    alternative base in window orientation, class] -- +0.0 at the reference base, NaN in all four entries of a column whose reference
    symbol is not A/C/G/T; ``ref_logp`` (n, n_class); ``ref_symbols`` uint8 (n, W), strand-oriented MURAL_SYM_* codes; ``var_logp`` (the
    variants' log-probabilities in the layout of ``delta``, ref_logp at the reference base) when asked for, else None."""

    __slots__ = ("delta", "ref_logp", "ref_symbols", "var_logp", "pos", "strand", "radius", "model_type")

    def __init__(self, delta, ref_logp, ref_symbols, var_logp, pos, strand, radius, model_type="snv"):
        self.delta, self.ref_logp, self.ref_symbols, self.var_logp = delta, ref_logp, ref_symbols, var_logp
        self.pos, self.strand, self.radius, self.model_type = pos, strand, radius, model_type

    def genomic_positions(self):
        """int64 (n, W): the '+'-strand position of every window column (SNV: pos + (j - R) on '+', pos - (j - R) on '-'; INDEL, W = 2 R:
        pos - R + 1 + j on '+', pos + R - j on '-'; may lie outside the record, where the column is N)."""
        off0, W = _window(self.radius, self.model_type)
        j = torch.arange(W, dtype=torch.int64, device=self.pos.device)
        neg = self.strand.to(torch.bool)
        return self.pos[:, None] + off0 + torch.where(neg[:, None], W - 1 - j[None, :], j[None, :])

    def importance(self):
        """float32 (n, W): the largest |delta| over alternatives and classes; NaN where the column has no substitutions."""
        mag = self.delta.abs().flatten(2)
        nan = torch.isnan(mag)
        best = torch.where(nan, torch.full_like(mag, -1.0), mag).amax(dim=2)
        return torch.where(nan.all(dim=2), torch.full_like(best, float("nan")), best)


def saturation_mutagenesis(model, genome, pos, strand, local_radius=None, local_order=3, chunk_windows=1 << 17, return_logp=False,
                           timings=None, distal_radius=None):
    """The saturation-mutagenesis map of the sites `pos` / `strand` (device int64 / uint8, 1 = '-') of a ``PackedGenome``: a
    ``MutagenesisMap``.  Every chunk of `chunk_windows` variant ids runs enumerate -> encode -> ``forward_symbols`` -> reduce; the row
    buffers are allocated once.  The map is bit-identical for every `chunk_windows`.  Serves Network1 / Network2 in eval mode whose
    ``symbols_entry_ok()``; anything else raises RuntimeError with the reason.  `timings`: an optional dict that receives the device
    time of the chunks' three phases from HIP events (``rows_encode_ms``, ``forward_ms``, ``reduce_ms``; it synchronises at the end).

    A ``UNet_Small`` in eval mode gives the map of the INDEL window: `distal_radius` R is required (or ``model.distal_radius``), W = 2 R,
    `local_radius` / `local_order` are ignored, and the log-probabilities are the log-softmax of ``forward_symbols``' scores (counted in
    ``forward_ms``).  The INDEL forward picks kernels by the size of a call, so its map is reproducible for one `chunk_windows` and
    agrees across values of it within the forward's own accuracy, not bit for bit."""
    out = {}

    def begin(ref_logp, ref_symbols, pos, strand, R, model_type):
        n, W = ref_symbols.shape
        # every element is written by the reduce (one writer each): no fill
        delta = torch.empty((n, W, 4, ref_logp.shape[1]), dtype=torch.float32, device=pos.device)
        logp_map = torch.empty_like(delta) if return_logp else None
        out["map"] = MutagenesisMap(delta, ref_logp, ref_symbols, logp_map, pos, strand, R, model_type)
        lib, n_class = _lib.lib(), ref_logp.shape[1]

        def reduce(var, first, m, stream):
            _lib.check(lib.mural_mutagenesis_reduce_window(ref_logp.data_ptr(), var.data_ptr(), ref_symbols.data_ptr(), n, W, n_class, first,
                                                           m, delta.data_ptr(), logp_map.data_ptr() if return_logp else None, stream))
        return reduce

    _mutagenesis_chunks(model, genome, pos, strand, local_radius, local_order, chunk_windows, distal_radius, timings, begin)
    return out["map"]


def _mutagenesis_chunks(model, genome, pos, strand, local_radius, local_order, chunk_windows, distal_radius, timings, begin):
    """The chunk loop ``saturation_mutagenesis`` and ``mutagenesis_profile`` share: checks the model and the sites, predicts the
    unchanged windows, then runs enumerate -> encode -> ``forward_symbols`` -> reduce per chunk of `chunk_windows` variant ids with row
    buffers allocated once.  ``begin(ref_logp, ref_symbols, pos, strand, R, model_type)`` is called once, before the first chunk, and
    returns ``reduce(var_logp, first, m, stream)``, which consumes a chunk's log-probabilities (the third phase of `timings`)."""
    indel = _is_indel(model)
    if indel:
        R, r = _require_indel(model, distal_radius), 0
    else:
        R, r = _require_model(model, local_radius, local_order)
    pos, strand = _sites(genome, model, pos, strand)
    if chunk_windows < 1:
        raise ValueError("chunk_windows must be >= 1")
    model_type = "indel" if indel else "snv"
    dev, n, W, n_class = pos.device, pos.shape[0], _window(R, model_type)[1], model.n_class
    with_cat = not indel and model.model_no == 2

    def forward(cat, sym):
        return scores_log_softmax(model.forward_symbols(sym)) if indel else model.forward_symbols(cat, sym)

    with torch.no_grad(), torch.cuda.device(dev):
        ref_symbols = genome.encode_symbols(pos, strand, R, model_type).sym
        ref_cat = genome.encode_kmer(pos, strand, r, local_order) if with_cat else None
        ref_logp = forward(ref_cat, ref_symbols) if n else torch.empty((0, n_class), dtype=torch.float32, device=dev)
        reduce = begin(ref_logp, ref_symbols, pos, strand, R, model_type)
        total = n * W * 3
        cap = min(int(chunk_windows), max(total, 1))
        row_pos = torch.empty(cap, dtype=torch.int64, device=dev)
        row_strand = torch.empty(cap, dtype=torch.uint8, device=dev)
        sub_pos = torch.empty(cap, dtype=torch.int64, device=dev)
        sub_base = torch.empty(cap, dtype=torch.uint8, device=dev)
        symbols = torch.empty((cap, W), dtype=torch.uint8, device=dev)
        cat_x = torch.empty((cap, 2 * r + 1 - (local_order - 1)), dtype=torch.int64, device=dev) if with_cat else None
        lib, g, stream = _lib.lib(), genome.as_struct(dev), _lib.current_stream_ptr(dev)
        marks = []

        def mark():
            if timings is not None:
                marks.append(torch.cuda.Event(enable_timing=True))
                marks[-1].record()

        for first in range(0, total, cap):
            m = min(cap, total - first)
            mark()
            _lib.check(lib.mural_mutagenesis_rows_window(C.byref(g), pos.data_ptr(), strand.data_ptr(), n, R, int(indel), first, m,
                                                         row_pos.data_ptr(), row_strand.data_ptr(), sub_pos.data_ptr(), sub_base.data_ptr(),
                                                         stream))
            if indel:
                _lib.check(lib.mural_encode_subst_symbols(C.byref(g), row_pos.data_ptr(), row_strand.data_ptr(), sub_pos.data_ptr(),
                                                          sub_base.data_ptr(), m, R, 1, symbols.data_ptr(), stream))
            else:
                _lib.check(lib.mural_encode_subst_windows(C.byref(g), row_pos.data_ptr(), row_strand.data_ptr(), sub_pos.data_ptr(),
                                                          sub_base.data_ptr(), m, R, r, int(local_order), symbols.data_ptr(),
                                                          cat_x.data_ptr() if with_cat else None, stream))
            mark()
            var = forward(cat_x[:m] if with_cat else None, symbols[:m])
            mark()
            reduce(var, first, m, stream)
            mark()
        if timings is not None:
            torch.cuda.synchronize(dev)
            for k, name in enumerate(("rows_encode_ms", "forward_ms", "reduce_ms")):
                timings[name] = timings.get(name, 0.0) + sum(marks[c + k].elapsed_time(marks[c + k + 1]) for c in range(0, len(marks), 4))


def mutagenesis_profile_window(ref_logp, var_logp, ref_symbols, group, first, table, status):
    """``mural_mutagenesis_profile_window`` on the device: the terms of the ids [first, first + count) added into `table` (int64 bit
    patterns of the uint64 words, (n_groups, W, 4, 3, n_class, 5)) and `status` (int64 (3,)) in place.  Contiguous device tensors; `group`
    int32 (n_sites,) or None."""
    n, W = ref_symbols.shape
    n_class, n_groups = ref_logp.shape[1], table.shape[0]
    tensors = [(ref_logp, torch.float32, (n, n_class)), (var_logp, torch.float32, (var_logp.shape[0], n_class)),
               (ref_symbols, torch.uint8, (n, W)), (table, torch.int64, (n_groups, W, 4, 3, n_class, PROFILE_WORDS)),
               (status, torch.int64, (3,))]
    if group is not None:
        tensors.append((group, torch.int32, (n,)))
    for t, dt, shape in tensors:
        _lib.require_cuda(t, "mutagenesis_profile input")
        if t.dtype != dt or tuple(t.shape) != shape or not t.is_contiguous():
            raise ValueError(f"mutagenesis_profile: expected a contiguous {dt} tensor of shape {shape}, got {t.dtype} {tuple(t.shape)}")
    dev = table.device
    with torch.cuda.device(dev):
        _lib.check(_lib.lib().mural_mutagenesis_profile_window(ref_logp.data_ptr(), var_logp.data_ptr(), ref_symbols.data_ptr(),
                                                              None if group is None else group.data_ptr(), n, W, n_class, n_groups,
                                                              int(first), var_logp.shape[0], table.data_ptr(), status.data_ptr(),
                                                              _lib.current_stream_ptr(dev)))
    return table


class MutagenesisProfile:
    """Saturation-mutagenesis maps reduced over sites: exact integer sums of q = rne(delta * 2^30) per [group,
    window column, reference base, alternative, class].  ``words`` is one int64 tensor (the bit patterns of the uint64 words) that holds
    the table and, in its last three entries, the status counters; ``table`` (n_groups, W, 4, 3, n_class, 5) and ``status`` (3,) are views
    of it.  Tables add: across chunks, calls (``into=``), profiles (``merge``) and ranks (``all_reduce_``), to the same integers in any
    order.  The float64 statistics are computed on the host from the integers.  A cell's words are sized for 2^24 terms; whoever adds
    more than that many sites into one profile watches ``counts()``."""

    __slots__ = ("words", "radius", "model_type", "n_class", "n_groups")

    def __init__(self, words, radius, model_type, n_class, n_groups):
        self.words, self.radius, self.model_type, self.n_class, self.n_groups = words, int(radius), model_type, int(n_class), int(n_groups)
        if words.dtype != torch.int64 or words.dim() != 1 or words.shape[0] != self._cells() * PROFILE_WORDS + 3 or not words.is_contiguous():
            raise ValueError(f"MutagenesisProfile: words must be a contiguous int64 tensor of {self._cells() * PROFILE_WORDS + 3} entries")

    def _cells(self):
        return self.n_groups * self.width * 12 * self.n_class

    @classmethod
    def zeros(cls, radius, model_type, n_class, n_groups=1, device="cpu"):
        W = _window(radius, model_type)[1]
        if n_class < 1 or n_groups < 1:
            raise ValueError("MutagenesisProfile: n_class and n_groups must be >= 1")
        return cls(torch.zeros(n_groups * W * 12 * n_class * PROFILE_WORDS + 3, dtype=torch.int64, device=device), radius, model_type,
                   n_class, n_groups)

    @property
    def width(self):
        return _window(self.radius, self.model_type)[1]

    @property
    def table(self):
        return self.words[:-3].view(self.n_groups, self.width, 4, 3, self.n_class, PROFILE_WORDS)

    @property
    def status(self):
        return self.words[-3:]

    def table_host(self):
        """The table as a uint64 numpy array (a copy unless the profile lives on the host, where it shares memory: the twin adds in place)."""
        return self.table.cpu().numpy().view(np.uint64)

    def status_host(self):
        """(bits, non-finite terms, finite terms of |delta| >= 256) as Python ints."""
        return tuple(int(x) for x in self.status.cpu().numpy().view(np.uint64))

    def offsets(self):
        """int64 (W,): the columns' distance from the site in window orientation.  SNV: -R .. R.  INDEL (W = 2 R): -R + 1 .. R, the
        distances on '+'; a '-' site sits one column further right, its distances are these minus one."""
        return np.arange(self.width, dtype=np.int64) + _window(self.radius, self.model_type)[0]

    # -- statistics: float64 (n_groups, W, 4, 4, n_class) indexed [group, column, ref, alt base in window orientation, class] ---------
    def _folded(self):
        """(n, sum, abs, sq) as float64 in the (G, W, 4, 4, C) layout, zero where nothing was added, and the mask of empty entries."""
        t = self.table_host()
        G, W, C = self.n_groups, self.width, self.n_class
        words = (t[..., 0].astype(np.float64), t[..., 1].view(np.int64).astype(np.float64), t[..., 2].astype(np.float64),
                 t[..., 4].astype(np.float64) * float(1 << 40) + t[..., 3].astype(np.float64))
        out = [np.zeros((G, W, 4, 4, C), np.float64) for _ in words]
        for ref in range(4):
            for a in range(3):
                for o, w in zip(out, words):
                    o[:, :, ref, a + (a >= ref)] = w[:, :, ref, a]
        return out, out[0] == 0

    def _stat(self, value):
        (n, s, ab, sq), empty = self._folded()
        with np.errstate(invalid="ignore", divide="ignore"):
            return np.where(empty, np.nan, value(n, s, ab, sq))

    def counts(self):
        return self._stat(lambda n, s, ab, sq: n)

    def mean(self):
        return self._stat(lambda n, s, ab, sq: s / n / float(1 << PROFILE_SCALE))

    def mean_abs(self):
        return self._stat(lambda n, s, ab, sq: ab / n / float(1 << PROFILE_SCALE))

    def rms(self):
        return self._stat(lambda n, s, ab, sq: np.sqrt(sq / n) / float(1 << PROFILE_SCALE))

    def by_distance(self):
        """float64 (n_groups, W, n_class): mean |delta| over reference bases and alternatives, weighted by their counts, per window column
        (``offsets()`` gives the columns' signed distance from the focal base); NaN where a column received nothing."""
        (n, _, ab, _), _ = self._folded()
        n, ab = n.sum(axis=(2, 3)), ab.sum(axis=(2, 3))
        with np.errstate(invalid="ignore", divide="ignore"):
            return np.where(n == 0, np.nan, ab / n / float(1 << PROFILE_SCALE))

    # -- adding tables ------------------------------------------------------------------------------------------------------------------
    def _require_same(self, other, what):
        mine = (self.radius, self.model_type, self.n_class, self.n_groups)
        theirs = (other.radius, other.model_type, other.n_class, other.n_groups)
        if mine != theirs:
            raise ValueError(f"{what}: profiles of (radius, model_type, n_class, n_groups) = {mine} and {theirs} do not add")

    def require_continues(self, radius, model_type, n_class, n_groups, device):
        """ValueError unless a run of this window, class count and device can add into this profile (``mutagenesis_profile(.., into=)``;
        n_groups = 1, the default, stands for the profile's own)."""
        if (self.radius, self.model_type, self.n_class) != (radius, model_type, n_class) or self.words.device != torch.device(device):
            raise ValueError(f"into: a profile of (radius, model_type, n_class) = {(self.radius, self.model_type, self.n_class)} on "
                             f"{self.words.device} cannot continue with {(radius, model_type, n_class)} on {device}")
        if n_groups not in (1, self.n_groups):
            raise ValueError(f"into: the profile has {self.n_groups} groups, n_groups = {n_groups} was asked for")

    def merge(self, other):
        """Adds `other`'s integers and status counters to this profile in place; returns self."""
        if not isinstance(other, MutagenesisProfile):
            raise TypeError("merge: a MutagenesisProfile is needed")
        self._require_same(other, "merge")
        theirs = other.words.to(self.words.device)
        self.words[:-3] += theirs[:-3]                       # int64 adds wrap as the uint64 adds do
        self.words[-3] |= theirs[-3]
        self.words[-2:] += theirs[-2:]
        return self

    __iadd__ = merge

    def all_reduce_(self, process_group=None):
        """One SUM all-reduce of ``words`` (table and counters) viewed as int64 -- wraparound is the two's-complement sum, so the result is
        the uint64 sum -- after which the status bits are those of the summed counters.  Returns self."""
        import torch.distributed as dist
        dist.all_reduce(self.words, op=dist.ReduceOp.SUM, group=process_group)
        self.words[-3] = (self.words[-2] != 0).to(torch.int64) * PROFILE_NONFINITE + (self.words[-1] != 0).to(torch.int64) * PROFILE_RANGE
        return self

    def save(self, path):
        """The integers and the metadata as one .npz (``load`` reads it back)."""
        with open(path, "wb") as fh:
            np.savez(fh, table=self.table_host(), status=self.status.cpu().numpy().view(np.uint64), radius=np.int64(self.radius),
                     model_type=np.array(self.model_type), n_class=np.int64(self.n_class), n_groups=np.int64(self.n_groups))

    @classmethod
    def load(cls, path, device="cpu"):
        with np.load(path, allow_pickle=False) as z:
            prof = cls.zeros(int(z["radius"]), str(z["model_type"]), int(z["n_class"]), int(z["n_groups"]))
            table, status = z["table"], z["status"]
        if table.dtype != np.uint64 or table.shape != tuple(prof.table.shape) or status.dtype != np.uint64 or status.shape != (3,):
            raise ValueError(f"{path}: not a mutagenesis profile (table {table.dtype} {table.shape}, status {status.dtype} {status.shape})")
        prof.words[:-3] = torch.from_numpy(table.view(np.int64).reshape(-1))
        prof.words[-3:] = torch.from_numpy(status.view(np.int64))
        prof.words = prof.words.to(device)
        return prof


def mutagenesis_profile(model, genome, pos, strand, groups=None, n_groups=1, local_radius=None, local_order=3, chunk_windows=1 << 17,
                        distal_radius=None, into=None, timings=None):
    """The saturation-mutagenesis maps of the sites reduced in flight into a ``MutagenesisProfile``: the chunk loop of
    ``saturation_mutagenesis`` (same models, same refusals, same `timings`) with ``mural_mutagenesis_profile_window`` in the place of the
    reduce, so no map is written.  `groups`: int32 group id per site (device tensor, or anything ``torch.as_tensor`` takes), None for one
    group; a site whose id lies outside [0, n_groups) adds nothing.  `into` continues an existing profile (its n_groups holds; shapes and
    model type must match, ValueError otherwise) and is returned.  For the SNV models the table equals, bit for bit, the twin applied to
    the map's ``delta``, and does not depend on `chunk_windows`, on the order of the sites or on how they are split over calls; a
    ``UNet_Small``'s is reproducible per `chunk_windows` only, as its map is."""
    out = {}

    def begin(ref_logp, ref_symbols, pos, strand, R, model_type):
        n, n_class, dev = pos.shape[0], ref_logp.shape[1], pos.device
        if n > PROFILE_MAX_SITES:
            raise ValueError(f"mutagenesis_profile: {n} sites in one call; at most 2^24 are taken, because a cell's integer sums are sized "
                             "for 2^24 terms (|q| < 2^38 each): split the sites over calls joined by into=")
        if into is not None:
            if not isinstance(into, MutagenesisProfile):
                raise TypeError("into must be a MutagenesisProfile")
            into.require_continues(R, model_type, n_class, n_groups, dev)
            prof = into
        else:
            prof = MutagenesisProfile.zeros(R, model_type, n_class, n_groups, dev)
        group = None
        if groups is not None:
            group = torch.as_tensor(groups).to(dev)
            if group.shape != pos.shape or group.dtype.is_floating_point:
                raise ValueError("groups must hold one integer id per site")
            if group.dtype != torch.int32:             # ids that int32 cannot hold are outside every [0, n_groups)
                group = torch.where((group < 0) | (group >= prof.n_groups), torch.full_like(group, -1), group).to(torch.int32)
            group = group.contiguous()
        out["profile"] = prof
        table, status = prof.table, prof.status
        lib, W = _lib.lib(), prof.width

        def reduce(var, first, m, stream):
            _lib.check(lib.mural_mutagenesis_profile_window(ref_logp.data_ptr(), var.data_ptr(), ref_symbols.data_ptr(),
                                                            None if group is None else group.data_ptr(), n, W, n_class, prof.n_groups,
                                                            first, m, table.data_ptr(), status.data_ptr(), stream))
        return reduce

    _mutagenesis_chunks(model, genome, pos, strand, local_radius, local_order, chunk_windows, distal_radius, timings, begin)
    return out["profile"]


def footprint_offsets(radius, model_type="snv", device=None):
    """int64 offsets d of ``variant_footprint``'s second axis: [-R, R] for the SNV models, [-R, R - 1] for the INDEL model."""
    if model_type not in ("snv", "indel"):
        raise ValueError(f"model_type {model_type} not supported!")
    return torch.arange(-radius, radius + (1 if model_type == "snv" else 0), dtype=torch.int64, device=device)


def variant_footprint(model, genome, var_pos, var_base, strand, local_radius=None, local_order=3, chunk_windows=1 << 17,
                      distal_radius=None):
    """What each variant does to the sites around it: for variant i (`var_pos` '+'-strand position, `var_base` '+'-strand base 0..3) the
    change in log-probability of every neighbouring site var_pos + d, d in [-R, R], read on `strand` (uint8 per variant, 1 = '-'), as
    ``(delta float32 (m, W, n_class), focal uint8 (m, W))``: entry [i, d + R].  d = 0 and neighbours outside the chromosome are NaN.
    `focal` is each neighbour's reference focal symbol on `strand` (MURAL_SYM_*; N outside the chromosome), for masking to the model's
    site class.  Rows go through the same encoder and ``forward_symbols`` as ``saturation_mutagenesis``: entry (i, d) equals, bit for
    bit, that map's entry of site var_pos + d at the column and alternative that name the same genomic substitution.

    A ``UNet_Small`` (`distal_radius` as in ``saturation_mutagenesis``): the neighbours are the sites whose INDEL window holds the variant,
    d in [-R, R - 1], entry [i, d + R] of ``(delta (m, 2 R, n_class), focal (m, 2 R))``.  d = 0 is a live entry (a substitution at the
    focal base does not remove an INDEL site); only neighbours outside the chromosome are NaN.  Entries equal the map's where both ran
    calls of the same size, and agree within the forward's accuracy otherwise.  ``footprint_offsets`` gives d."""
    indel = _is_indel(model)
    if indel:
        R, r = _require_indel(model, distal_radius), 0
    else:
        R, r = _require_model(model, local_radius, local_order)
    var_pos, strand = _sites(genome, model, var_pos, strand)
    var_base = _lib.require_cuda(torch.as_tensor(var_base), "var_base").to(torch.uint8).contiguous()
    if var_base.shape != var_pos.shape:
        raise ValueError("var_base must be as long as var_pos")
    if chunk_windows < 1:
        raise ValueError("chunk_windows must be >= 1")
    dev, m, W, n_class = var_pos.device, var_pos.shape[0], 2 * R if indel else 2 * R + 1, model.n_class
    with_cat = not indel and model.model_no == 2
    with torch.no_grad(), torch.cuda.device(dev):
        d = footprint_offsets(R, "indel" if indel else "snv", dev)
        row_pos = (var_pos[:, None] + d[None, :]).reshape(-1).contiguous()
        row_strand = strand[:, None].expand(m, W).reshape(-1).contiguous()
        sub_pos = var_pos[:, None].expand(m, W).reshape(-1).contiguous()
        sub_base = var_base[:, None].expand(m, W).reshape(-1).contiguous()
        none = torch.full_like(sub_base, NO_SUBST)
        total = m * W
        cap = min(int(chunk_windows), max(total, 1))
        symbols = torch.empty((cap, W), dtype=torch.uint8, device=dev)
        cat_x = torch.empty((cap, 2 * r + 1 - (local_order - 1)), dtype=torch.int64, device=dev) if with_cat else None
        delta = torch.empty((total, n_class), dtype=torch.float32, device=dev)
        focal = torch.empty(total, dtype=torch.uint8, device=dev)
        for c0 in range(0, total, cap):
            k = min(cap, total - c0)
            rows = slice(c0, c0 + k)
            logp = []
            for base in (sub_base, none):
                if indel:
                    _encode_subst_symbols_into(genome, row_pos[rows], row_strand[rows], sub_pos[rows], base[rows], R, 1, symbols)
                    logp.append(scores_log_softmax(model.forward_symbols(symbols[:k])))
                else:
                    _encode_subst_into(genome, row_pos[rows], row_strand[rows], sub_pos[rows], base[rows], R, r, local_order, symbols, cat_x)
                    logp.append(model.forward_symbols(cat_x[:k] if with_cat else None, symbols[:k]))
            delta[rows] = logp[0] - logp[1]
            # (the unchanged windows were encoded last; the INDEL window holds the site in column R - 1 on '+', R on '-')
            if indel:
                focal[rows] = symbols[:k].gather(1, (R - 1 + row_strand[rows].to(torch.int64))[:, None])[:, 0]
            else:
                focal[rows] = symbols[:k, R]
        dead = (row_pos < 0) | (row_pos >= genome.length)
        if not indel:
            dead |= row_pos == sub_pos
        delta = torch.where(dead[:, None], torch.full_like(delta, float("nan")), delta)
    return delta.reshape(m, W, n_class), focal.reshape(m, W)


# ----------------------------------------------------------------------------------------------------------------------------------
# alleles that change the sequence's length: insertions, deletions, multi-base replacements
# ----------------------------------------------------------------------------------------------------------------------------------
MAX_ALT = 32                        # bases of an alternate allele: 2 bits each in one uint64


def _pack_alt(alt):
    """The alternate bases as one integer (base i in bits 2i, 2i+1); ValueError for more than 32 bases or anything but A/C/G/T."""
    if len(alt) > MAX_ALT:
        raise ValueError(f"alternate allele of {len(alt)} bases: at most {MAX_ALT} are held")
    word = 0
    for i, ch in enumerate(alt):
        b = "ACGT".find(ch.upper())
        if b < 0 or len(ch) != 1:
            raise ValueError(f"alternate allele {alt!r}: only A/C/G/T can be inserted")
        word |= b << (2 * i)
    return word


def _live(length, p, d, k):
    return (p >= 0) & (d >= 0) & (p + d <= length) & (k >= 0) & (k <= MAX_ALT)


def alternate_sequence(seq, p, d, alt):
    """The string patch: `seq` with [p, p + d) replaced by `alt`; `seq` itself where the allele is not live."""
    if not bool(_live(len(seq), p, d, len(alt))):
        return seq
    return seq[:p] + alt + seq[p + d:]


class Alleles:
    """A table of alleles on the device: allele v replaces the '+'-strand reference bases [pos[v], pos[v] + ref_len[v]) by alt_len[v] plain
    bases, base i (0..3 = A, C, G, T) in bits 2i, 2i+1 of alt[v].  Four int64 tensors of one length (``alt`` holds the uint64 bit
    pattern).  ref_len = 0 inserts before pos (pos = chromosome length appends), alt_len = 0 deletes.  An allele is live iff 0 <= pos,
    0 <= ref_len, pos + ref_len <= length and 0 <= alt_len <= 32; the encoder reads the genome as it is for any other."""

    __slots__ = ("pos", "ref_len", "alt_len", "alt")

    def __init__(self, pos, ref_len, alt_len, alt):
        self.pos, self.ref_len, self.alt_len, self.alt = (t.to(torch.int64).contiguous() for t in (pos, ref_len, alt_len, alt))
        if self.pos.dim() != 1 or any(t.shape != self.pos.shape or t.device != self.pos.device for t in (self.ref_len, self.alt_len, self.alt)):
            raise ValueError("Alleles: four 1-D tensors of one length on one device")

    def __len__(self):
        return self.pos.shape[0]

    @property
    def device(self):
        return self.pos.device

    @classmethod
    def from_host(cls, pos, ref_len, alt_strings, device="cuda"):
        """From 0-based positions, reference lengths and alternate strings ("" deletes).  ValueError for an alternate longer than 32, one
        that holds anything but A/C/G/T, or a negative reference length."""
        pos, ref_len = np.asarray(pos, np.int64).reshape(-1), np.asarray(ref_len, np.int64).reshape(-1)
        if len(pos) != len(ref_len) or len(pos) != len(alt_strings):
            raise ValueError("Alleles.from_host: pos, ref_len and alt_strings must be equally long")
        if (ref_len < 0).any():
            raise ValueError("Alleles.from_host: a reference length is negative")
        words = np.array([_pack_alt(a) for a in alt_strings], np.uint64).reshape(-1)
        alt_len = np.array([len(a) for a in alt_strings], np.int64).reshape(-1)
        return cls(*(torch.from_numpy(a).to(device) for a in (pos, ref_len, alt_len, words.view(np.int64))))

    @staticmethod
    def from_vcf_fields(pos1, ref, alt):
        """0-based (p, d, alt) of a VCF record's 1-based POS, REF and one ALT: the shared prefix (the anchor base of an insertion or
        deletion) and then the shared suffix are trimmed.  Identical REF and ALT give the identity (d = 0, alt "")."""
        ref, alt = ref.upper(), alt.upper()
        lead = 0
        while lead < len(ref) and lead < len(alt) and ref[lead] == alt[lead]:
            lead += 1
        ref, alt = ref[lead:], alt[lead:]
        tail = 0
        while tail < len(ref) and tail < len(alt) and ref[-1 - tail] == alt[-1 - tail]:
            tail += 1
        return int(pos1) - 1 + lead, len(ref) - tail, alt[:len(alt) - tail]

    def host(self):
        """(pos, ref_len, alt_len int64; alt uint64) as numpy arrays."""
        p, d, k, a = (t.cpu().numpy() for t in (self.pos, self.ref_len, self.alt_len, self.alt))
        return p, d, k, a.view(np.uint64)


def _alleles_host(alleles):
    if isinstance(alleles, Alleles):
        return alleles.host()
    p, d, k, a = alleles
    a = np.asarray(a)
    return (np.asarray(p, np.int64), np.asarray(d, np.int64), np.asarray(k, np.int64),
            a.view(np.uint64) if a.dtype == np.int64 else a.astype(np.uint64))


def _allele_symbols_host(codes, pos, neg, off0, W, live, p, k, shift, alt):
    """(n, W) strand-oriented symbols of the windows at `pos` on the rows' alternate haplotypes (per-row live / p / k / shift / alt)"""
    L = len(codes)
    j = np.arange(W, dtype=np.int64)
    q = pos[:, None] + off0 + np.where(neg[:, None], W - 1 - j[None, :], j[None, :])     # position on the alternate haplotype
    p, k, shift, live = p[:, None], k[:, None], shift[:, None], live[:, None]
    hit = live & (q >= p) & (q < p + k)
    ref = np.where(live & (q >= p + k), q - shift, q)
    inside = (ref >= 0) & (ref < L)
    sym = np.full(q.shape, 4, np.uint8)
    sym[inside] = codes[ref[inside]]
    idx = np.where(hit, q - p, 0).astype(np.uint64)
    own = ((alt[:, None] >> (np.uint64(2) * idx)) & np.uint64(3)).astype(np.uint8)
    sym = np.where(hit, own, sym)
    return np.where(neg[:, None], _COMPLEMENT[sym], sym).astype(np.uint8)


def encode_allele_windows_host(genome, pos, strand, allele, alleles, radius, local_radius=None, local_order=None, model_type="snv"):
    """The numpy twin of ``mural_encode_allele_windows``: (symbols uint8 (n, W), cat_x int64 or None) of the windows at `pos` (alternate-
    haplotype coordinates) / `strand`, row i on the haplotype of allele ``allele[i]`` of `alleles` (an ``Alleles`` or a (pos, ref_len,
    alt_len, alt) tuple of arrays); -1, an index outside the table or an allele that is not live: the genome as it is."""
    codes = _codes(genome)
    pos, neg = np.asarray(pos, np.int64), np.asarray(strand) != 0
    a_pos, a_d, a_k, a_alt = _alleles_host(alleles)
    v = np.asarray(allele, np.int64)
    named = (v >= 0) & (v < len(a_pos))
    vi = np.where(named, v, 0)
    if len(a_pos):
        p, d, k, alt = a_pos[vi], a_d[vi], a_k[vi], a_alt[vi]
    else:
        p = d = k = np.zeros(len(v), np.int64)
        alt = np.zeros(len(v), np.uint64)
    live = named & _live(len(codes), p, d, k)
    p, k, shift = np.where(live, p, 0), np.where(live, k, 0), np.where(live, k - d, 0)
    off0, W = _window(radius, model_type)
    symbols = _allele_symbols_host(codes, pos, neg, off0, W, live, p, k, shift, alt)
    if model_type == "indel":
        return symbols, None
    loff, lW = _window(local_radius)
    digit = _allele_symbols_host(codes, pos, neg, loff, lW, live, p, k, shift, alt).astype(np.int64)
    ncol = lW - (local_order - 1)
    val = np.zeros((len(digit), ncol), np.int64)
    bad = np.zeros((len(digit), ncol), bool)
    for t in range(local_order):
        col = digit[:, t:t + ncol]
        bad |= col > 3
        val = val * 4 + np.where(col > 3, 0, col)
    return symbols, np.where(bad, 4 ** local_order, val)


def allele_footprint_offsets(radius, model_type="snv", device=None):
    """int64 offsets e of ``allele_footprint``'s second axis: [-R, R - 1] for the SNV models, [-R, R - 2] for the INDEL model.  e < 0 is
    the site p + e left of the allele, e >= 0 the site p + ref_len + e right of the replaced span."""
    off0, W = _window(radius, model_type)
    return torch.arange(W - 1, dtype=torch.int64, device=device) - (off0 + W - 1)


def allele_rows_host(length, alleles, strand, radius, first, count, model_type="snv"):
    """The numpy twin of ``mural_allele_rows``: (ref_pos int64, alt_pos int64, row_strand uint8, row_allele int64) of the row ids [first,
    first + count), id = v * (W - 1) + c.  `length` is the chromosome's."""
    a_pos, a_d, a_k, _ = _alleles_host(alleles)
    strand = (np.asarray(strand) != 0).astype(np.uint8)
    off0, W = _window(radius, model_type)
    slots = W - 1
    if first < 0 or count < 0 or first + count > len(a_pos) * slots:
        raise ValueError("allele_rows: ids [first, first + count) must lie in [0, n_alleles * (W - 1))")
    ids = first + np.arange(count, dtype=np.int64)
    v = ids // slots
    e = ids % slots - (off0 + W - 1)
    p = a_pos[v]
    live = _live(length, p, a_d[v], a_k[v])
    d, k = np.where(live, a_d[v], 0), np.where(live, a_k[v], 0)
    ref_pos = p + e + np.where(e < 0, 0, d)
    alt_pos = np.where(e < 0, ref_pos, ref_pos + k - d)
    return ref_pos, alt_pos, strand[v], np.where(live, v, -1)


def _encode_allele_into(genome, pos, strand, allele, alleles, radius, indel, local_radius, local_order, symbols, cat_x):
    g = genome.as_struct()
    with torch.cuda.device(genome.device):
        _lib.check(_lib.lib().mural_encode_allele_windows(
            C.byref(g), pos.data_ptr(), strand.data_ptr(), allele.data_ptr(), pos.shape[0], alleles.pos.data_ptr(),
            alleles.ref_len.data_ptr(), alleles.alt_len.data_ptr(), alleles.alt.data_ptr(), len(alleles), int(radius), int(indel),
            int(local_radius), int(local_order), None if symbols is None else symbols.data_ptr(),
            None if cat_x is None else cat_x.data_ptr(), _lib.current_stream_ptr(genome.device)))


def _require_alleles(alleles, device):
    if not isinstance(alleles, Alleles):
        raise TypeError("alleles must be a mural_amd.mutagenesis.Alleles")
    _lib.require_cuda(alleles.pos, "alleles")
    if alleles.device != torch.device(device):
        raise RuntimeError(f"alleles ({alleles.device}) and genome ({device}) must live on one HIP device")


def encode_allele_windows(genome, pos, strand, allele, alleles, radius, local_radius=None, local_order=None, model_type="snv"):
    """``PackedGenome.encode_allele_windows``: see there."""
    if model_type not in ("snv", "indel"):
        raise ValueError(f"model_type {model_type} not supported!")
    _require_alleles(alleles, genome.packed2.device)
    pos, strand = genome._prep(pos, strand)
    allele = torch.as_tensor(allele, dtype=torch.int64, device=genome.device).contiguous()
    if allele.shape != pos.shape:
        raise ValueError("allele must be 1-D and as long as pos")
    n = pos.shape[0]
    if model_type == "indel":
        symbols = torch.empty((n, 2 * radius), dtype=torch.uint8, device=genome.device)
        _encode_allele_into(genome, pos, strand, allele, alleles, radius, 1, 0, 0, symbols, None)
        return symbols, None
    if local_radius is None or local_order is None:
        raise ValueError("encode_allele_windows: the SNV windows need local_radius and local_order")
    symbols = torch.empty((n, 2 * radius + 1), dtype=torch.uint8, device=genome.device)
    cat_x = torch.empty((n, 2 * local_radius + 1 - (local_order - 1)), dtype=torch.int64, device=genome.device)
    _encode_allele_into(genome, pos, strand, allele, alleles, radius, 0, local_radius, local_order, symbols, cat_x)
    return symbols, cat_x


def _allele_rows_into(genome, alleles, strand, radius, indel, first, count, out):
    g = genome.as_struct()
    with torch.cuda.device(genome.device):
        _lib.check(_lib.lib().mural_allele_rows(C.byref(g), alleles.pos.data_ptr(), alleles.ref_len.data_ptr(), alleles.alt_len.data_ptr(),
                                               len(alleles), strand.data_ptr(), int(radius), int(indel), int(first), int(count),
                                               *[t.data_ptr() for t in out], _lib.current_stream_ptr(genome.device)))


def allele_rows(genome, alleles, strand, radius, first, count, model_type="snv"):
    """``mural_allele_rows`` on the device: (ref_pos, alt_pos, row_strand, row_allele) of the row ids [first, first + count); `strand` is
    one byte per allele.  ValueError for ids outside [0, n_alleles * (W - 1))."""
    if model_type not in ("snv", "indel"):
        raise ValueError(f"model_type {model_type} not supported!")
    _require_alleles(alleles, genome.packed2.device)
    dev = genome.device
    strand = torch.as_tensor(strand, dtype=torch.uint8, device=dev).contiguous()
    if strand.shape != alleles.pos.shape:
        raise ValueError("strand must hold one byte per allele")
    count = max(int(count), -1)
    out = (torch.empty(max(count, 0), dtype=torch.int64, device=dev), torch.empty(max(count, 0), dtype=torch.int64, device=dev),
           torch.empty(max(count, 0), dtype=torch.uint8, device=dev), torch.empty(max(count, 0), dtype=torch.int64, device=dev))
    _allele_rows_into(genome, alleles, strand, radius, model_type == "indel", first, count, out)
    return out


def allele_footprint(model, genome, alleles, strand, local_radius=None, local_order=3, chunk_windows=1 << 17, distal_radius=None, timings=None):
    """What each allele of an ``Alleles`` table (insertions, deletions, multi-base replacements) does to the sites it can reach, read on
    `strand` (uint8 per allele, 1 = '-'): ``(delta float32 (m, W - 1, n_class), focal uint8 (m, W - 1))``, second axis
    ``allele_footprint_offsets`` (e < 0: the site pos + e; e >= 0: the site pos + ref_len + e, which sits at + alt_len - ref_len on the
    alternate haplotype).  These are exactly the sites outside the replaced span whose window can differ between the two haplotypes.
    Every chunk of `chunk_windows` rows runs enumerate (``mural_allele_rows``) -> encode on the alternate haplotype -> encode on the
    reference -> two ``forward_symbols`` (and ``scores_log_softmax`` for a ``UNet_Small``) -> one float32 subtraction.  NaN where the
    site lies outside the chromosome and in every row of an allele that is not live; `focal` is the site's reference focal symbol on
    `strand` (N outside the chromosome).

    Sites inside the replaced span and on inserted bases have no counterpart on the other haplotype and are not part of the footprint;
    for what a one-base substitution does to the rate of its own site, ``saturation_mutagenesis`` / ``variant_footprint`` remain the
    tools.  Models and errors as ``variant_footprint``.  `timings`: as in ``saturation_mutagenesis`` (``rows_encode_ms``,
    ``forward_ms``)."""
    indel = _is_indel(model)
    if indel:
        R, r = _require_indel(model, distal_radius), 0
    else:
        R, r = _require_model(model, local_radius, local_order)
    if not isinstance(alleles, Alleles):
        raise TypeError("alleles must be a mural_amd.mutagenesis.Alleles")
    a_pos, strand = _sites(genome, model, alleles.pos, strand)
    if chunk_windows < 1:
        raise ValueError("chunk_windows must be >= 1")
    model_type = "indel" if indel else "snv"
    dev, m, slots, n_class = a_pos.device, len(alleles), _window(R, model_type)[1] - 1, model.n_class
    W = slots + 1
    with_cat = not indel and model.model_no == 2
    with torch.no_grad(), torch.cuda.device(dev):
        total = m * slots
        cap = min(int(chunk_windows), max(total, 1))
        rows = (torch.empty(cap, dtype=torch.int64, device=dev), torch.empty(cap, dtype=torch.int64, device=dev),
                torch.empty(cap, dtype=torch.uint8, device=dev), torch.empty(cap, dtype=torch.int64, device=dev))
        ref_pos, alt_pos, row_strand, row_allele = rows
        none = torch.full((cap,), -1, dtype=torch.int64, device=dev)
        symbols = torch.empty((cap, W), dtype=torch.uint8, device=dev)
        cat_x = torch.empty((cap, 2 * r + 1 - (local_order - 1)), dtype=torch.int64, device=dev) if with_cat else None
        delta = torch.empty((total, n_class), dtype=torch.float32, device=dev)
        focal = torch.empty(total, dtype=torch.uint8, device=dev)
        nan = torch.full((), float("nan"), dtype=torch.float32, device=dev)
        marks = []

        def mark():
            if timings is not None:
                marks.append(torch.cuda.Event(enable_timing=True))
                marks[-1].record()

        def forward(k):
            if indel:
                return scores_log_softmax(model.forward_symbols(symbols[:k]))
            return model.forward_symbols(cat_x[:k] if with_cat else None, symbols[:k])

        for c0 in range(0, total, cap):
            k = min(cap, total - c0)
            mark()
            _allele_rows_into(genome, alleles, strand, R, indel, c0, k, rows)
            _encode_allele_into(genome, alt_pos[:k], row_strand[:k], row_allele[:k], alleles, R, indel, r, local_order, symbols, cat_x)
            mark()
            alt_logp = forward(k)
            mark()
            _encode_allele_into(genome, ref_pos[:k], row_strand[:k], none[:k], alleles, R, indel, r, local_order, symbols, cat_x)
            mark()
            ref_logp = forward(k)
            mark()
            dead = (ref_pos[:k] < 0) | (ref_pos[:k] >= genome.length) | (row_allele[:k] < 0)
            delta[c0:c0 + k] = torch.where(dead[:, None], nan, alt_logp - ref_logp)
            # (the reference windows were encoded last; the INDEL window holds the site in column R - 1 on '+', R on '-')
            if indel:
                focal[c0:c0 + k] = symbols[:k].gather(1, (R - 1 + row_strand[:k].to(torch.int64))[:, None])[:, 0]
            else:
                focal[c0:c0 + k] = symbols[:k, R]
        if timings is not None:
            torch.cuda.synchronize(dev)
            for c in range(0, len(marks), 5):
                t = [marks[c + i].elapsed_time(marks[c + i + 1]) for i in range(4)]
                timings["rows_encode_ms"] = timings.get("rows_encode_ms", 0.0) + t[0] + t[2]
                timings["forward_ms"] = timings.get("forward_ms", 0.0) + t[1] + t[3]
    return delta.reshape(m, slots, n_class), focal.reshape(m, slots)
