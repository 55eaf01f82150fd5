"""Inputs and references of the edge tests of the window encoders (csrc/encode.hip: mural_encode_kmer / _onehot / _symbols;
csrc/mutagenesis.hip: mural_encode_subst_symbols; csrc/train_batch.hip: mural_train_batch_encode).  CPU only (numpy):
tests/test_encode_edges_host.py checks here that every family holds what it names, tests/test_gpu_encode_edges.py runs the families
through the C entries.

Every output is an integer, or a float32 from a table of seven values, so every comparison is bit equality.

References are oracle/encode_ref.py's (``seq_to_codes`` / ``gather_windows`` / ``kmer_encode`` / ``onehot_encode``), restated only where
the oracle has no function of that name:
  * symbols: the oracle's one-hot columns mapped back to the one code whose ``_OHE`` row they equal (``symbols_from_onehot``: the 15
    rows are distinct).  The symbol of a column is thereby defined by the reference's one-hot semantics (reverse the window, flip the
    channels), never by a complement table copied from the kernel.  The large cases use ``symbols_direct``: the window reversed and
    each code replaced by the code whose base set is the complement of its own (``COMPLEMENT``, derived from ``_OHE``); the host test
    proves the two equal on the small cases;
  * one substitution per row: the base is put into the gathered forward window, where the column's genome position equals ``sub_pos``,
    before the strand orientation;
  * a training batch: row by row from the references above."""
import functools

import numpy as np

from oracle import encode_ref as E

GUARD = 64                                   # elements in front of and behind every output
SYM_FILL = 0xA5                              # no symbol (symbols are 0..14)
KMER_FILL = -0x5A5A5A5A5A5A5A5B              # no k-mer id (ids are >= 0)
OHE_FILL = -7.25                             # no one-hot value
MURAL_E_INVALID = 1

# ------------------------------------------------------------------------------------------------------------------ launch code
# read off the launch code: (workgroups, threads, elements per thread, what an element is)
CAPS = {
    "encode_symbols_kernel": (16384, 256, 4, "bytes, in groups of 4"),
    "encode_onehot_kernel": (16384, 256, 1, "columns"),
    "encode_kmer_kernel": (8192, 256, 1, "k-mer ids"),
    "reader_windows_kernel": (16384, 256, 4, "bytes, in units of 4"),
}
CAP_RADIUS, CAP_WIDTH = 1024, 2048           # indel window
CAP_ROWS = {"encode_symbols_kernel": (8192, 8193), "encode_onehot_kernel": (2048, 2049), "encode_kmer_kernel": (1024, 1025),
            "reader_windows_kernel": (8192, 8193)}
TB_LDS_LIMIT = 48 * 1024


def cap_elements(kernel):
    wg, threads, per, _ = CAPS[kernel]
    return wg * threads * per


def window(radius, indel):
    """(offset of the window's first position from the site, width)"""
    return E.window_geometry(radius, "indel" if indel else "snv")


def mt(indel):
    return "indel" if indel else "snv"


def strand_symbols(strand):
    return ["-" if s else "+" for s in strand]


# ------------------------------------------------------------------------------------------------------------------ references
def _base_set(code):
    return frozenset(int(i) for i in np.nonzero(E._OHE[code])[0])


def _complement_table():
    """code -> the code whose base set is {3 - b : b in this code's base set} (A<->T, C<->G applied to the set)"""
    sets = {_base_set(c): c for c in range(len(E.IUPAC))}
    assert len(sets) == len(E.IUPAC)
    return np.array([sets[frozenset(3 - b for b in _base_set(c))] for c in range(len(E.IUPAC))], np.uint8)


COMPLEMENT = _complement_table()


def symbols_from_onehot(ohe):
    """(n, 4, W) float32 columns -> (n, W) uint8: the one code whose _OHE row equals the column, bit for bit"""
    n, _, w = ohe.shape
    out = np.empty((n, w), np.uint8)
    step = max(1, (1 << 20) // max(w, 1))
    table = E._OHE.view(np.uint32)
    for lo in range(0, n, step):
        cols = np.ascontiguousarray(ohe[lo:lo + step].transpose(0, 2, 1)).view(np.uint32)
        eq = (cols[:, :, None, :] == table[None, None, :, :]).all(axis=-1)
        assert (eq.sum(axis=-1) == 1).all(), "a column that is not exactly one _OHE row"
        out[lo:lo + step] = eq.argmax(axis=-1)
    return out


def orient_onehot(win, strand):
    """forward windows (n, W) of codes -> strand-oriented (n, 4, W) float32, by encode_ref.onehot_encode's own rule"""
    neg = np.asarray(strand, dtype=bool)
    fwd = E._OHE[win]
    out = np.where(neg[:, None, None], fwd[:, ::-1, ::-1], fwd)
    return np.ascontiguousarray(out.transpose(0, 2, 1))


def orient_direct(win, strand, complement=None):
    """forward windows -> strand-oriented symbols: reversed and complemented by base set on '-'"""
    comp = COMPLEMENT if complement is None else complement
    neg = np.asarray(strand, dtype=bool)
    return np.where(neg[:, None], comp[win[:, ::-1]], win).astype(np.uint8)


def onehot_ref(g, pos, strand, radius, indel):
    return E.onehot_encode(g.codes, pos, strand_symbols(strand), radius, mt(indel))


def symbols_ref(g, pos, strand, radius, indel):
    return symbols_from_onehot(onehot_ref(g, pos, strand, radius, indel))


def symbols_direct(g, pos, strand, radius, indel, complement=None):
    return orient_direct(E.gather_windows(g.codes, pos, radius, mt(indel)), strand, complement)


def kmer_ref(g, pos, strand, radius, order, indel):
    return E.kmer_encode(g.codes, pos, strand_symbols(strand), radius, order, mt(indel))


def subst_windows(g, pos, strand, sub_pos, sub_base, radius, indel):
    """forward windows with the column at genome position sub_pos set to the plain base sub_base (0..3); no substitution where
    sub_base > 3 or sub_pos lies outside the record; (windows, rows x columns that were hit)"""
    off, width = window(radius, indel)
    pos, sub_pos, sub_base = np.asarray(pos, np.int64), np.asarray(sub_pos, np.int64), np.asarray(sub_base, np.uint8)
    win = E.gather_windows(g.codes, pos, radius, mt(indel))
    idx = pos[:, None] + off + np.arange(width, dtype=np.int64)[None, :]
    live = (sub_base < 4) & (sub_pos >= 0) & (sub_pos < g.length)
    hit = live[:, None] & (idx == sub_pos[:, None])
    win[hit] = np.broadcast_to(sub_base[:, None], win.shape)[hit]
    return win, hit


def subst_symbols_ref(g, pos, strand, sub_pos, sub_base, radius, indel, direct=False):
    win, _ = subst_windows(g, pos, strand, sub_pos, sub_base, radius, indel)
    return orient_direct(win, strand) if direct else symbols_from_onehot(orient_onehot(win, strand))


# ------------------------------------------------------------------------------------------------------------------ genomes
class Genome:
    """codes (oracle alphabet, one uint8 per base) and the packed form the product reads: packed2 / nmask words by
    encode_ref.pack_codes, the side table of the ambiguity codes other than N in ascending position"""

    def __init__(self, name, codes):
        self.name, self.codes, self.length = name, np.asarray(codes, np.uint8), len(codes)
        self.packed, self.mask = E.pack_codes(self.codes)
        self.amb_pos = np.nonzero(self.codes > E.CODE_N)[0].astype(np.int64)
        self.amb_sym = self.codes[self.amb_pos].astype(np.uint8)

    def __repr__(self):
        return self.name


def _acgt(length, seed):
    return np.random.default_rng(seed).integers(0, 4, size=length).astype(np.uint8)


SMALL_LENGTHS = [1, 15, 16, 17, 31, 32, 33, 63, 64, 65]
BIG_LENGTH = 5003                                # no multiple of 16
SIDE_TABLE_SIZES = [0, 1, 2, 63, 64, 65, 4096, 4097]


def end_genome(length, kind):
    """'acgt'; 'n': first and last base N; 'iupac': first and last base an ambiguity code other than N"""
    codes = _acgt(length, 100 + length)
    if kind == "n":
        codes[0] = codes[-1] = E.CODE_N
    elif kind == "iupac":
        codes[0], codes[-1] = 5 + length % 10, 5 + (length + 3) % 10
    else:
        assert kind == "acgt"
    return Genome(f"L{length} {kind}", codes)


def n_run_genome(length):
    """N at 27 .. 36 (across the mask-word boundary at 32), and up to the last base across the last boundary of a longer record"""
    codes = _acgt(length, 200 + length)
    codes[27:37] = E.CODE_N
    last = (length - 1) // 32 * 32
    if last > 64:
        codes[last - 4:length] = E.CODE_N
    return Genome(f"L{length} N run", codes)


def side_table_genome(k, first=True):
    """BIG_LENGTH bases with exactly k ambiguity codes other than N: at 0 and length - 1 (k = 1: at 0 if `first`, else at length - 1),
    then 1, 2, length - 2 (adjacent entries), the rest drawn; the ten codes in turn.  20 bases are N, two of them next to an entry:
    their mask bits are set and no side-table entry answers for them (with k = 0 the struct holds NULL pointers)."""
    length = BIG_LENGTH
    rng = np.random.default_rng(300 + k)
    codes = _acgt(length, 400 + k)
    fixed = [0, length - 1, 1, 2, length - 2]
    if k == 1 and not first:
        fixed = [length - 1]
    at = fixed[:k]
    if k > len(at):
        rest = np.setdiff1d(np.arange(3, length - 2), [3, length - 3])
        at = at + rng.choice(rest, size=k - len(at), replace=False).tolist()
    at = np.sort(np.asarray(at, np.int64))
    codes[at] = 5 + np.arange(k) % 10
    free = np.setdiff1d(np.arange(length), at)
    n_at = np.union1d(rng.choice(free, size=18, replace=False), [3, length - 3])
    n_at = np.setdiff1d(n_at, at)
    codes[n_at] = E.CODE_N
    return Genome(f"L{length} side table {k}" + ("" if k != 1 else " first" if first else " last"), codes)


@functools.lru_cache(maxsize=None)
def genomes():
    out = [end_genome(n, kind) for n in SMALL_LENGTHS for kind in ("acgt", "n", "iupac")]
    out += [end_genome(BIG_LENGTH, "acgt"), n_run_genome(65), n_run_genome(BIG_LENGTH)]
    out += [side_table_genome(k) for k in SIDE_TABLE_SIZES] + [side_table_genome(1, first=False)]
    return tuple(out)


def genome_named(name):
    return next(g for g in genomes() if g.name == name)


def mixed_genome():
    """the record of the row-count, cap and wrapper cases: 65 ambiguity codes, N, both ends ambiguous"""
    return genome_named(f"L{BIG_LENGTH} side table 65")


def all_codes_genome():
    """every code of the alphabet in 64 bases, in both orders: what the complement checks read on both strands"""
    return Genome("L64 every code", np.r_[np.arange(15), np.arange(15)[::-1], _acgt(34, 9)].astype(np.uint8))


# ------------------------------------------------------------------------------------------------------------------ sites
RADII = [1, 2, 3, 100, 1000]
GEOMETRIES = [(r, indel) for r in RADII for indel in (0, 1)]
ROW_COUNTS = [1, 2, 3, 4, 5, 7, 64, 257]


def edge_positions(length, radius):
    """0, 1, length - 2, length - 1; the middle; a window wholly in front of the record and one wholly behind it; either side of every
    multiple of 16 (so of 32) within 64 bases of either end"""
    at = {0, 1, length - 2, length - 1, length // 2, -radius - 5, length + radius + 5}
    for m in range(0, length + 17, 16):
        if m <= 64 or m >= length - 64:
            at.update((m - 1, m, m + 1))
    return np.array(sorted(at), np.int64)


def edge_sites(length, radius):
    """every edge position on both strands, strands alternating within the call"""
    pos = np.repeat(edge_positions(length, radius), 2)
    strand = (np.arange(len(pos)) % 2).astype(np.uint8)
    return pos, strand


def site_cases(radius, indel):
    """(label, genome, pos, strand) for every genome at its edge sites"""
    return [(f"{g.name} R{radius} {mt(indel)}", g) + edge_sites(g.length, radius) for g in genomes()]


def count_case(n, radius, indel):
    """n drawn sites (outside the record too) of the mixed genome, strands drawn"""
    g = mixed_genome()
    rng = np.random.default_rng(1000 * n + 2 * radius + indel)
    pos = rng.integers(-radius - 2, g.length + radius + 2, size=n).astype(np.int64)
    strand = rng.integers(0, 2, size=n).astype(np.uint8)
    return f"n{n} R{radius} {mt(indel)}", g, pos, strand


def subst_case(n, radius, indel):
    """count_case with one substitution per row, by row number mod 6: in the window; on the site; outside the window; outside the
    record; base 255 (none); on an ambiguity code or N of the record when the window holds one"""
    label, g, pos, strand = count_case(n, radius, indel)
    off, width = window(radius, indel)
    rng = np.random.default_rng(7 * n + radius)
    sub_pos = pos + off + rng.integers(0, width, size=n)
    sub_base = rng.integers(0, 4, size=n).astype(np.uint8)
    kind = np.arange(n) % 6
    sub_pos[kind == 1] = pos[kind == 1]
    sub_pos[kind == 2] = pos[kind == 2] + off + width
    sub_pos[kind == 3] = g.length + (np.arange(n)[kind == 3] % 3) * (-g.length - 1)       # length, -1, -length - 2
    sub_base[kind == 4] = 255
    masked = np.nonzero(g.codes >= E.CODE_N)[0]
    for i in np.nonzero(kind == 5)[0]:
        inside = masked[(masked >= pos[i] + off) & (masked < pos[i] + off + width)]
        if len(inside):
            sub_pos[i] = inside[i % len(inside)]
    return label + " subst", g, pos, strand, sub_pos.astype(np.int64), sub_base


# ------------------------------------------------------------------------------------------------------------------ k-mer
ORDERS = list(range(1, 13))
KMER_GENOMES = ["L1 iupac", "L15 n", "L16 acgt", "L17 iupac", "L33 n", "L65 N run", f"L{BIG_LENGTH} side table 65"]


def kmer_geometries(order):
    """(radius, indel, ncol): the narrowest window the order fits (ncol 1 where a window of exactly `order` columns exists: odd orders
    from 3 on the snv window, even orders on the indel window; order 1 has none, the narrowest window has 2 columns), the window of
    order + 1 columns (ncol 2), and both windows of radius 10"""
    out = []
    for radius in range(1, 12):
        for indel in (0, 1):
            ncol = window(radius, indel)[1] - (order - 1)
            if ncol in (1, 2) or radius == 10:
                out.append((radius, indel, ncol))
    return out


KMER_REJECTED = [(1, 0, 0), (1, 13, 0), (10, 0, 1), (10, 13, 1), (1, 4, 0), (1, 3, 1), (5, 11, 1), (5, 12, 0), (0, 1, 0), (-1, 1, 1)]     # (radius, order, indel)


def kmer_cases(order):
    out = []
    for radius, indel, ncol in kmer_geometries(order):
        for name in KMER_GENOMES:
            g = genome_named(name)
            out.append((f"{g.name} order {order} R{radius} {mt(indel)} ncol {ncol}", g) + edge_sites(g.length, radius) + (radius, indel))
    return out


# ------------------------------------------------------------------------------------------------------------------ grid caps
def cap_case(n):
    """n sites of the indel window of radius 1024 on the mixed genome: positions drawn from -1100 .. length + 1100, strands drawn"""
    g = mixed_genome()
    rng = np.random.default_rng(n)
    pos = rng.integers(-1100, g.length + 1100, size=n).astype(np.int64)
    strand = rng.integers(0, 2, size=n).astype(np.uint8)
    return g, pos, strand


def cap_subst(n):
    """one live substitution per row: a column of the row's window that lies inside the record, a base that differs from the record's"""
    g, pos, strand = cap_case(n)
    pos = np.clip(pos, 0, g.length - 1)
    off, width = window(CAP_RADIUS, 1)
    rng = np.random.default_rng(n + 1)
    lo, hi = np.maximum(pos + off, 0), np.minimum(pos + off + width, g.length)
    sub_pos = lo + rng.integers(0, 1 << 30, size=n) % (hi - lo)
    sub_base = ((np.where(g.codes[sub_pos] < 4, g.codes[sub_pos], 0) + 1 + rng.integers(0, 3, size=n)) % 4).astype(np.uint8)
    return g, pos, strand, sub_pos.astype(np.int64), sub_base


# ------------------------------------------------------------------------------------------------------------------ training batch
def batch_geometry(local_radius, order, distal_radius, indel):
    """TrainBatchGeom as the entry computes it: the union of the two windows and the staging bytes"""
    off_l, width_l = window(local_radius, indel)
    off_d, width_d = window(distal_radius, indel)
    lo = min(off_l, off_d)
    span = max(off_l + width_l, off_d + width_d) - lo
    lds = (span // 16 + 2 + span // 32 + 2) * 4 + span
    return dict(off_l=off_l, width_l=width_l, ncol=width_l - (order - 1), off_d=off_d, width_d=width_d, lo=lo, span=span, lds=lds)


def staging_boundary_radius(indel=0):
    """the largest distal radius (local radius 2) whose staging fits TB_LDS_LIMIT"""
    radius = 1
    while batch_geometry(2, 2, radius + 1, indel)["lds"] <= TB_LDS_LIMIT:
        radius += 1
    return radius


@functools.lru_cache(maxsize=None)
def batch_genomes():
    """three records: one base (an ambiguity code), 17 bases (first an ambiguity code, last N), 40009 bases with N, N runs and codes"""
    one = Genome("L1 R", np.array([5], np.uint8))
    codes = _acgt(17, 17)
    codes[0], codes[-1] = 9, E.CODE_N
    small = Genome("L17 W..N", codes)
    rng = np.random.default_rng(40009)
    codes = rng.choice(np.arange(15, dtype=np.uint8), size=40009, p=[.2475] * 4 + [.005] + [.0005] * 10)
    codes[27:37] = E.CODE_N
    codes[0], codes[-1] = 14, 12
    return (one, small, Genome("L40009 mixed", codes))


class RowTable:
    """rows over the three records: the edge positions of each on both strands; then two rows whose chromosome is -1 and n_genomes"""

    def __init__(self):
        gs = batch_genomes()
        chrom, pos, strand = [], [], []
        for c, g in enumerate(gs):
            at = edge_positions(g.length, 3)
            chrom += [c] * (2 * len(at))
            pos += np.repeat(at, 2).tolist()
            strand += [0, 1] * len(at)
        self.n_valid = len(chrom)
        chrom += [-1, len(gs)]
        pos += [5, 5]
        strand += [0, 1]
        self.chrom, self.pos = np.array(chrom, np.int32), np.array(pos, np.int64)
        self.strand = np.array(strand, np.uint8)
        self.label = (np.random.default_rng(5).integers(0, 4, size=len(chrom))).astype(np.uint8)
        self.label[:4] = (0, 1, 2, 3)
        self.n_rows = len(chrom)
        self.bad_chrom_rows = (self.n_rows - 2, self.n_rows - 1)


@functools.lru_cache(maxsize=None)
def row_table():
    return RowTable()


# (label, local_radius, order, distal_radius, indel, B values)
def batch_cases():
    big = staging_boundary_radius(0)
    out = [("local wider than distal", 40, 3, 8, 0, (37,)), ("local wider than distal, indel", 40, 3, 8, 1, (37,)),
           ("equal radii", 8, 3, 8, 0, (37,)), ("equal radii, indel", 8, 3, 8, 1, (37,)),
           ("order 12, ncol 1", 6, 12, 10, 1, (37,)), ("order 11, ncol 1", 5, 11, 9, 0, (37,)),
           ("distal radius 1", 4, 3, 1, 0, (37,)), ("distal radius 1, indel", 4, 3, 1, 1, (37,)),
           ("the existing geometry", 4, 3, 110, 0, (37,))]
    for radius, indel in ((1, 0), (2, 0), (1, 1), (2, 1)):
        out.append((f"distal width {window(radius, indel)[1]}", 2, 2, radius, indel, (1, 2, 3, 4, 5)))
    out.append((f"staging limit: distal radius {big}", 2, 2, big, 0, (3,)))
    return out


def batch_order(first, B, seed, table=None):
    """`first` + B + 2 entries: valid rows, drawn with repeats"""
    table = table or row_table()
    return np.random.default_rng(seed).integers(0, table.n_valid, size=first + B + 2).astype(np.int64)


def batch_ref(order, first, B, local_radius, local_order, distal_radius, indel, table=None, gs=None):
    """dict(cat int64 (B, ncol), sym uint8 (B, W), onehot float32 (B, 4, W), y float32 (B,), status) of rows order[first : first + B]; a
    row number outside the table and a chromosome outside the list read an empty record (every column N), label 0, status
    MURAL_E_INVALID"""
    table, gs = table or row_table(), gs or batch_genomes()
    gm = batch_geometry(local_radius, local_order, distal_radius, indel)
    empty = Genome("empty", np.zeros(0, np.uint8))
    cat = np.empty((B, gm["ncol"]), np.int64)
    onehot = np.empty((B, 4, gm["width_d"]), np.float32)
    y = np.zeros(B, np.float32)
    status = 0
    for b in range(B):
        r = int(order[first + b])
        g, pos, strand = empty, np.zeros(1, np.int64), np.zeros(1, np.uint8)
        if 0 <= r < table.n_rows and 0 <= table.chrom[r] < len(gs):
            g, pos, strand = gs[table.chrom[r]], table.pos[r:r + 1], table.strand[r:r + 1]
            y[b] = float(table.label[r])
        else:
            status |= MURAL_E_INVALID
        cat[b] = kmer_ref(g, pos, strand, local_radius, local_order, indel)[0]
        onehot[b] = onehot_ref(g, pos, strand, distal_radius, indel)[0]
    return dict(cat=cat, sym=symbols_from_onehot(onehot), onehot=onehot, y=y, status=status)
