"""The window encoders one by one through their C entries (csrc/encode.hip: mural_encode_symbols / _onehot / _kmer; csrc/mutagenesis.hip:
mural_encode_subst_symbols; csrc/train_batch.hip: mural_train_batch_encode) at the record, word, row and grid edges of
tests/_encode_edges_data.py, against references built on oracle/encode_ref.py (tests/test_encode_edges_host.py checks those inputs and
references first).  The genomes are packed by the oracle's ``pack_codes`` and handed over as a MuralGenome struct built here, so a side
table of no entries is two NULL pointers.  Every output lies between two guards of 64 elements and holds a sentinel before the call;
every return code and status word is read; every comparison is bit equality (integer kernels: no tolerance exists)."""
import ctypes as C

import numpy as np
import pytest
import torch

from mural_amd import _lib
from tests import _encode_edges_data as D

pytestmark = pytest.mark.gpu
GUARD = D.GUARD


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


class _DevGenome:
    """the record on the device and its struct (NULL side-table pointers when it has no entry)"""

    def __init__(self, g):
        self.packed, self.mask = _dev(g.packed.view(np.int32)), _dev(g.mask.view(np.int32))
        self.amb_pos = _dev(g.amb_pos) if len(g.amb_pos) else None
        self.amb_sym = _dev(g.amb_sym) if len(g.amb_pos) else None
        self.struct = _lib.MuralGenome(self.packed.data_ptr(), self.mask.data_ptr(), g.length,
                                       None if self.amb_pos is None else self.amb_pos.data_ptr(),
                                       None if self.amb_sym is None else self.amb_sym.data_ptr(), len(g.amb_pos))
        assert (self.struct.amb_pos is None) == (len(g.amb_pos) == 0)

    @property
    def ref(self):
        return C.byref(self.struct)


_genomes = {}


def _genome(g):
    if g.name not in _genomes:
        _genomes[g.name] = _DevGenome(g)
    return _genomes[g.name]


class _Guarded:
    """n elements of `dtype` holding `fill`, GUARD elements of it in front and behind (and `shift` more in front: a pointer that is not
    aligned to 4 bytes); ``take`` reads the elements back after checking that nothing around them changed"""

    def __init__(self, n, dtype, fill, shift=0):
        self.n, self.at, self.fill = n, GUARD + shift, fill
        self.buf = torch.full((GUARD + shift + n + GUARD,), fill, dtype=dtype, device="cuda")
        assert self.buf.data_ptr() % 16 == 0
        self.ptr = self.buf.data_ptr() + self.at * self.buf.element_size()

    def take(self, case):
        torch.cuda.synchronize()
        host = self.buf.cpu().numpy()
        assert (host[:self.at] == self.fill).all() and (host[self.at + self.n:] == self.fill).all(), f"{case}: a guard was written"
        return host[self.at:self.at + self.n]

    def untouched(self, case):
        assert (self.take(case) == self.fill).all(), f"{case}: the output was written"


def _same(got, want, what, case):
    """bit equality (float32 compared as words: -0 is not 0)"""
    got, want = np.ascontiguousarray(got), np.ascontiguousarray(want)
    assert got.shape == want.shape and got.dtype == want.dtype, (what, case, got.shape, want.shape)
    if got.dtype == np.float32:
        got, want = got.view(np.uint32), want.view(np.uint32)
    if not np.array_equal(got, want):
        bad = np.argwhere(got != want)
        raise AssertionError(f"{what} at {case}: {len(bad)} of {got.size} differ, first at {bad[0].tolist()}: "
                             f"{got[tuple(bad[0])]} for {want[tuple(bad[0])]}")


def _sites(pos, strand):
    return _dev(np.asarray(pos, np.int64)), _dev(np.asarray(strand, np.uint8))


def _symbols(g, pos, strand, radius, indel, case, shift=0):
    n, width = len(pos), D.window(radius, indel)[1]
    dp, ds = _sites(pos, strand)
    out = _Guarded(n * width, torch.uint8, D.SYM_FILL, shift)
    rc = _lib.lib().mural_encode_symbols(_genome(g).ref, dp.data_ptr(), ds.data_ptr(), n, radius, indel, out.ptr, None)
    assert rc == 0, (case, _lib.lib().mural_last_error())
    return out.take(case).reshape(n, width)


def _onehot(g, pos, strand, radius, indel, case):
    n, width = len(pos), D.window(radius, indel)[1]
    dp, ds = _sites(pos, strand)
    out = _Guarded(n * 4 * width, torch.float32, D.OHE_FILL)
    rc = _lib.lib().mural_encode_onehot(_genome(g).ref, dp.data_ptr(), ds.data_ptr(), n, radius, indel, out.ptr, None)
    assert rc == 0, (case, _lib.lib().mural_last_error())
    return out.take(case).reshape(n, 4, width)


def _kmer(g, pos, strand, radius, order, indel, case):
    n, ncol = len(pos), D.window(radius, indel)[1] - (order - 1)
    dp, ds = _sites(pos, strand)
    out = _Guarded(n * ncol, torch.int64, D.KMER_FILL)
    rc = _lib.lib().mural_encode_kmer(_genome(g).ref, dp.data_ptr(), ds.data_ptr(), n, radius, order, indel, out.ptr, None)
    assert rc == 0, (case, _lib.lib().mural_last_error())
    return out.take(case).reshape(n, ncol)


def _subst(g, pos, strand, sub_pos, sub_base, radius, indel, case):
    n, width = len(pos), D.window(radius, indel)[1]
    dp, ds = _sites(pos, strand)
    dsp, dsb = _dev(np.asarray(sub_pos, np.int64)), _dev(np.asarray(sub_base, np.uint8))
    out = _Guarded(n * width, torch.uint8, D.SYM_FILL)
    rc = _lib.lib().mural_encode_subst_symbols(_genome(g).ref, dp.data_ptr(), ds.data_ptr(), dsp.data_ptr(), dsb.data_ptr(), n, radius, indel,
                                               out.ptr, None)
    assert rc == 0, (case, _lib.lib().mural_last_error())
    return out.take(case).reshape(n, width)


# ================================================================================================================== record and word edges
@pytest.mark.parametrize("radius,indel", D.GEOMETRIES)
def test_encoders_at_the_record_edges(radius, indel):
    """every genome of the data module (lengths 1 .. 65 around the word sizes and 5003; N or an ambiguity code first and last; N runs
    across a mask word; side tables of 0 (NULL), 1, 2, 63, 64, 65, 4096, 4097 entries) at its edge sites on both strands: positions 0, 1,
    length - 2, length - 1, either side of the multiples of 16, windows over both ends and wholly outside the record.  The one-hot
    tensor equals the oracle's; the symbols equal the oracle's one-hot columns mapped back to codes; the k-mer ids of order 3 (2 on the
    window of two columns) equal the oracle's."""
    order = min(3, D.window(radius, indel)[1])
    for case, g, pos, strand in D.site_cases(radius, indel):
        want = D.onehot_ref(g, pos, strand, radius, indel)
        _same(_onehot(g, pos, strand, radius, indel, case), want, "one-hot", case)
        _same(_symbols(g, pos, strand, radius, indel, case), D.symbols_from_onehot(want), "symbols", case)
        _same(_kmer(g, pos, strand, radius, order, indel, case), D.kmer_ref(g, pos, strand, radius, order, indel), "k-mer ids", case)


@pytest.mark.parametrize("radius,indel", D.GEOMETRIES)
def test_encoders_at_every_row_count_and_alignment(radius, indel):
    """n = 1, 2, 3, 4, 5, 7, 64, 257 drawn sites: n * W mod 4 takes every residue and the rows of the odd windows start at every byte
    alignment, so groups of 4 bytes straddle two rows and the last group is partial.  The symbols also into a buffer that starts 1, 2
    and 3 bytes past a 4-byte boundary (the kernel's byte-by-byte branch), and with one substitution per row (reader_windows_kernel);
    k-mer ids of order 3 (2 on the window of two columns) of the same sites."""
    order = min(3, D.window(radius, indel)[1])
    for n in D.ROW_COUNTS:
        case, g, pos, strand = D.count_case(n, radius, indel)
        _same(_kmer(g, pos, strand, radius, order, indel, case), D.kmer_ref(g, pos, strand, radius, order, indel), "k-mer ids", case)
        want = D.onehot_ref(g, pos, strand, radius, indel)
        sym = D.symbols_from_onehot(want)
        _same(_onehot(g, pos, strand, radius, indel, case), want, "one-hot", case)
        for shift in (0, 1, 2, 3):
            _same(_symbols(g, pos, strand, radius, indel, f"{case} shift {shift}", shift), sym, "symbols", f"{case} shift {shift}")
        case, g, pos, strand, sub_pos, sub_base = D.subst_case(n, radius, indel)
        _same(_subst(g, pos, strand, sub_pos, sub_base, radius, indel, case),
              D.subst_symbols_ref(g, pos, strand, sub_pos, sub_base, radius, indel), "substituted symbols", case)


@pytest.mark.parametrize("order", D.ORDERS)
def test_kmer_ids_at_every_order(order):
    """orders 1 .. 12 on the narrowest window that holds the order (one column from order 2 on), the window of two columns and both
    windows of radius 10; records of 1 to 65 bases with N / ambiguity codes at their ends and the mixed record, edge sites on both
    strands: the sentinel 4^order, the '-' strand's digits next to a bad symbol, and ids of clean k-mers are all among the values"""
    seen_clean = seen_sentinel = False
    for case, g, pos, strand, radius, indel in D.kmer_cases(order):
        want = D.kmer_ref(g, pos, strand, radius, order, indel)
        _same(_kmer(g, pos, strand, radius, order, indel, case), want, "k-mer ids", case)
        seen_clean |= bool((want[strand != 0] < 4 ** order).any())
        seen_sentinel |= bool((want[strand != 0] == 4 ** order).any())
    assert seen_clean and seen_sentinel


# ================================================================================================================== refusals, empty calls
def test_refused_calls_leave_their_outputs():
    """orders 0 and 13, an order wider than the window, radius 0 and -1: a non-zero code, a message, nothing written; n = 0 is OK with
    NULL pointers and writes nothing; a NULL genome pointer and a side table of one entry without its pointers are refused"""
    lib = _lib.lib()
    g = D.mixed_genome()
    dg = _genome(g)
    pos, strand = D.edge_sites(g.length, 3)
    dp, ds = _sites(pos, strand)
    n = len(pos)
    out = _Guarded(n * 64, torch.int64, D.KMER_FILL)
    for radius, order, indel in D.KMER_REJECTED:
        rc = lib.mural_encode_kmer(dg.ref, dp.data_ptr(), ds.data_ptr(), n, radius, order, indel, out.ptr, None)
        assert rc != 0, (radius, order, indel)
        with pytest.raises(ValueError, match="order|radius|window"):
            _lib.check(rc)
    out.untouched("k-mer refusals")
    sym = _Guarded(n * 64, torch.uint8, D.SYM_FILL)
    ohe = _Guarded(n * 64, torch.float32, D.OHE_FILL)
    sp, sb = _dev(pos), _dev(np.zeros(n, np.uint8))
    for radius in (0, -1):
        for indel in (0, 1):
            for rc in (lib.mural_encode_symbols(dg.ref, dp.data_ptr(), ds.data_ptr(), n, radius, indel, sym.ptr, None),
                       lib.mural_encode_onehot(dg.ref, dp.data_ptr(), ds.data_ptr(), n, radius, indel, ohe.ptr, None),
                       lib.mural_encode_subst_symbols(dg.ref, dp.data_ptr(), ds.data_ptr(), sp.data_ptr(), sb.data_ptr(), n, radius, indel,
                                                      sym.ptr, None)):
                assert rc != 0
                with pytest.raises(ValueError, match="radius"):
                    _lib.check(rc)
    # a genome without words, and a counted side table without pointers
    no_words = _lib.MuralGenome(None, None, g.length, None, None, 0)
    no_table = _lib.MuralGenome(dg.packed.data_ptr(), dg.mask.data_ptr(), g.length, None, None, 1)
    for bad in (no_words, no_table):
        assert lib.mural_encode_symbols(C.byref(bad), dp.data_ptr(), ds.data_ptr(), n, 3, 0, sym.ptr, None) != 0
        assert lib.mural_encode_onehot(C.byref(bad), dp.data_ptr(), ds.data_ptr(), n, 3, 0, ohe.ptr, None) != 0
        assert lib.mural_encode_subst_symbols(C.byref(bad), dp.data_ptr(), ds.data_ptr(), sp.data_ptr(), sb.data_ptr(), n, 3, 0, sym.ptr, None) != 0
    assert lib.mural_encode_kmer(C.byref(no_words), dp.data_ptr(), ds.data_ptr(), n, 3, 3, 0, out.ptr, None) != 0
    assert lib.mural_encode_symbols(None, dp.data_ptr(), ds.data_ptr(), n, 3, 0, sym.ptr, None) != 0
    # NULL row arrays with n > 0
    assert lib.mural_encode_symbols(dg.ref, None, ds.data_ptr(), n, 3, 0, sym.ptr, None) != 0
    assert lib.mural_encode_onehot(dg.ref, dp.data_ptr(), None, n, 3, 0, ohe.ptr, None) != 0
    assert lib.mural_encode_kmer(dg.ref, dp.data_ptr(), ds.data_ptr(), n, 3, 3, 0, None, None) != 0
    # empty calls
    assert lib.mural_encode_symbols(dg.ref, None, None, 0, 3, 0, sym.ptr, None) == 0
    assert lib.mural_encode_onehot(dg.ref, None, None, 0, 3, 1, ohe.ptr, None) == 0
    assert lib.mural_encode_kmer(dg.ref, None, None, 0, 3, 3, 0, out.ptr, None) == 0
    assert lib.mural_encode_subst_symbols(dg.ref, None, None, None, None, 0, 3, 0, sym.ptr, None) == 0
    assert lib.mural_encode_symbols(dg.ref, None, None, 0, 3, 0, None, None) == 0
    for buf, what in ((out, "k-mer"), (sym, "symbols"), (ohe, "one-hot")):
        buf.untouched(what + " refusals and empty calls")


# ================================================================================================================== capped grids
@pytest.mark.parametrize("n", D.CAP_ROWS["encode_symbols_kernel"])
def test_symbols_on_and_beyond_one_round_of_the_grid(n):
    """indel windows of 2048 columns: 8192 rows are 16384 x 256 groups of 4 bytes, one round of the capped grid exactly; row 8193 belongs
    to a second round"""
    g, pos, strand = D.cap_case(n)
    assert (n * D.CAP_WIDTH > D.cap_elements("encode_symbols_kernel")) == (n == 8193)
    _same(_symbols(g, pos, strand, D.CAP_RADIUS, 1, f"n{n}"), D.symbols_direct(g, pos, strand, D.CAP_RADIUS, 1), "symbols", f"n{n}")


@pytest.mark.parametrize("n", D.CAP_ROWS["encode_onehot_kernel"])
def test_onehot_on_and_beyond_one_round_of_the_grid(n):
    """2048 rows of 2048 columns are 16384 x 256 columns; row 2049 belongs to a second round (67 MB of output)"""
    g, pos, strand = D.cap_case(n)
    assert (n * D.CAP_WIDTH > D.cap_elements("encode_onehot_kernel")) == (n == 2049)
    _same(_onehot(g, pos, strand, D.CAP_RADIUS, 1, f"n{n}"), D.onehot_ref(g, pos, strand, D.CAP_RADIUS, 1), "one-hot", f"n{n}")


@pytest.mark.parametrize("n", D.CAP_ROWS["encode_kmer_kernel"])
def test_kmer_on_and_beyond_one_round_of_the_grid(n):
    """order 1: 1024 rows of 2048 ids are 8192 x 256 ids; row 1025 belongs to a second round"""
    g, pos, strand = D.cap_case(n)
    assert (n * D.CAP_WIDTH > D.cap_elements("encode_kmer_kernel")) == (n == 1025)
    _same(_kmer(g, pos, strand, D.CAP_RADIUS, 1, 1, f"n{n}"), D.kmer_ref(g, pos, strand, D.CAP_RADIUS, 1, 1), "k-mer ids", f"n{n}")


@pytest.mark.parametrize("n", D.CAP_ROWS["reader_windows_kernel"])
def test_substituted_symbols_on_and_beyond_one_round_of_the_grid(n):
    """mural_encode_subst_symbols, one live substitution per row: 8192 rows are 16384 x 256 units; row 8193 belongs to a second round"""
    g, pos, strand, sub_pos, sub_base = D.cap_subst(n)
    assert (n * D.CAP_WIDTH > D.cap_elements("reader_windows_kernel")) == (n == 8193)
    want = D.subst_symbols_ref(g, pos, strand, sub_pos, sub_base, D.CAP_RADIUS, 1, direct=True)
    plain = D.symbols_direct(g, pos, strand, D.CAP_RADIUS, 1)
    assert ((want != plain).sum(axis=1) <= 1).all() and (want != plain).any(axis=1).sum() > n // 2
    _same(_subst(g, pos, strand, sub_pos, sub_base, D.CAP_RADIUS, 1, f"n{n}"), want, "substituted symbols", f"n{n}")


# ================================================================================================================== training batch
class _Batch:
    """the row table and the three records on the device"""

    def __init__(self):
        t, gs = D.row_table(), D.batch_genomes()
        self.keep = [_DevGenome(g) for g in gs]
        structs = (_lib.MuralGenome * len(gs))(*[d.struct for d in self.keep])
        self.structs = torch.frombuffer(bytearray(bytes(structs)), dtype=torch.uint8).cuda()
        self.n_genomes, self.n_rows = len(gs), t.n_rows
        self.chrom, self.pos, self.strand, self.label = _dev(t.chrom), _dev(t.pos), _dev(t.strand), _dev(t.label)

    def encode(self, order, first, B, local_radius, local_order, distal_radius, indel, mode, case, status0=0):
        """(return code, dict of outputs, status); mode 'sym', 'onehot' or 'both'.  An output that is not asked for is NULL."""
        gm = D.batch_geometry(local_radius, local_order, distal_radius, indel)
        ncol, width = max(gm["ncol"], 1), gm["width_d"]
        do = _dev(np.asarray(order, np.int64))
        cat = _Guarded(B * ncol, torch.int64, D.KMER_FILL)
        sym = _Guarded(B * width, torch.uint8, D.SYM_FILL)
        ohe = _Guarded(B * 4 * width, torch.float32, D.OHE_FILL)
        y = _Guarded(B, torch.float32, D.OHE_FILL)
        status = torch.full((1,), status0, dtype=torch.int32, device="cuda")
        rc = _lib.lib().mural_train_batch_encode(
            self.structs.data_ptr(), self.n_genomes, self.chrom.data_ptr(), self.pos.data_ptr(), self.strand.data_ptr(), self.label.data_ptr(),
            self.n_rows, do.data_ptr(), len(order), first, B, local_radius, local_order, distal_radius, indel, cat.ptr,
            sym.ptr if mode != "onehot" else None, ohe.ptr if mode != "sym" else None, y.ptr, status.data_ptr(), None)
        out = dict(cat=cat.take(case).reshape(B, ncol), sym=sym.take(case).reshape(B, width), onehot=ohe.take(case).reshape(B, 4, width),
                   y=y.take(case))
        return rc, out, int(status.item())


@pytest.fixture(scope="module")
def batch():
    return _Batch()


def _batch_check(out, ref, mode, case):
    _same(out["cat"], ref["cat"], "cat", case)
    _same(out["y"], ref["y"], "labels", case)
    if mode != "onehot":
        _same(out["sym"], ref["sym"], "symbols", case)
    else:
        assert (out["sym"] == D.SYM_FILL).all(), case
    if mode != "sym":
        _same(out["onehot"], ref["onehot"], "one-hot", case)
    else:
        assert (out["onehot"].view(np.uint32) == np.float32(D.OHE_FILL).view(np.uint32)).all(), case


@pytest.mark.parametrize("label,local_radius,order,distal_radius,indel,sizes", D.batch_cases(), ids=[c[0] for c in D.batch_cases()])
def test_train_batch_encode_equals_the_oracle(batch, label, local_radius, order, distal_radius, indel, sizes):
    """rows order[first : first + B], first = 3, of a table over records of 1, 17 and 40009 bases, drawn with repeats: k-mer ids, symbols,
    one-hot columns and labels equal the oracle-built rows, with `sym_out` only, `onehot_out` only and both.  Geometries: a local window
    wider than the distal one; equal radii; orders 11 and 12 on one column; distal radius 1; distal widths 3, 5, 2, 4 with B = 1 .. 5
    (every residue of B * W mod 4: rows start at every byte alignment, two rows share a 4-byte slot); the largest distal radius whose
    staging fits 48 KB."""
    first = 3
    for B in sizes:
        rows = D.batch_order(first, B, 10 * B + distal_radius)
        ref = D.batch_ref(rows, first, B, local_radius, order, distal_radius, indel)
        for mode in ("sym", "onehot", "both"):
            case = f"{label} B{B} {mode}"
            rc, out, status = batch.encode(rows, first, B, local_radius, order, distal_radius, indel, mode, case)
            assert rc == 0 and status == ref["status"] == 0, (case, rc, status, _lib.lib().mural_last_error())
            _batch_check(out, ref, mode, case)


def test_train_batch_encode_invalid_rows(batch):
    """an order entry of -1 and of n_rows, a row whose chromosome is -1 and one whose chromosome is n_genomes: that row is all N (k-mer
    ids 4^order), its label 0, the status word holds MURAL_E_INVALID beside the bits it held, and every other row of the batch is what
    it was"""
    t = D.row_table()
    first, B = 2, 9
    rows = D.batch_order(first, B, 77)
    clean = D.batch_ref(rows, first, B, 4, 3, 2, 0)
    for at in (0, 4, 8):
        for bad in (-1, t.n_rows, -2 ** 40, 2 ** 40) + t.bad_chrom_rows:
            r2 = rows.copy()
            r2[first + at] = bad
            ref = D.batch_ref(r2, first, B, 4, 3, 2, 0)
            case = f"row {at} = {bad}"
            rc, out, status = batch.encode(r2, first, B, 4, 3, 2, 0, "both", case, status0=4)
            assert rc == 0 and ref["status"] == D.MURAL_E_INVALID and status == 4 | D.MURAL_E_INVALID, (case, rc, status)
            _batch_check(out, ref, "both", case)
            assert (out["sym"][at] == 4).all() and (out["cat"][at] == 64).all() and out["y"][at] == 0
            keep = np.arange(B) != at
            _same(out["sym"][keep], clean["sym"][keep], "other rows", case)
            _same(out["cat"][keep], clean["cat"][keep], "other rows' ids", case)
    rc, out, status = batch.encode(rows, first, B, 4, 3, 2, 0, "both", "clean", status0=4)
    assert rc == 0 and status == 4
    _batch_check(out, clean, "both", "clean")


def test_train_batch_encode_refusals_and_empty_batches(batch):
    """the distal radius past the staging limit, orders 0 and 13, an order wider than the local window, radius 0, rows beyond the order:
    a non-zero code, a message, outputs and status untouched; B = 0 is OK and writes nothing"""
    big = D.staging_boundary_radius(0)
    rows = D.batch_order(3, 5, 1)
    # (local_radius, order, distal_radius, indel, first, B, message)
    for args in ((2, 2, big + 1, 0, 3, 2, "staging"), (2, 2, big + 1000, 1, 3, 2, "staging"), (4, 0, 8, 0, 3, 5, "order"),
                 (4, 13, 8, 0, 3, 5, "order"), (5, 12, 8, 0, 3, 5, "order"), (5, 11, 8, 1, 3, 5, "order"), (0, 1, 8, 0, 3, 5, "radius"),
                 (4, 3, 0, 1, 3, 5, "radius"), (4, 3, 8, 0, 3, len(rows) - 2, "order"), (4, 3, 8, 0, len(rows) + 1, 0, "order"),
                 (4, 3, 8, 0, -1, 2, "order")):
        local_radius, order, distal_radius, indel, first, B, message = args
        gm = D.batch_geometry(max(local_radius, 1), min(max(order, 1), 12), max(distal_radius, 1), indel)      # (outputs of the full size)
        cat = _Guarded(max(B, 1) * max(gm["ncol"], 1), torch.int64, D.KMER_FILL)
        sym = _Guarded(max(B, 1) * gm["width_d"], torch.uint8, D.SYM_FILL)
        y = _Guarded(max(B, 1), torch.float32, D.OHE_FILL)
        status = torch.full((1,), 4, dtype=torch.int32, device="cuda")
        do = _dev(rows)
        rc = _lib.lib().mural_train_batch_encode(
            batch.structs.data_ptr(), batch.n_genomes, batch.chrom.data_ptr(), batch.pos.data_ptr(), batch.strand.data_ptr(),
            batch.label.data_ptr(), batch.n_rows, do.data_ptr(), len(rows), first, B, local_radius, order, distal_radius, indel, cat.ptr, sym.ptr,
            None, y.ptr, status.data_ptr(), None)
        assert rc != 0, args
        with pytest.raises(ValueError, match=message):
            _lib.check(rc)
        for buf in (cat, sym, y):
            buf.untouched(str(args))
        assert int(status.item()) == 4
    for first in (0, 3, len(rows)):
        rc, out, status = batch.encode(rows, first, 0, 4, 3, 8, 0, "both", f"B0 first {first}", status0=4)
        assert rc == 0 and status == 4
    assert _lib.lib().mural_train_batch_encode(None, 0, None, None, None, None, 0, None, 0, 0, 0, 4, 3, 8, 0, None, None, None, None, None, None) == 0


# ================================================================================================================== the Python wrappers
def test_python_wrappers_equal_the_c_entries():
    """PackedGenome.encode_symbols / encode_kmer / encode_onehot on the mixed record (packed by the product's own packer from the same
    sequence) give what the C entries give on the oracle-packed record: one mixed case per window kind"""
    from mural_amd.data import PackedGenome
    g = D.mixed_genome()
    seq = "".join(D.E.IUPAC[c] for c in g.codes)
    pg = PackedGenome.from_sequence(seq, "cuda")
    assert pg.length == g.length and np.array_equal(pg.ambiguous[0], g.amb_pos) and np.array_equal(pg.ambiguous[1], g.amb_sym)
    for radius, model_type in ((100, "snv"), (3, "indel")):
        indel = int(model_type == "indel")
        _, _, pos, strand = D.count_case(257, radius, indel)
        case = f"wrappers R{radius} {model_type}"
        _same(pg.encode_symbols(pos, strand, radius, model_type).sym.cpu().numpy(), _symbols(g, pos, strand, radius, indel, case), "symbols", case)
        _same(pg.encode_onehot(pos, strand, radius, model_type).cpu().numpy(), _onehot(g, pos, strand, radius, indel, case), "one-hot", case)
        _same(pg.encode_kmer(pos, strand, radius, 3, model_type).cpu().numpy(), _kmer(g, pos, strand, radius, 3, indel, case), "k-mer ids", case)
