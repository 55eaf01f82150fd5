"""What tests/_encode_edges_data.py promises about its inputs and references, checked on the CPU before a GPU sees them: the restated
references against oracle/encode_ref.py, the uniqueness of the one-hot inversion, the base-set complement against "one-hot column
reversed", and that every family holds what it names (residues, side-table sizes, the cap arithmetic, the staging boundary)."""
import numpy as np
import pytest

from oracle import encode_ref as E
from tests import _encode_edges_data as D


# ------------------------------------------------------------------------------------------------------------------ references
def test_onehot_rows_are_distinct_and_the_inversion_is_the_identity_on_codes():
    rows = {E._OHE[c].tobytes() for c in range(15)}
    assert len(rows) == 15 and len(E.IUPAC) == 15
    codes = np.arange(15, dtype=np.uint8)[None, :]
    assert np.array_equal(D.symbols_from_onehot(np.ascontiguousarray(E._OHE[codes].transpose(0, 2, 1))), codes)
    bad = np.ascontiguousarray(E._OHE[codes].transpose(0, 2, 1)).copy()
    bad[0, 0, 3] = 0.75
    with pytest.raises(AssertionError):
        D.symbols_from_onehot(bad)


def test_base_set_complement_is_the_reversed_onehot_column():
    """the complement of a code is the code whose one-hot column is this code's column read backwards (A<->T, C<->G): what
    encode_ref.onehot_encode does on '-'.  Pairs: A-T, C-G, R-Y, M-K, B-V, D-H; N, S, W are their own."""
    flipped = np.ascontiguousarray(E._OHE[:, ::-1][None].transpose(0, 2, 1))
    assert np.array_equal(D.symbols_from_onehot(flipped)[0], D.COMPLEMENT)
    name = {c: i for i, c in enumerate(E.IUPAC)}
    for a, b in ("AT", "CG", "RY", "MK", "BV", "DH", "NN", "SS", "WW"):
        assert D.COMPLEMENT[name[a]] == name[b] and D.COMPLEMENT[name[b]] == name[a]
    assert np.array_equal(D.COMPLEMENT[D.COMPLEMENT], np.arange(15))


def _small_cases():
    g = D.all_codes_genome()
    yield (g,) + D.edge_sites(g.length, 3) + (3, 0)
    yield (g,) + D.edge_sites(g.length, 100) + (100, 1)
    for radius, indel in ((1, 0), (2, 1), (3, 0), (100, 1)):
        for n in (5, 64):
            yield D.count_case(n, radius, indel)[1:] + (radius, indel)
        for name in ("L1 iupac", "L17 iupac", "L33 n", "L65 N run"):
            g = D.genome_named(name)
            yield (g,) + D.edge_sites(g.length, radius) + (radius, indel)


def test_symbol_references_agree_and_a_broken_complement_is_seen():
    """the inversion of the oracle's one-hot output equals the direct form on the small cases; with one IUPAC pair of the complement
    table swapped back (R and Y left uncomplemented) the direct form differs on the case that holds every code on '-'"""
    seen = set()
    for g, pos, strand, radius, indel in _small_cases():
        want = D.symbols_ref(g, pos, strand, radius, indel)
        assert np.array_equal(D.symbols_direct(g, pos, strand, radius, indel), want), (g, radius, indel)
        assert np.array_equal(E._OHE[want].transpose(0, 2, 1), D.onehot_ref(g, pos, strand, radius, indel))
        seen.update(np.unique(want[strand != 0]).tolist())
    assert seen == set(range(15))                      # every symbol is read on the '-' strand
    broken = D.COMPLEMENT.copy()
    broken[5], broken[6] = 5, 6
    g = D.all_codes_genome()
    pos, strand = D.edge_sites(g.length, 100)
    assert not np.array_equal(D.symbols_direct(g, pos, strand, 100, 1, complement=broken), D.symbols_ref(g, pos, strand, 100, 1))


def test_substitution_reference():
    """no substitution = the plain window; a live substitution changes exactly its column, to the base on '+' and its complement on '-';
    the direct and the one-hot orientation agree; every kind of row occurs"""
    for radius, indel in ((1, 0), (3, 1), (100, 0)):
        label, g, pos, strand, sub_pos, sub_base = D.subst_case(64, radius, indel)
        plain = D.symbols_ref(g, pos, strand, radius, indel)
        none = np.full(64, 255, np.uint8)
        assert np.array_equal(D.subst_symbols_ref(g, pos, strand, sub_pos, none, radius, indel), plain)
        want = D.subst_symbols_ref(g, pos, strand, sub_pos, sub_base, radius, indel)
        assert np.array_equal(D.subst_symbols_ref(g, pos, strand, sub_pos, sub_base, radius, indel, direct=True), want)
        win, hit = D.subst_windows(g, pos, strand, sub_pos, sub_base, radius, indel)
        off, width = D.window(radius, indel)
        assert (hit.sum(axis=1) <= 1).all() and 0 < hit.any(axis=1).sum() < 64
        for i in range(64):
            cols = np.nonzero(want[i] != plain[i])[0]
            if hit[i].any():
                j = int(np.nonzero(hit[i])[0][0])
                col = width - 1 - j if strand[i] else j
                assert want[i, col] == (3 - sub_base[i] if strand[i] else sub_base[i]) and set(cols) <= {col}
            else:
                assert len(cols) == 0
        on_masked = hit.any(axis=1) & (g.codes[np.clip(sub_pos, 0, g.length - 1)] >= 4)
        assert radius < 100 or on_masked.any()


# ------------------------------------------------------------------------------------------------------------------ genomes
def test_genomes_hold_what_they_name():
    gs = D.genomes()
    assert len({g.name for g in gs}) == len(gs)
    lengths = {g.length for g in gs}
    assert lengths == set(D.SMALL_LENGTHS) | {D.BIG_LENGTH} and D.BIG_LENGTH % 32 not in (0, 16) and D.BIG_LENGTH % 16 != 0
    for g in gs:
        assert np.array_equal(E.unpack_codes(g.packed, g.mask, g.length), np.where(g.codes > 4, 4, g.codes))
        assert len(g.packed) == (g.length + 15) // 16 and len(g.mask) == (g.length + 31) // 32
        assert np.array_equal(g.amb_sym, g.codes[g.amb_pos]) and (np.diff(g.amb_pos) > 0).all()
        assert len(g.amb_pos) == 0 or (g.amb_sym.min() >= 5 and g.amb_sym.max() <= 14)
    for n in D.SMALL_LENGTHS:
        g = D.genome_named(f"L{n} n")
        assert g.codes[0] == 4 and g.codes[-1] == 4 and len(g.amb_pos) == 0
        g = D.genome_named(f"L{n} iupac")
        assert g.codes[0] > 4 and g.codes[-1] > 4 and g.amb_pos[0] == 0 and g.amb_pos[-1] == n - 1
        assert (D.genome_named(f"L{n} acgt").codes < 4).all()
    for name in ("L65 N run", f"L{D.BIG_LENGTH} N run"):
        g = D.genome_named(name)
        assert (g.codes[27:37] == 4).all() and g.codes[26] < 4 and g.codes[37] < 4          # bits 27 .. 31 of word 0, 0 .. 4 of word 1
    g = D.genome_named(f"L{D.BIG_LENGTH} N run")
    assert g.codes[-1] == 4 and (g.codes[4988:] == 4).all() and 4992 % 32 == 0
    sizes = []
    for g in gs:
        if "side table" in g.name:
            k = len(g.amb_pos)
            sizes.append(k)
            assert (g.codes == 4).sum() >= 18
            if k >= 2:
                assert g.amb_pos[0] == 0 and g.amb_pos[-1] == g.length - 1
            if k >= 5:
                assert (np.diff(g.amb_pos) == 1).sum() >= 3                                   # 0, 1, 2 and length - 2, length - 1
                assert g.codes[3] == 4 and g.codes[g.length - 3] == 4                         # N next to an entry: masked, not in the table
            if k >= 10:
                assert set(g.amb_sym.tolist()) == set(range(5, 15))
    assert sorted(sizes) == sorted(D.SIDE_TABLE_SIZES + [1])
    assert D.genome_named(f"L{D.BIG_LENGTH} side table 1 first").amb_pos[0] == 0
    assert D.genome_named(f"L{D.BIG_LENGTH} side table 1 last").amb_pos[0] == D.BIG_LENGTH - 1
    assert len(D.mixed_genome().amb_pos) == 65


def test_edge_sites_reach_the_edges():
    for g in D.genomes():
        for radius, indel in D.GEOMETRIES:
            pos, strand = D.edge_sites(g.length, radius)
            off, width = D.window(radius, indel)
            assert {0, 1, g.length - 2, g.length - 1} <= set(pos.tolist())
            assert set(strand[pos == 0].tolist()) == {0, 1} and (strand[::2] == 0).all() and (strand[1::2] == 1).all()
            lo, hi = pos + off, pos + off + width
            assert (hi <= 0).any() and (lo >= g.length).any()                                 # wholly outside, on either side
            win = E.gather_windows(g.codes, pos, radius, D.mt(indel))
            assert (win[hi <= 0] == 4).all() and (win[lo >= g.length] == 4).all()
            if g.length + 2 <= width:
                assert ((lo < 0) & (hi > g.length)).any()                                     # over both ends at once
            for m in range(0, g.length + 1, 16):
                if m <= 64 or m >= g.length - 64:
                    assert {m - 1, m, m + 1} <= set(pos.tolist())
    assert D.window(1, 0) == (-1, 3) and D.window(1, 1) == (0, 2) and D.window(1000, 0) == (-1000, 2001)


def test_row_counts_take_every_residue_and_alignment():
    assert D.ROW_COUNTS == [1, 2, 3, 4, 5, 7, 64, 257] and D.RADII == [1, 2, 3, 100, 1000]
    for radius in D.RADII:
        width = D.window(radius, 0)[1]
        assert width % 2 == 1
        assert {n * width % 4 for n in D.ROW_COUNTS} == {0, 1, 2, 3}                          # the tail of the last group of 4 bytes
        assert {b * width % 4 for b in range(7)} == {0, 1, 2, 3}                              # rows start at every byte alignment
        assert D.window(radius, 1)[1] % 2 == 0
    assert {D.window(r, i)[1] % 4 for r, i in D.GEOMETRIES} == {0, 1, 2, 3}
    _, g, pos, strand = D.count_case(257, 100, 0)
    assert set(strand.tolist()) == {0, 1} and (pos < 0).any() and (pos >= g.length).any()


# ------------------------------------------------------------------------------------------------------------------ k-mer
def test_kmer_geometries_and_rejections():
    for order in D.ORDERS:
        geoms = D.kmer_geometries(order)
        ncols = [n for _, _, n in geoms]
        assert 2 in ncols and (1 in ncols) == (order >= 2) and max(ncols) >= 21 - (order - 1) - 1
        for radius, indel, ncol in geoms:
            assert ncol == D.window(radius, indel)[1] - (order - 1) >= 1
    assert D.ORDERS == list(range(1, 13))
    for radius, order, indel in D.KMER_REJECTED:
        assert radius < 1 or order < 1 or order > 12 or order > D.window(radius, indel)[1]
    assert {o for _, o, _ in D.KMER_REJECTED} >= {0, 13}
    assert any(1 <= o <= 12 and r >= 1 and o > D.window(r, i)[1] for r, o, i in D.KMER_REJECTED)
    # the sentinel, and a bad symbol on '-', are in the cases: the first column of "L17 iupac" on '-' reads the last base
    g = D.genome_named("L17 iupac")
    pos, strand = D.edge_sites(g.length, 6)
    ids = D.kmer_ref(g, pos, strand, 6, 12, 1)
    assert ids.shape[1] == 1 and (ids == 4 ** 12).any() and (ids < 4 ** 12).any() and (ids[strand != 0] < 4 ** 12).any()


# ------------------------------------------------------------------------------------------------------------------ caps
def test_cap_cases_land_on_and_cross_each_cap():
    assert D.window(D.CAP_RADIUS, 1)[1] == D.CAP_WIDTH == 2048
    assert D.cap_elements("encode_symbols_kernel") == 2 ** 24 and D.cap_elements("encode_onehot_kernel") == 2 ** 22
    assert D.cap_elements("encode_kmer_kernel") == 2 ** 21 and D.cap_elements("reader_windows_kernel") == 2 ** 24
    for kernel, (on, over) in D.CAP_ROWS.items():
        ncol = D.CAP_WIDTH                       # k-mer: order 1, one id per column
        assert on * ncol == D.cap_elements(kernel), kernel
        assert over == on + 1 and over * ncol > D.cap_elements(kernel), kernel
    assert 2049 * 4 * 2048 * 4 < 68 * 10 ** 6    # the largest output of the suite's encoder cases
    g, pos, strand, sub_pos, sub_base = D.cap_subst(8193)
    off, width = D.window(D.CAP_RADIUS, 1)
    assert ((sub_pos >= pos + off) & (sub_pos < pos + off + width) & (sub_pos >= 0) & (sub_pos < g.length) & (sub_base < 4)).all()
    acgt = g.codes[sub_pos] < 4
    assert (sub_base[acgt] != g.codes[sub_pos][acgt]).all() and (~acgt).any()
    g, pos, strand = D.cap_case(8193)
    assert set(strand.tolist()) == {0, 1} and (pos < 0).any() and (pos > g.length).any()


# ------------------------------------------------------------------------------------------------------------------ training batch
def test_batch_geometries_and_the_staging_boundary():
    big = D.staging_boundary_radius(0)
    gm, over = D.batch_geometry(2, 2, big, 0), D.batch_geometry(2, 2, big + 1, 0)
    assert gm["lds"] <= D.TB_LDS_LIMIT < over["lds"] and gm["span"] == 2 * big + 1
    assert (gm["span"] // 16 + 2 + gm["span"] // 32 + 2) * 4 + gm["span"] == gm["lds"]
    cases = {c[0]: c for c in D.batch_cases()}
    gm = D.batch_geometry(*cases["local wider than distal"][1:5])
    assert gm["lo"] == gm["off_l"] < gm["off_d"] and gm["span"] == gm["width_l"] > gm["width_d"]
    gm = D.batch_geometry(*cases["equal radii"][1:5])
    assert gm["off_l"] == gm["off_d"] and gm["width_l"] == gm["width_d"] == gm["span"]
    assert D.batch_geometry(*cases["order 12, ncol 1"][1:5])["ncol"] == 1 and cases["order 12, ncol 1"][2] == 12
    assert D.batch_geometry(*cases["order 11, ncol 1"][1:5])["ncol"] == 1
    assert cases["distal radius 1"][3] == 1
    widths = {D.batch_geometry(*c[1:5])["width_d"] % 4: c[5] for c in cases.values() if c[0].startswith("distal width")}
    assert set(widths) == {0, 1, 2, 3} and all(b == (1, 2, 3, 4, 5) for b in widths.values())
    assert any(c[3] == big for c in cases.values())
    # a span that starts at the last position of a word touches span / 16 + 2 words: such a row is in the table
    t = D.row_table()
    for c in cases.values():
        gm = D.batch_geometry(*c[1:5])
        g_lo = t.pos[:t.n_valid] + gm["lo"]
        words = ((g_lo + gm["span"] - 1) >> 4) - (g_lo >> 4) + 1
        assert words.max() <= gm["span"] // 16 + 2
    gm = D.batch_geometry(4, 3, 110, 0)
    assert ((((t.pos + gm["lo"] + gm["span"] - 1) >> 4) - ((t.pos + gm["lo"]) >> 4) + 1) == gm["span"] // 16 + 2).any()


def test_row_table_and_batch_reference():
    t, gs = D.row_table(), D.batch_genomes()
    assert [g.length for g in gs] == [1, 17, 40009] and gs[1].codes[-1] == 4 and gs[1].codes[0] > 4 and gs[0].codes[0] > 4
    assert set(t.chrom[:t.n_valid].tolist()) == {0, 1, 2} and t.chrom[t.bad_chrom_rows[0]] == -1 and t.chrom[t.bad_chrom_rows[1]] == 3
    assert set(t.label.tolist()) == {0, 1, 2, 3} and (t.pos < 0).any()
    order = D.batch_order(3, 37, 1)
    assert len(order) == 42 and set(t.chrom[order[3:40]].tolist()) == {0, 1, 2} and len(set(order[3:40].tolist())) < 37
    ref = D.batch_ref(order, 3, 37, 4, 3, 110, 0)
    assert ref["status"] == 0 and ref["cat"].shape == (37, 7) and ref["sym"].shape == (37, 221) and ref["onehot"].shape == (37, 4, 221)
    # row by row the single-call references of the same site
    for b in (0, 17, 36):
        r = order[3 + b]
        g = gs[t.chrom[r]]
        assert np.array_equal(ref["sym"][b], D.symbols_direct(g, t.pos[r:r + 1], t.strand[r:r + 1], 110, 0)[0])
        assert np.array_equal(ref["cat"][b], E.kmer_encode(g.codes, t.pos[r:r + 1], ["-" if t.strand[r] else "+"], 4, 3)[0])
        assert ref["y"][b] == t.label[r]
    # an invalid entry: that row all N, label 0, status; the others as before
    for bad in (-1, t.n_rows) + t.bad_chrom_rows:
        o2 = order.copy()
        o2[3 + 20] = bad
        r2 = D.batch_ref(o2, 3, 37, 4, 3, 110, 0)
        assert r2["status"] == D.MURAL_E_INVALID and (r2["sym"][20] == 4).all() and (r2["onehot"][20] == 0.25).all()
        assert (r2["cat"][20] == 64).all() and r2["y"][20] == 0
        keep = np.arange(37) != 20
        assert all(np.array_equal(r2[k][keep], ref[k][keep]) for k in ("cat", "sym", "onehot", "y"))
