"""CPU tests of the mutagenesis host twins (mural_amd/mutagenesis.py): the specification the device kernels of csrc/mutagenesis.hip are
compared with on the GPU.  The twins are judged against brute force: patch the sequence string, run the oracle encoders on it."""
import numpy as np
import pytest

from oracle import encode_ref
from tests import _mutagenesis_data as D


@pytest.mark.parametrize("cfg", D.CONFIGS)
def test_subst_encoder_twin_matches_the_patched_string(cfg):
    from mural_amd.predict import encode_subst_windows_host
    radius, lr, order = cfg
    seq = D.sequence()
    pos, strand, sub_pos, sub_base = D.substitution_cases(*D.sites(), radius, lr, order)
    want_sym, want_cat = D.brute_force(seq, pos, strand, sub_pos, sub_base, radius, lr, order)
    got_sym, got_cat = encode_subst_windows_host(seq, pos, strand, sub_pos, sub_base, radius, lr, order)
    assert got_sym.dtype == np.uint8 and got_cat.dtype == np.int64
    assert np.array_equal(got_sym, want_sym)
    assert np.array_equal(got_cat, want_cat)
    # the cases are not vacuous: some rows differ from the unchanged encodings, in the symbols and in the k-mer columns
    none = np.full_like(sub_base, 255)
    ref_sym, ref_cat = encode_subst_windows_host(seq, pos, strand, sub_pos, none, radius, lr, order)
    assert (got_sym != ref_sym).any(axis=1).sum() > 50 and (got_cat != ref_cat).any(axis=1).sum() > 20
    # a substitution changes one symbol column at the most, and at most `order` k-mer columns
    assert (got_sym != ref_sym).sum(axis=1).max() == 1 and (got_cat != ref_cat).sum(axis=1).max() <= order


def test_outermost_local_base_changes_exactly_the_outermost_kmer_column():
    from mural_amd.predict import encode_subst_windows_host
    seq, lr, order = D.sequence(), 5, 3
    pos, base = 100, (encode_ref.seq_to_codes(D.sequence())[[95, 105]] + 1) % 4
    for strand in (0, 1):
        ref = encode_subst_windows_host(seq, [pos], [strand], [0], [255], 6, lr, order)[1][0]
        first = encode_subst_windows_host(seq, [pos], [strand], [pos - lr], [base[0]], 6, lr, order)[1][0]
        last = encode_subst_windows_host(seq, [pos], [strand], [pos + lr], [base[1]], 6, lr, order)[1][0]
        ncol = len(ref)
        lo, hi = (0, ncol - 1) if strand == 0 else (ncol - 1, 0)
        assert np.nonzero(first != ref)[0].tolist() == [lo] and np.nonzero(last != ref)[0].tolist() == [hi]


def test_replacing_n_and_iupac_positions_makes_them_plain_bases():
    from mural_amd.predict import encode_subst_windows_host
    seq = D.sequence()
    for target in (D.N_RUN[0] + 3, D.IUPAC_POS):
        for strand in (0, 1):
            sym, cat = encode_subst_windows_host(seq, [target], [strand], [target], [2], 6, 5, 3)
            ref_sym, ref_cat = encode_subst_windows_host(seq, [target], [strand], [target], [255], 6, 5, 3)
            assert ref_sym[0, 6] > 3 and sym[0, 6] == (1 if strand else 2)         # G on '+', its complement C on '-'
            assert (ref_cat[0, 3:6] == 64).all()
            if target == D.IUPAC_POS:
                assert (cat[0, 3:6] < 64).all()


def test_variant_ids_map_to_site_column_alternative():
    from mural_amd.mutagenesis import mutagenesis_ids_host
    from mural_amd.predict import mutagenesis_rows_host
    seq, radius = D.sequence(), 6
    codes = encode_ref.seq_to_codes(seq)
    pos, strand = D.sites()
    W = 2 * radius + 1
    total = len(pos) * W * 3
    site, col, a = mutagenesis_ids_host(0, total, radius)
    assert np.array_equal((site * W + col) * 3 + a, np.arange(total))
    row_pos, row_strand, sub_pos, sub_base = mutagenesis_rows_host(seq, pos, strand, radius, 0, total)
    assert np.array_equal(row_pos, pos[site]) and np.array_equal(row_strand, strand[site])
    sign = np.where(strand[site] != 0, -1, 1)
    assert np.array_equal(sub_pos, pos[site] + sign * (col - radius))
    # brute force per id: the reference base on the '+' strand, the a-th other base of the WINDOW-oriented alphabet
    for v in range(total):
        g = int(sub_pos[v])
        plus = int(codes[g]) if 0 <= g < len(codes) else 4
        if plus > 3:
            assert sub_base[v] == 255
            continue
        neg = strand[site[v]] != 0
        ref_w = 3 - plus if neg else plus
        alt_w = [b for b in range(4) if b != ref_w][a[v]]
        assert sub_base[v] == (3 - alt_w if neg else alt_w)
        assert sub_base[v] != plus
    # per column the three alternatives are distinct, and on '-' rows they descend on the '+' strand
    trip = sub_base.reshape(-1, 3)
    live = trip[:, 0] != 255
    assert (trip[live, 0] != trip[live, 1]).all() and (trip[live, 1] != trip[live, 2]).all()
    neg_cols = np.repeat(strand != 0, W)
    assert (np.diff(trip[live & neg_cols].astype(int), axis=1) < 0).all() and (np.diff(trip[live & ~neg_cols].astype(int), axis=1) > 0).all()


@pytest.mark.parametrize("first,count", [(0, 1), (5, 64), (38, 101), (3 * 13 * 2 + 4, 3 * 13 + 1)])
def test_row_chunks_are_slices_of_the_whole(first, count):
    from mural_amd.predict import mutagenesis_rows_host
    seq, radius = D.sequence(), 6
    pos, strand = D.sites()
    whole = mutagenesis_rows_host(seq, pos, strand, radius, 0, len(pos) * 13 * 3)
    part = mutagenesis_rows_host(seq, pos, strand, radius, first, count)
    for w, p in zip(whole, part):
        assert np.array_equal(w[first:first + count], p)
    with pytest.raises(ValueError):
        mutagenesis_rows_host(seq, pos, strand, radius, len(pos) * 13 * 3 - 1, 2)


def _reduce_case(n_class=3, radius=6):
    from mural_amd.predict import encode_subst_windows_host
    seq = D.sequence()
    pos, strand = D.sites()
    W = 2 * radius + 1
    ref_symbols = encode_subst_windows_host(seq, pos, strand, pos, np.full(len(pos), 255, np.uint8), radius, 5, 3)[0]
    rng = np.random.default_rng(3)
    ref_logp = rng.normal(size=(len(pos), n_class)).astype(np.float32)
    var_logp = rng.normal(size=(len(pos) * W * 3, n_class)).astype(np.float32)
    return ref_symbols, ref_logp, var_logp, W


def test_reduce_semantics_zero_at_the_reference_base_nan_elsewhere_not_acgt():
    from mural_amd.mutagenesis import mutagenesis_ids_host
    from mural_amd.predict import mutagenesis_reduce_host
    ref_symbols, ref_logp, var_logp, W = _reduce_case()
    n, C = ref_logp.shape
    delta = np.full((n, W, 4, C), 7.0, np.float32)
    logp = np.full((n, W, 4, C), 7.0, np.float32)
    mutagenesis_reduce_host(ref_logp, var_logp, ref_symbols, 0, delta, logp)
    assert not (delta == 7.0).any() and not (logp == 7.0).any()                    # every element written
    site, col, a = mutagenesis_ids_host(0, len(var_logp), (W - 1) // 2)
    plain = ref_symbols < 4
    assert (~plain).any() and np.isnan(delta[~plain]).all() and np.isnan(logp[~plain]).all()
    assert not np.isnan(delta[plain]).any()
    s, c = np.nonzero(plain)
    at_ref = delta[s, c, ref_symbols[s, c]]
    assert (at_ref == 0).all() and not np.signbit(at_ref).any()                    # exactly +0.0
    assert np.array_equal(logp[s, c, ref_symbols[s, c]], ref_logp[s])
    for v in range(0, len(var_logp), 7):
        ref = int(ref_symbols[site[v], col[v]])
        if ref > 3:
            continue
        alt = [b for b in range(4) if b != ref][a[v]]
        assert np.array_equal(delta[site[v], col[v], alt], var_logp[v] - ref_logp[site[v]])
        assert np.array_equal(logp[site[v], col[v], alt], var_logp[v])


@pytest.mark.parametrize("chunk", [1, 2, 5, 64, 101])
def test_reduce_is_independent_of_chunks_that_cut_a_site_and_a_column(chunk):
    from mural_amd.predict import mutagenesis_reduce_host
    ref_symbols, ref_logp, var_logp, W = _reduce_case()
    n, C = ref_logp.shape
    whole = mutagenesis_reduce_host(ref_logp, var_logp, ref_symbols, 0, np.full((n, W, 4, C), 7.0, np.float32))
    parts = np.full((n, W, 4, C), 7.0, np.float32)
    written = np.zeros(parts.shape, np.int32)
    for first in range(0, len(var_logp), chunk):
        probe = np.full(parts.shape, 7.0, np.float32)
        mutagenesis_reduce_host(ref_logp, var_logp[first:first + chunk], ref_symbols, first, probe)
        written += probe.view(np.uint32) != np.float32(7.0).view(np.uint32)
        mutagenesis_reduce_host(ref_logp, var_logp[first:first + chunk], ref_symbols, first, parts)
    assert np.array_equal(whole.view(np.uint32), parts.view(np.uint32))
    assert (written == 1).all()                                                     # one writer per element


def test_table_rows_name_the_genomic_strand_and_top_keeps_the_most_important_columns():
    """tools/mutagenesis_files.py: the rows of a map (built here from the host twins, on CPU tensors)."""
    import importlib.util
    import io
    import os

    import torch

    from mural_amd.mutagenesis import MutagenesisMap
    from mural_amd.predict import mutagenesis_reduce_host
    spec = importlib.util.spec_from_file_location("mutagenesis_files", os.path.join(os.path.dirname(os.path.dirname(
        os.path.abspath(__file__))), "tools", "mutagenesis_files.py"))
    tool = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(tool)
    ref_symbols, ref_logp, var_logp, W = _reduce_case(n_class=2)
    pos, strand = D.sites()
    n = len(pos)
    delta = mutagenesis_reduce_host(ref_logp, var_logp, ref_symbols, 0, np.zeros((n, W, 4, 2), np.float32))
    res = MutagenesisMap(torch.from_numpy(delta), torch.from_numpy(ref_logp), torch.from_numpy(ref_symbols), None, torch.from_numpy(pos),
                         torch.from_numpy(strand), (W - 1) // 2)
    seq = D.sequence()
    out = io.StringIO()
    rows = tool.write_rows(out, "chrT", res)
    lines = [ln.split("\t") for ln in out.getvalue().splitlines()]
    assert rows == len(lines) == 3 * int((ref_symbols < 4).sum())
    for f in lines:
        chrom, site, st, off, gpos, ref, alt = f[0], int(f[1]), f[2], int(f[3]), int(f[4]), f[5], f[6]
        assert chrom == "chrT" and len(f) == 9 and gpos == site + (off if st == "+" else -off)
        assert seq[gpos] == ref and alt != ref and alt in "ACGT"                      # ref / alt on the genomic strand
    s, b = 22, 1                                                                    # a '-' site: window base C is genomic G
    j = int(np.nonzero((ref_symbols[s] < 4) & (ref_symbols[s] != b))[0][0])
    assert strand[s] == 1 and pos[s] == 77
    want = ["chrT", str(pos[s]), "-", str(j - 6), str(pos[s] - (j - 6)), seq[pos[s] - (j - 6)], "G"] + ["%.4g" % v for v in delta[s, j, b]]
    assert want in lines
    top = io.StringIO()
    assert tool.write_rows(top, "chrT", res, top=2) <= 6 * n
    imp = res.importance().numpy()
    kept = {(int(f[1]), f[2], int(f[3])) for f in (ln.split("\t") for ln in top.getvalue().splitlines())}
    for s in range(n):
        best = np.nanmax(imp[s])
        assert any(k[0] == pos[s] and k[1] == "+-"[strand[s]] and imp[s, k[2] + 6] == best for k in kept)
