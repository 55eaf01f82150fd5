"""CPU tests of the mutagenesis host twins on the INDEL window ([pos - R + 1, pos + R], W = 2 R; mural_amd/mutagenesis.py with
``model_type="indel"``): the specification the window-generic kernels of csrc/mutagenesis.hip are compared with on the GPU.  The twins
are judged against brute force: patch the sequence string, run ``oracle/encode_ref.onehot_encode(.., "indel")`` on it."""
import numpy as np
import pytest

from oracle import encode_ref
from tests import _mutagenesis_data as D

RADII = [6, 100]


def _cases(pos, strand, radius):
    """Rows (pos, strand, sub_pos, sub_base) for every site: the substitution at window column 0, at column W - 1, at the focal base, next
    to it, inside the N run, on the IUPAC position, just outside the window on both sides, outside the record, and 255 / 4."""
    rows = []
    for p, s in zip(pos.tolist(), strand.tolist()):
        first, last = p - radius + 1, p + radius                     # '+'-strand ends of the window: column 0 / W - 1 on '+', swapped on '-'
        targets = [first, last, p, p + 1, D.N_RUN[0] + 3, D.IUPAC_POS, first - 1, last + 1, -1, D.LENGTH, D.LENGTH + 7, -radius]
        for k, t in enumerate(targets):
            rows.append((p, s, t, (k + p) % 4))
        rows.append((p, s, p, 255))
        rows.append((p, s, p + 1, 4))
    a = np.array(rows, np.int64)
    return a[:, 0].copy(), a[:, 1].astype(np.uint8), a[:, 2].copy(), a[:, 3].astype(np.uint8)


def _brute_force(seq, pos, strand, sub_pos, sub_base, radius):
    syms, cache = [], {}
    for p, s, sp, sb in zip(pos.tolist(), strand.tolist(), sub_pos.tolist(), sub_base.tolist()):
        text = D.patched(seq, sp, sb)
        if text not in cache:
            cache[text] = encode_ref.seq_to_codes(text)
        syms.append(D.symbols_of_onehot(encode_ref.onehot_encode(cache[text], [p], ["-" if s else "+"], radius, "indel"))[0])
    return np.stack(syms)


@pytest.mark.parametrize("radius", RADII)
def test_subst_encoder_twin_matches_the_patched_string(radius):
    from mural_amd.mutagenesis import encode_subst_windows_host
    seq = D.sequence()
    pos, strand, sub_pos, sub_base = _cases(*D.sites(), radius)
    want = _brute_force(seq, pos, strand, sub_pos, sub_base, radius)
    got, cat = encode_subst_windows_host(seq, pos, strand, sub_pos, sub_base, radius, model_type="indel")
    assert cat is None and got.dtype == np.uint8 and got.shape == (len(pos), 2 * radius)
    assert np.array_equal(got, want)
    ref, _ = encode_subst_windows_host(seq, pos, strand, sub_pos, np.full_like(sub_base, 255), radius, model_type="indel")
    changed = got != ref
    assert changed.any(axis=1).sum() > 50 and changed.sum(axis=1).max() == 1
    # the named columns: per site the first three rows substitute window column 0 / W - 1 ('+'; swapped on '-') and the focal base
    per = 14
    W = 2 * radius
    for i in range(0, len(pos), per):
        neg = strand[i] != 0
        for k, col in ((0, W - 1 if neg else 0), (1, 0 if neg else W - 1), (2, radius if neg else radius - 1)):
            hit = np.nonzero(changed[i + k])[0].tolist()
            assert hit in ([], [col])              # ([]: the substitute equals the reference base, or the position is outside the record)
        for k in (6, 7, 8, 9, 10, 12, 13):         # outside the window, outside the record, no substitution
            if k in (6, 7) or sub_pos[i + k] < 0 or sub_pos[i + k] >= D.LENGTH or sub_base[i + k] > 3:
                assert not changed[i + k].any()
    cols = {int(np.nonzero(c)[0][0]) for c in changed if c.any()}
    assert {0, W - 1, radius - 1, radius} <= cols


def test_unsupported_model_type_is_refused():
    from mural_amd.mutagenesis import encode_subst_windows_host, mutagenesis_rows_host
    with pytest.raises(ValueError):
        encode_subst_windows_host(D.sequence(), [5], [0], [5], [1], 6, model_type="sv")
    with pytest.raises(ValueError):
        mutagenesis_rows_host(D.sequence(), [5], [0], 6, 0, 1, model_type="sv")


@pytest.mark.parametrize("radius", RADII)
def test_variant_ids_map_to_site_column_alternative(radius):
    from mural_amd.mutagenesis import mutagenesis_ids_host, mutagenesis_rows_host
    seq = D.sequence()
    codes = encode_ref.seq_to_codes(seq)
    pos, strand = D.sites()
    W = 2 * radius
    total = len(pos) * W * 3
    site, col, a = mutagenesis_ids_host(0, total, radius, "indel")
    assert np.array_equal((site * W + col) * 3 + a, np.arange(total))
    row_pos, row_strand, sub_pos, sub_base = mutagenesis_rows_host(seq, pos, strand, radius, 0, total, "indel")
    assert np.array_equal(row_pos, pos[site]) and np.array_equal(row_strand, strand[site])
    neg = strand[site] != 0
    assert np.array_equal(sub_pos, np.where(neg, pos[site] + radius - col, pos[site] - radius + 1 + col))
    plus = np.where((sub_pos >= 0) & (sub_pos < len(codes)), codes[np.clip(sub_pos, 0, len(codes) - 1)], 4).astype(int)
    for v in range(0, total, 7 if radius > 6 else 1):
        if plus[v] > 3:
            assert sub_base[v] == 255
            continue
        ref_w = 3 - plus[v] if neg[v] else plus[v]
        alt_w = [b for b in range(4) if b != ref_w][a[v]]
        assert sub_base[v] == (3 - alt_w if neg[v] else alt_w) and sub_base[v] != plus[v]
    # every id's row, encoded, differs from the site's reference window in exactly its own column (or in none where there is no base)
    from mural_amd.mutagenesis import encode_subst_windows_host
    pick = np.arange(0, total, 11 if radius > 6 else 1)
    got, _ = encode_subst_windows_host(seq, row_pos[pick], row_strand[pick], sub_pos[pick], sub_base[pick], radius, model_type="indel")
    ref, _ = encode_subst_windows_host(seq, row_pos[pick], row_strand[pick], sub_pos[pick], np.full(len(pick), 255, np.uint8), radius,
                                       model_type="indel")
    diff = got != ref
    live = sub_base[pick] != 255
    assert np.array_equal(diff.sum(axis=1), live.astype(int))
    assert np.array_equal(np.argmax(diff[live], axis=1), col[pick][live])


@pytest.mark.parametrize("first,count", [(0, 1), (5, 64), (38, 101), (3 * 12 * 2 + 4, 3 * 12 + 1)])
def test_row_chunks_are_slices_of_the_whole(first, count):
    from mural_amd.mutagenesis import mutagenesis_rows_host
    seq, radius = D.sequence(), 6
    pos, strand = D.sites()
    whole = mutagenesis_rows_host(seq, pos, strand, radius, 0, len(pos) * 12 * 3, "indel")
    part = mutagenesis_rows_host(seq, pos, strand, radius, first, count, "indel")
    for w, p in zip(whole, part):
        assert np.array_equal(w[first:first + count], p)
    with pytest.raises(ValueError):
        mutagenesis_rows_host(seq, pos, strand, radius, len(pos) * 12 * 3 - 1, 2, "indel")


@pytest.mark.parametrize("radius", RADII)
def test_reduce_twin_on_an_even_window(radius):
    from mural_amd.mutagenesis import encode_subst_windows_host, mutagenesis_reduce_host
    seq, n_class = D.sequence(), 3
    pos, strand = D.sites()
    W = 2 * radius
    ref_symbols = encode_subst_windows_host(seq, pos, strand, pos, np.full(len(pos), 255, np.uint8), radius, model_type="indel")[0]
    rng = np.random.default_rng(3)
    ref_logp = rng.normal(size=(len(pos), n_class)).astype(np.float32)
    var_logp = rng.normal(size=(len(pos) * W * 3, n_class)).astype(np.float32)
    whole = np.full((len(pos), W, 4, n_class), 7.0, np.float32)
    mutagenesis_reduce_host(ref_logp, var_logp, ref_symbols, 0, whole)
    # brute force, element by element
    want = np.empty_like(whole)
    for s in range(len(pos)):
        for j in range(W):
            ref = int(ref_symbols[s, j])
            if ref > 3:
                want[s, j] = np.nan
                continue
            alts = [b for b in range(4) if b != ref]
            want[s, j, ref] = 0.0
            for a, b in enumerate(alts):
                want[s, j, b] = var_logp[(s * W + j) * 3 + a] - ref_logp[s]
    assert np.array_equal(whole, want, equal_nan=True)
    assert not np.signbit(whole[~np.isnan(whole) & (whole == 0)]).any()
    # chunks that start and end mid-site and mid-column write every element once
    parts = np.full_like(whole, 7.0)
    total = len(var_logp)
    cuts = [0, 1, 5, 3 * W + 2, 3 * W * 5 + 1, total]
    for lo, hi in zip(cuts[:-1], cuts[1:]):
        mutagenesis_reduce_host(ref_logp, var_logp[lo:hi], ref_symbols, lo, parts)
    assert np.array_equal(parts, whole, equal_nan=True)


def test_log_softmax_twin():
    from mural_amd.mutagenesis import log_softmax_host
    rng = np.random.default_rng(0)
    s = np.abs(rng.normal(size=(50, 8))) * 5
    got = log_softmax_host(s)
    assert got.dtype == np.float64 and np.allclose(np.exp(got).sum(axis=1), 1.0, rtol=0, atol=1e-12)
    assert np.allclose(got - got[:, :1], s - s[:, :1], rtol=0, atol=1e-12)
    big = log_softmax_host(np.array([[1000.0, 0.0], [0.0, 0.0]]))
    assert np.isfinite(big).all() and big[0, 0] == 0.0 and np.allclose(big[1], np.log(0.5))


def test_genomic_positions_follow_the_indel_window():
    import torch
    from mural_amd.mutagenesis import MutagenesisMap, mutagenesis_rows_host
    seq, radius = D.sequence(), 6
    pos, strand = D.sites()
    W = 2 * radius
    res = MutagenesisMap(None, None, None, None, torch.from_numpy(pos), torch.from_numpy(strand), radius, "indel")
    gp = res.genomic_positions().numpy()
    sub_pos = mutagenesis_rows_host(seq, pos, strand, radius, 0, len(pos) * W * 3, "indel")[2]
    assert np.array_equal(gp, sub_pos.reshape(len(pos), W, 3)[:, :, 0])
    snv = MutagenesisMap(None, None, None, None, torch.from_numpy(pos), torch.from_numpy(strand), radius)
    sign = np.where(strand != 0, -1, 1)
    assert np.array_equal(snv.genomic_positions().numpy(), pos[:, None] + sign[:, None] * np.arange(-radius, radius + 1)[None, :])
