"""CPU tests of the allele path's specification (mural_amd/mutagenesis.py): the numpy twins
``encode_allele_windows_host`` / ``allele_rows_host`` against brute force (patch the sequence string, run the oracle encoders at the
alternate-haplotype position), the reachability property the enumerator rests on, and the host-side validation of ``Alleles``."""
import numpy as np
import pytest

from tests import _alleles_data as A
from tests import _mutagenesis_data as D

SNV = [(cfg, "snv") for cfg in D.CONFIGS]
INDEL = [((R, None, None), "indel") for R in A.INDEL_RADII]


@pytest.mark.parametrize("cfg,model_type", SNV + INDEL)
def test_encoder_twin_equals_the_oracle_encoders_on_the_patched_string(cfg, model_type):
    from mural_amd.mutagenesis import alternate_sequence, encode_allele_windows_host
    radius, lr, order = cfg
    seq = D.sequence()
    pos, strand, allele = A.rows_for(radius, lr, order, model_type)
    got_sym, got_cat = encode_allele_windows_host(seq, pos, strand, allele, A.table(), radius, lr, order, model_type)
    want_sym, want_cat = A.brute_force(seq, pos, strand, allele, radius, lr, order, model_type)
    W = 2 * radius + (1 if model_type == "snv" else 0)
    assert got_sym.dtype == np.uint8 and got_sym.shape == (len(pos), W)
    assert np.array_equal(got_sym, want_sym)
    if model_type == "snv":
        assert got_cat.dtype == np.int64 and np.array_equal(got_cat, want_cat)
    else:
        assert got_cat is None
    # the cases are not vacuous: most live alleles change rows, rows of alleles that are not live and of "no allele" equal the plain windows
    plain, _ = encode_allele_windows_host(seq, pos, strand, np.full_like(allele, -1), A.table(), radius, lr, order, model_type)
    n_live = len(A.LIVE)
    dead = (allele < 0) | (allele >= n_live)
    assert np.array_equal(got_sym[dead], plain[dead]) and dead.sum() > 200
    changed = {int(v) for v in allele[(got_sym != plain).any(axis=1)]}
    assert changed == set(range(n_live - 1)), sorted(changed)                      # every live allele but the identity (the last one)
    # alternate_sequence is the patch the brute force applied
    rows = A.LIVE + A.NOT_LIVE
    for v, (p, d, alt) in enumerate(rows):
        assert alternate_sequence(seq, p, d, alt) == A.patched(seq, v)
    assert len(alternate_sequence(seq, *A.LIVE[2])) == len(seq) + 32 and alternate_sequence(seq, 5, 0, "A" * 33) == seq


@pytest.mark.parametrize("cfg", D.CONFIGS)
def test_a_one_for_one_allele_is_the_substitution_encoder(cfg):
    from mural_amd.mutagenesis import encode_allele_windows_host, encode_subst_windows_host
    radius, lr, order = cfg
    seq = D.sequence()
    p, d, alt = A.LIVE[A.SUBST_CASE]
    assert d == 1 and len(alt) == 1
    pos = np.arange(p - radius - 2, p + radius + 3, dtype=np.int64)
    pos = np.r_[pos, pos]
    strand = np.r_[np.zeros(len(pos) // 2, np.uint8), np.ones(len(pos) // 2, np.uint8)]
    got = encode_allele_windows_host(seq, pos, strand, np.full(len(pos), A.SUBST_CASE), A.table(), radius, lr, order)
    want = encode_subst_windows_host(seq, pos, strand, np.full(len(pos), p), np.full(len(pos), "ACGT".index(alt), np.uint8), radius, lr, order)
    assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1])
    assert (got[0] != encode_subst_windows_host(seq, pos, strand, pos, np.full(len(pos), 255, np.uint8), radius, lr, order)[0]).any()


def _rows_by_definition(length, radius, model_type, strand):
    """worked out here from the issue's definition, one Python loop, not through the twin"""
    a_pos, a_d, a_k, _ = A.table()
    off0, W = (-radius, 2 * radius + 1) if model_type == "snv" else (-radius + 1, 2 * radius)
    out = []
    for v in range(len(a_pos)):
        p, d, k = int(a_pos[v]), int(a_d[v]), int(a_k[v])
        live = 0 <= p and 0 <= d and p + d <= length and 0 <= k <= 32
        if not live:
            d = k = 0
        for c in range(W - 1):
            e = c - (off0 + W - 1)
            ref = p + e if e < 0 else p + d + e
            alt = ref if e < 0 else ref + k - d
            out.append((ref, alt, int(strand[v] != 0), v if live else -1))
    return np.array(out, np.int64)


@pytest.mark.parametrize("radius,model_type", [(6, "snv"), (100, "snv"), (6, "indel"), (100, "indel")])
def test_enumerator_twin_is_the_definition(radius, model_type):
    from mural_amd.mutagenesis import allele_footprint_offsets, allele_rows_host
    tab = A.table()
    strand = (np.arange(len(tab[0])) % 2).astype(np.uint8) * 3               # any nonzero byte is '-'
    want = _rows_by_definition(A.LENGTH, radius, model_type, strand)
    slots = 2 * radius if model_type == "snv" else 2 * radius - 1
    total = len(tab[0]) * slots
    assert len(want) == total
    for step in (1, 97, total):
        parts = [allele_rows_host(A.LENGTH, tab, strand, radius, first, min(step, total - first), model_type) for first in range(0, total, step)]
        got = [np.concatenate([p[k] for p in parts]) for k in range(4)]
        assert got[0].dtype == np.int64 and got[1].dtype == np.int64 and got[2].dtype == np.uint8 and got[3].dtype == np.int64
        for k in range(4):
            assert np.array_equal(got[k].astype(np.int64), want[:, k]), (step, k)
    assert (want[:, 3] == -1).sum() == (len(A.NOT_LIVE) + 1) * slots
    e = allele_footprint_offsets(radius, model_type).numpy()
    assert np.array_equal(e, np.arange(-radius, radius if model_type == "snv" else radius - 1)) and len(e) == slots
    for bad in ((total - 1, 2), (-1, 1), (0, -1)):
        with pytest.raises(ValueError):
            allele_rows_host(A.LENGTH, tab, strand, radius, *bad, model_type)


@pytest.mark.parametrize("radius,model_type", [(6, "snv"), (100, "snv"), (6, "indel"), (100, "indel")])
def test_sites_outside_the_enumerated_set_see_the_same_window_on_both_haplotypes(radius, model_type):
    """The reachability property: a surviving site (outside [p, p + d)) that the enumerator does not name has identical reference and
    alternate windows on both strands, chromosome ends included -- and the set is tight: every slot is needed by some allele."""
    from mural_amd.mutagenesis import allele_rows_host, encode_allele_windows_host
    seq = D.sequence()
    tab = A.table()
    slots = 2 * radius if model_type == "snv" else 2 * radius - 1
    needed = np.zeros(slots, bool)
    for v, (p, d, alt) in enumerate(A.LIVE):
        k = len(alt)
        ref_pos, alt_pos, _, row_allele = allele_rows_host(A.LENGTH, tab, np.zeros(len(tab[0]), np.uint8), radius, v * slots, slots, model_type)
        assert (row_allele == v).all()
        s = np.arange(-3, A.LENGTH + 3, dtype=np.int64)
        s = s[(s < p) | (s >= p + d)]                                              # the sites that survive the allele
        on_alt = np.where(s < p, s, s + k - d)
        # the enumerated rows pair each surviving site of the set with its position on the alternate haplotype
        named = np.isin(s, ref_pos)
        lookup = dict(zip(ref_pos.tolist(), alt_pos.tolist()))
        assert all(lookup[int(a)] == int(b) for a, b in zip(s[named], on_alt[named]))
        for strand in (0, 1):
            st = np.full(len(s), strand, np.uint8)
            ref_w, _ = encode_allele_windows_host(seq, s, st, np.full(len(s), -1), tab, radius, 3, 1, model_type)
            alt_w, _ = encode_allele_windows_host(seq, on_alt, st, np.full(len(s), v), tab, radius, 3, 1, model_type)
            differs = (ref_w != alt_w).any(axis=1)
            assert not differs[~named].any(), (v, strand, s[~named][differs[~named]])
            if strand == 0:
                needed |= np.isin(ref_pos, s[differs])
    assert needed.all()


def test_alleles_from_host_validates_and_packs():
    import torch
    from mural_amd.mutagenesis import Alleles
    tab = Alleles.from_host([5, 9, 0], [0, 2, 1], ["ACGT", "", "t"], "cpu")
    assert len(tab) == 3 and all(t.dtype == torch.int64 for t in (tab.pos, tab.ref_len, tab.alt_len, tab.alt))
    p, d, k, alt = tab.host()
    assert p.tolist() == [5, 9, 0] and d.tolist() == [0, 2, 1] and k.tolist() == [4, 0, 1]
    assert alt.dtype == np.uint64 and alt.tolist() == [0b11100100, 0, 3]
    full = Alleles.from_host([1], [0], ["T" * 32], "cpu")
    assert full.host()[3].tolist() == [2 ** 64 - 1] and int(full.alt[0]) == -1       # the uint64 bit pattern in an int64 tensor
    live = A.LIVE
    mine = Alleles.from_host([p for p, _, _ in live], [d for _, d, _ in live], [a for _, _, a in live], "cpu").host()
    for got, want in zip(mine, A.table()):
        assert np.array_equal(got, want[:len(live)])
    for bad in (([1], [0], ["A" * 33]), ([1], [0], ["ACN"]), ([1], [0], ["AR"]), ([1], [-1], ["A"]), ([1, 2], [0], ["A"])):
        with pytest.raises(ValueError):
            Alleles.from_host(*bad, "cpu")


def test_from_vcf_fields_trims_the_anchor_and_the_shared_suffix():
    from mural_amd.mutagenesis import Alleles
    f = Alleles.from_vcf_fields
    assert f(10, "A", "ACG") == (10, 0, "CG")                     # an anchored insertion: before 0-based 10
    assert f(10, "ACG", "A") == (10, 2, "")                       # an anchored deletion
    assert f(10, "AC", "AC") == (11, 0, "")                       # identical: the identity
    assert f(10, "A", "G") == (9, 1, "G")
    assert f(10, "ACG", "TCA") == (9, 3, "TCA")                   # an MNV: nothing shared
    assert f(10, "ACGT", "AGGT") == (10, 1, "G")                  # prefix and suffix
    assert f(10, "CAA", "CA") == (11, 1, "")                      # a repeat contraction: the prefix takes what both ends could
    assert f(10, "ca", "cat") == (11, 0, "T")
    assert f(1, "GT", "T") == (0, 1, "")                          # no shared prefix: the suffix is trimmed
