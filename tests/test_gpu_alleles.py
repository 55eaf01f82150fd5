"""GPU tests of the allele path (csrc/mutagenesis.hip: mural_encode_allele_windows, mural_allele_rows; mural_amd/mutagenesis.py:
allele_footprint): the encoder bit for bit against the plain encoders on the patched genome and against its
numpy twin, the enumerator against its twin, the footprint against ``variant_footprint`` (1-for-1 alleles), against the float64 oracle
on windows of the patched string, and against its own contracts (NaN placement, chunking), the errors, tools/allele_files.py."""
import os

import numpy as np
import pytest
import torch

from oracle import encode_ref
from tests import _alleles_data as A
from tests import _mutagenesis_data as D

pytestmark = pytest.mark.gpu

SNV = [(cfg, "snv") for cfg in D.CONFIGS]
INDEL = [((R, None, None), "indel") for R in A.INDEL_RADII]


def _bits(t):
    return t.contiguous().view(torch.int32)


def device_table(tab=None):
    from mural_amd.mutagenesis import Alleles
    p, d, k, alt = A.table() if tab is None else tab
    return Alleles(*(torch.from_numpy(np.ascontiguousarray(a)).cuda() for a in (p, d, k, alt.view(np.int64))))


# ----------------------------------------------------------------------------------------------------------------------------------
# encoder
# ----------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cfg,model_type", SNV + INDEL)
def test_allele_encoder_equals_the_plain_encoders_on_the_patched_genome(cfg, model_type):
    """W = 13 and 201 (SNV) end rows inside a 4-byte group: the byte tail of the dword path; W = 12 and 200 (INDEL) keep every group
    in one row: the aligned path."""
    from mural_amd.data import PackedGenome
    from mural_amd.mutagenesis import _encode_allele_into, encode_allele_windows_host
    radius, lr, order = cfg
    indel = model_type == "indel"
    seq = D.sequence()
    genome = PackedGenome.from_sequence(seq, "cuda")
    before = [t.clone() for t in (genome.packed2, genome.nmask, genome.amb_pos, genome.amb_sym)]
    table = device_table()
    pos, strand, allele = A.rows_for(radius, lr, order, model_type)
    got_sym, got_cat = genome.encode_allele_windows(pos, strand, allele, table, radius, lr, order, model_type)
    W = 2 * radius + (0 if indel else 1)
    assert got_sym.dtype == torch.uint8 and got_sym.shape == (len(pos), W)
    if indel:
        assert got_cat is None
    else:
        assert got_cat.dtype == torch.int64 and got_cat.shape == (len(pos), 2 * lr + 1 - (order - 1))
    # the plain encoders on PackedGenome.from_sequence(patched), the rows grouped by their patched text
    groups = {}
    for i, v in enumerate(allele.tolist()):
        groups.setdefault(A.patched(seq, v), []).append(i)
    assert len(groups) == len(A.LIVE)                             # (the identity and the alleles that are not live share the plain text)
    want_sym = torch.empty_like(got_sym)
    want_cat = None if indel else torch.empty_like(got_cat)
    for text, rows in groups.items():
        g2 = PackedGenome.from_sequence(text, "cuda")
        idx = torch.tensor(rows, device="cuda")
        want_sym[idx] = g2.encode_symbols(pos[rows], strand[rows], radius, model_type).sym
        if not indel:
            want_cat[idx] = g2.encode_kmer(pos[rows], strand[rows], lr, order)
    assert torch.equal(got_sym, want_sym)
    assert indel or torch.equal(got_cat, want_cat)
    # ... and the numpy twin the CPU tests pin against the oracle encoders
    host_sym, host_cat = encode_allele_windows_host(seq, pos, strand, allele, A.table(), radius, lr, order, model_type)
    assert np.array_equal(got_sym.cpu().numpy(), host_sym) and (indel or np.array_equal(got_cat.cpu().numpy(), host_cat))
    # either output alone
    t = [torch.as_tensor(pos, device="cuda"), torch.as_tensor(strand, device="cuda"), torch.as_tensor(allele, device="cuda")]
    only_sym = torch.zeros_like(got_sym)
    _encode_allele_into(genome, *t, table, radius, int(indel), lr or 0, order or 0, only_sym, None)
    assert torch.equal(only_sym, got_sym)
    if not indel:
        only_cat = torch.zeros_like(got_cat)
        _encode_allele_into(genome, *t, table, radius, 0, lr, order, None, only_cat)
        assert torch.equal(only_cat, got_cat)
    # no rows: nothing launched, empty outputs; an empty table: every row is the plain window
    e_sym, e_cat = genome.encode_allele_windows(pos[:0], strand[:0], allele[:0], table, radius, lr, order, model_type)
    assert e_sym.shape == (0, W) and (indel or e_cat.shape[0] == 0)
    no_table = device_table(tuple(a[:0] for a in A.table()))
    plain, _ = genome.encode_allele_windows(pos, strand, allele, no_table, radius, lr, order, model_type)
    assert torch.equal(plain, genome.encode_symbols(pos, strand, radius, model_type).sym)
    torch.cuda.synchronize()
    for b, t in zip(before, (genome.packed2, genome.nmask, genome.amb_pos, genome.amb_sym)):
        assert torch.equal(b, t)                                                      # the genome's device buffers are unchanged


# ----------------------------------------------------------------------------------------------------------------------------------
# enumerator
# ----------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("radius,model_type", [(6, "snv"), (100, "snv"), (6, "indel"), (100, "indel")])
def test_allele_enumerator_matches_the_host_twin(radius, model_type):
    from mural_amd.data import PackedGenome
    from mural_amd.mutagenesis import allele_rows, allele_rows_host
    genome = PackedGenome.from_sequence(D.sequence(), "cuda")
    table = device_table()
    strand = (np.arange(len(table)) % 2).astype(np.uint8) * 3
    slots = 2 * radius - (1 if model_type == "indel" else 0)
    total = len(table) * slots
    want = allele_rows_host(A.LENGTH, A.table(), strand, radius, 0, total, model_type)
    assert (want[3] == -1).any() and (want[3] >= 0).any() and (want[0] != want[1]).any()
    for step in (1, 97, total):                                   # chunks of 1 and 97 cut alleles
        if step == 1 and radius == 100:
            continue
        parts = [allele_rows(genome, table, strand, radius, first, min(step, total - first), model_type) for first in range(0, total, step)]
        got = [torch.cat([p[k] for p in parts]).cpu().numpy() for k in range(4)]
        for g, w in zip(got, want):
            assert g.dtype == w.dtype and np.array_equal(g, w), step
    for bad in ((total - 1, 2), (-1, 1), (total + 1, 0)):
        with pytest.raises(ValueError):
            allele_rows(genome, table, strand, radius, *bad, model_type)
    assert allele_rows(genome, table, strand, radius, total, 0, model_type)[0].shape == (0,)


# ----------------------------------------------------------------------------------------------------------------------------------
# footprint, SNV
# ----------------------------------------------------------------------------------------------------------------------------------
def _oracle_windows(text_codes, p, neg, r, R):
    st = ["-" if neg else "+"]
    return encode_ref.kmer_encode(text_codes, [p], st, r, 3)[0], encode_ref.onehot_encode(text_codes, [p], st, R)[0]


@pytest.mark.parametrize("model_no", [2, 1])
def test_snv_allele_footprint(model_no):
    from mural_amd.data import PackedGenome
    from mural_amd.mutagenesis import Alleles, allele_footprint, allele_footprint_offsets, alternate_sequence, variant_footprint
    from tests import test_gpu_mutagenesis as G
    from tests.test_gpu_snv import assert_probs_close
    r, R = 5, 100
    seq = G.map_sequence()
    L = len(seq)
    codes = encode_ref.seq_to_codes(seq)
    genome = PackedGenome.from_sequence(seq, "cuda")
    model, orc = G.build_models(r, R, model_no)
    slots = 2 * R

    # 1. alleles with d = k = 1 are variant_footprint's entries for d != 0, bit for bit
    var_pos = np.array([1000, 1000, 30, L - 40, G.MAP_N_RUN[0] - 5, 3000], np.int64)
    strand = np.array([0, 1, 1, 0, 1, 0], np.uint8)
    var_base = ((codes[var_pos] + np.array([1, 2, 3, 1, 2, 0])) % 4).astype(np.uint8)
    subst = Alleles.from_host(var_pos, np.ones(len(var_pos), np.int64), ["ACGT"[b] for b in var_base], "cuda")
    t_strand = torch.from_numpy(strand).cuda()
    fp, focal = allele_footprint(model, genome, subst, t_strand, local_radius=r, local_order=3)
    assert fp.shape == (len(var_pos), slots, 4) and fp.dtype == torch.float32 and focal.shape == (len(var_pos), slots) and focal.dtype == torch.uint8
    old, old_focal = variant_footprint(model, genome, torch.from_numpy(var_pos).cuda(), torch.from_numpy(var_base).cuda(), t_strand,
                                       local_radius=r, local_order=3)
    keep = torch.arange(2 * R + 1, device="cuda") != R
    assert torch.equal(_bits(fp), _bits(old[:, keep])) and torch.equal(focal, old_focal[:, keep])
    assert bool(torch.isnan(fp[2]).any()) and bool(torch.isfinite(fp[0]).all()) and bool((_bits(fp[5]) == 0).all())
    e = allele_footprint_offsets(R, "snv").numpy()
    assert np.array_equal(e, np.arange(-R, R))

    # 2. length-changing alleles: chunking, NaN placement, the oracle
    cases = [(1000, 0, "A"), (1500, 0, "CGTTGCA"), (2000, 1, ""), (2600, 7, ""), (3100, 2, "ACGTA"), (3500, 4, "G"), (40, 3, "TGA"),
             (L - 30, 0, "ACGTTGCAAGCTTCGATCGGATCCATGCAGTA"), (G.MAP_N_RUN[0] - 3, 10, "T"), (G.MAP_IUPAC, 1, "")]
    dead = [(L - 2, 5, "A"), (-4, 1, "C")]                        # not live: p + d > length, p < 0
    rows = cases + dead
    a_strand = (np.arange(len(rows)) % 2).astype(np.uint8)
    table = Alleles.from_host([p for p, _, _ in rows], [d for _, d, _ in rows], [a for _, _, a in rows], "cuda")
    ts = torch.from_numpy(a_strand).cuda()
    fp, focal = allele_footprint(model, genome, table, ts, local_radius=r, local_order=3)
    for chunk in (333, 1000):                                     # both cut alleles; the default is one chunk here
        other = allele_footprint(model, genome, table, ts, local_radius=r, local_order=3, chunk_windows=chunk)
        assert torch.equal(_bits(other[0]), _bits(fp)) and torch.equal(other[1], focal), chunk
    assert bool(torch.isnan(fp[len(cases):]).all())               # every row of an allele that is not live
    picks, cats, xs = [], [], []
    rng = np.random.default_rng(model_no)
    for i, (p, d, alt) in enumerate(cases):
        k, neg = len(alt), bool(a_strand[i])
        ref_pos = np.where(e < 0, p + e, p + d + e)
        alt_pos = np.where(e < 0, ref_pos, ref_pos + k - d)
        inside = (ref_pos >= 0) & (ref_pos < L)
        assert bool(torch.isnan(fp[i][torch.from_numpy(~inside).cuda()]).all()) and bool(torch.isfinite(fp[i][torch.from_numpy(inside).cuda()]).all())
        assert i not in (6, 7) or (~inside).any()                 # the two alleles near the chromosome ends
        want_focal = np.where(inside, codes[np.clip(ref_pos, 0, L - 1)], 4)
        want_focal = np.where(neg, np.array([3, 2, 1, 0, 4, 6, 5, 10, 8, 9, 7, 14, 13, 12, 11])[want_focal], want_focal)
        assert np.array_equal(focal[i].cpu().numpy(), want_focal)
        assert float(fp[i][torch.from_numpy(inside).cuda()].abs().max()) > 0
        # the oracle on both haplotypes at: both ends of the reach, the slots next to the allele, the edges of the local window, seeded others
        text = encode_ref.seq_to_codes(alternate_sequence(seq, p, d, alt))
        take = np.unique(np.r_[[0, 1, R - r - 1, R - r, R - 2, R - 1, R, R + 1, R + r - 1, R + r, slots - 2, slots - 1], rng.choice(slots, 6, replace=False)])
        for c in take[inside[take]].tolist():
            for codes_h, site in ((text, int(alt_pos[c])), (codes, int(ref_pos[c]))):
                cat, x = _oracle_windows(codes_h, site, neg, r, R)
                cats.append(cat)
                xs.append(x)
            picks.append((i, c))
    with torch.no_grad():
        want = orc((torch.zeros(len(xs), 1, dtype=torch.float64), torch.from_numpy(np.stack(cats))), torch.from_numpy(np.stack(xs))).numpy()
    want_alt, want_ref = want[0::2], want[1::2]
    # the footprint's own two forwards, row by row through the same entries: the probabilities against the oracle, and delta is ONE float32
    # subtraction of them (the bar test_gpu_mutagenesis.py applies to its map: bit equality with var_logp - ref_logp)
    ii, cc = (np.array(c) for c in zip(*picks))
    p_all, d_all, k_all = (np.array([x[j] if j < 2 else len(x[2]) for x in rows])[ii] for j in range(3))
    ref_pos = np.where(e[cc] < 0, p_all + e[cc], p_all + d_all + e[cc])
    alt_pos = np.where(e[cc] < 0, ref_pos, ref_pos + k_all - d_all)
    with torch.no_grad():
        sym, cat = genome.encode_allele_windows(alt_pos, a_strand[ii], ii, table, R, r, 3)
        got_alt = model.forward_symbols(cat if model_no == 2 else None, sym)
        sym, cat = genome.encode_allele_windows(ref_pos, a_strand[ii], np.full(len(ii), -1), table, R, r, 3)
        got_ref = model.forward_symbols(cat if model_no == 2 else None, sym)
    err = np.abs(np.exp(got_alt.cpu().numpy().astype(np.float64)) - np.exp(want_alt)).max()
    print(f"allele footprint Network{model_no}: {len(picks)} oracle row pairs, max prob err on the alternate haplotype {err:.3e}, "
          f"largest |delta| {np.abs(want_alt - want_ref).max():.3e}")
    assert_probs_close(got_alt.cpu().numpy(), want_alt, model_no, f"alternate haplotype Network{model_no}")
    assert_probs_close(got_ref.cpu().numpy(), want_ref, model_no, f"reference haplotype Network{model_no}")
    got = fp[torch.from_numpy(ii).cuda(), torch.from_numpy(cc).cuda()]
    assert torch.equal(_bits(got), _bits(got_alt - got_ref))
    assert np.abs(want_alt - want_ref).max() > 1e-2               # (the alleles do move the rates: the comparison is not of zeros)
    # empty table
    none = Alleles.from_host([], [], [], "cuda")
    fp0, focal0 = allele_footprint(model, genome, none, ts[:0], local_radius=r, local_order=3)
    assert fp0.shape == (0, slots, 4) and focal0.shape == (0, slots)


# ----------------------------------------------------------------------------------------------------------------------------------
# footprint, UNet_Small
# ----------------------------------------------------------------------------------------------------------------------------------
def test_indel_allele_footprint():
    from mural_amd.data import PackedGenome
    from mural_amd.mutagenesis import Alleles, allele_footprint, allele_footprint_offsets, alternate_sequence, variant_footprint
    from tests import test_gpu_mutagenesis_indel as GI
    model, orc, R = GI.models("indel_synth_small.npz")
    seq = GI.map_sequence()
    L = len(seq)
    codes = encode_ref.seq_to_codes(seq)
    genome = PackedGenome.from_sequence(seq, "cuda")
    slots = 2 * R - 1
    e = allele_footprint_offsets(R, "indel").numpy()
    assert np.array_equal(e, np.arange(-R, R - 1))
    # a homopolymer-like contraction and expansion, unequal lengths, one near each end, one over the N run; two that are not live
    cases = [(1000, 0, "A"), (1200, 0, "CGTTGCA"), (2000, 1, ""), (1700, 7, ""), (900, 2, "ACGTA"), (40, 3, "TGA"),
             (L - 30, 0, "ACGTTGCAAGCTTCGATCGGATCCATGCAGTA"), (GI.MAP_N_RUN[0] - 3, 10, "T")]
    dead = [(L - 2, 5, "A"), (-4, 1, "C")]
    rows = cases + dead
    a_strand = (np.arange(len(rows)) % 2).astype(np.uint8)
    table = Alleles.from_host([p for p, _, _ in rows], [d for _, d, _ in rows], [a for _, _, a in rows], "cuda")
    ts = torch.from_numpy(a_strand).cuda()
    fp, focal = allele_footprint(model, genome, table, ts, distal_radius=R)
    assert fp.shape == (len(rows), slots, model.n_class) and fp.dtype == torch.float32 and focal.shape == (len(rows), slots) and focal.dtype == torch.uint8
    assert bool(torch.isnan(fp[len(cases):]).all())
    rng = np.random.default_rng(R)
    xs, picks = [], []
    for i, (p, d, alt) in enumerate(cases):
        k, neg = len(alt), bool(a_strand[i])
        ref_pos = np.where(e < 0, p + e, p + d + e)
        alt_pos = np.where(e < 0, ref_pos, ref_pos + k - d)
        inside = (ref_pos >= 0) & (ref_pos < L)
        assert bool(torch.isnan(fp[i][torch.from_numpy(~inside).cuda()]).all()) and bool(torch.isfinite(fp[i][torch.from_numpy(inside).cuda()]).all())
        assert i not in (5, 6) or (~inside).any()
        text = encode_ref.seq_to_codes(alternate_sequence(seq, p, d, alt))
        take = np.unique(np.r_[[0, 1, R - 2, R - 1, R, R + 1, slots - 2, slots - 1], rng.choice(slots, 4, replace=False)])
        st = ["-" if neg else "+"]
        for c in take[inside[take]].tolist():
            xs.append(encode_ref.onehot_encode(text, [int(alt_pos[c])], st, R, "indel")[0])
            xs.append(encode_ref.onehot_encode(codes, [int(ref_pos[c])], st, R, "indel")[0])
            picks.append((i, c))
    with torch.no_grad():
        scores = orc(torch.from_numpy(np.stack(xs))).double()
    logp = torch.log_softmax(scores, dim=1).numpy()
    want = logp[0::2] - logp[1::2]
    bar = 4.0 * GI.SCORE_BAR * max(1.0, float(scores.abs().max()))            # section 3.28's rule: 4 x the forward's score bar
    ii, cc = (torch.tensor(c, device="cuda") for c in zip(*picks))
    got = fp[ii, cc].cpu().numpy().astype(np.float64)
    err = float(np.abs(got - want).max())
    print(f"INDEL allele footprint: {len(picks)} oracle row pairs, max |delta - oracle| {err:.3e}, bar {bar:.3e}, largest |delta| {np.abs(want).max():.3e}")
    assert err <= bar
    assert np.abs(want).max() > 10 * bar
    # another chunking: the same NaN placement, values within the bar (the INDEL forward picks kernels by the size of a call)
    other = allele_footprint(model, genome, table, ts, distal_radius=R, chunk_windows=1000)
    assert torch.equal(torch.isnan(other[0]), torch.isnan(fp)) and torch.equal(other[1], focal)
    assert float((other[0] - fp).nan_to_num().abs().max()) <= bar
    # substitution alleles against variant_footprint (entries d != 0), within the same bar
    var_pos = np.array([1000, 1000, 30, L - 40], np.int64)
    strand = np.array([0, 1, 1, 0], np.uint8)
    var_base = ((codes[var_pos] + np.array([1, 2, 3, 1])) % 4).astype(np.uint8)
    subst = Alleles.from_host(var_pos, np.ones(len(var_pos), np.int64), ["ACGT"[b] for b in var_base], "cuda")
    t_strand = torch.from_numpy(strand).cuda()
    new, new_focal = allele_footprint(model, genome, subst, t_strand, distal_radius=R)
    old, old_focal = variant_footprint(model, genome, torch.from_numpy(var_pos).cuda(), torch.from_numpy(var_base).cuda(), t_strand, distal_radius=R)
    keep = torch.arange(2 * R, device="cuda") != R                # variant_footprint's own-site entry d = 0 sits at index R
    assert torch.equal(torch.isnan(new), torch.isnan(old[:, keep])) and torch.equal(new_focal, old_focal[:, keep])
    diff = float((new - old[:, keep]).nan_to_num().abs().max())
    print(f"INDEL substitution alleles vs variant_footprint: max |difference| {diff:.3e} (bar {bar:.3e})")
    assert diff <= bar and float(new.nan_to_num().abs().max()) > 0


# ----------------------------------------------------------------------------------------------------------------------------------
# errors
# ----------------------------------------------------------------------------------------------------------------------------------
def test_unsupported_models_and_inputs_raise_with_the_reason():
    from mural_amd.data import PackedGenome
    from mural_amd.mutagenesis import Alleles, allele_footprint
    from tests import test_gpu_mutagenesis as G
    genome = PackedGenome.from_sequence(G.map_sequence(), "cuda")
    table = Alleles.from_host([1000, 2000], [0, 3], ["AC", ""], "cuda")
    strand = torch.tensor([0, 1], dtype=torch.uint8, device="cuda")
    net0, _ = G.build_models(5, 100, 0)
    with pytest.raises(RuntimeError, match="Network0"):
        allele_footprint(net0, genome, table, strand)
    model, _ = G.build_models(5, 100, 2)
    model.train()
    with pytest.raises(RuntimeError, match="eval mode"):
        allele_footprint(model, genome, table, strand)
    model.eval()
    with pytest.raises(RuntimeError, match="HIP device"):
        allele_footprint(model, genome, table, strand.cpu())
    with pytest.raises(RuntimeError, match="HIP device"):
        allele_footprint(model, genome, Alleles.from_host([1000, 2000], [0, 3], ["AC", ""], "cpu"), strand)
    on_cpu = G.build_models(5, 100, 1)[0].cpu()
    with pytest.raises(RuntimeError, match="HIP device"):
        allele_footprint(on_cpu, genome, table, strand)
    with pytest.raises(ValueError):
        allele_footprint(model, genome, table, strand, chunk_windows=0)
    with pytest.raises(ValueError):
        allele_footprint(model, genome, table, strand[:1])
    with pytest.raises(TypeError):
        allele_footprint(model, genome, (table.pos, table.ref_len, table.alt_len, table.alt), strand)
    from tests import test_gpu_mutagenesis_indel as GI
    indel, _, R = GI.models("indel_synth_small.npz")
    with pytest.raises(ValueError, match="distal_radius"):
        allele_footprint(indel, genome, table, strand)
    from mural_amd import _lib
    assert _lib.lib().mural_abi_version() == 4


# ----------------------------------------------------------------------------------------------------------------------------------
# tools/allele_files.py
# ----------------------------------------------------------------------------------------------------------------------------------
def test_allele_files_tool_writes_the_footprint_table_and_counts_what_it_skips(tmp_path, capsys):
    import importlib.util
    from mural_amd.data import PackedGenome
    from mural_amd.model import nn_utils
    from mural_amd.mutagenesis import Alleles, allele_footprint
    from tests import test_gpu_mutagenesis as G
    r, R, order = 5, 100, 3
    model, _ = G.build_models(r, R, 2)
    ncol = 2 * r + 1 - (order - 1)
    config = dict(local_radius=r, local_order=order, local_hidden1_size=150, local_hidden2_size=75, distal_radius=R, emb_dropout=0.1,
                  local_dropout=0.1, CNN_kernel_size=3, CNN_out_channels=32, distal_fc_dropout=0.25, n_class=4, model_no=2, seq_only=True,
                  emb_dims=[(4 ** order + 1, 2)] * ncol)
    nn_utils.save_model(model, None, config, str(tmp_path / "model"))
    seq = G.map_sequence()
    with open(tmp_path / "ref.fa", "w") as fh:
        fh.write(">chrT test\n" + "\n".join(seq[i:i + 60] for i in range(0, len(seq), 60)) + "\n>other\nACGT\n")
    s = seq
    wrong = "A" if s[699] != "A" else "C"
    lines = [
        "##fileformat=VCFv4.2",
        "#CHROM\tPOS\tID\tREF\tALT",
        f"chrT\t1001\t.\t{s[1000]}\t{s[1000]}ACG\t.\t.",                              # an anchored insertion before 0-based 1001
        f"chrT\t1501\t.\t{s[1500:1504]}\t{s[1500]}\t.\t.",                            # an anchored deletion of 1501..1503
        f"chrT\t2001\t.\t{s[2000:2002]}\tTTT,<DEL>\t.\t.",                            # 2-for-3, and a symbolic allele
        f"chrT\t31\t.\t{s[30]}\t{'ACGT'[('ACGT'.index(s[30]) + 1) % 4]}\t.\t.",       # a substitution near the chromosome start
        f"chrT\t3001\t.\t{s[3000]}\t*\t.\t.",                                         # the overlapping-deletion allele
        f"chrT\t3101\t.\t{s[3100]}\t{s[3100]}NA\t.\t.",                               # an inserted N
        f"chrT\t3201\t.\t{s[3200]}\t{s[3200]}{'ACGT' * 8}A\t.\t.",                    # 33 bases after trimming
        f"chrT\t700\t.\t{wrong}\tG\t.\t.",                                            # REF is not what the FASTA holds
    ]
    assert len(lines) == 10
    with open(tmp_path / "variants.vcf", "w") as fh:
        fh.write("\n".join(lines) + "\n")
    spec = importlib.util.spec_from_file_location("allele_files", os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))),
                                                                               "tools", "allele_files.py"))
    tool = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(tool)
    summary = tool.main(["--ref_genome", str(tmp_path / "ref.fa"), "--variants", str(tmp_path / "variants.vcf"), "--model_path",
                         str(tmp_path / "model"), "--out", str(tmp_path / "out"), "--strand", "both"])
    assert summary["skipped"] == dict(symbolic=2, non_acgt=1, too_long=1, ref_mismatch=1) and summary["alleles"] == 4
    printed = capsys.readouterr().out
    assert "symbolic 2" in printed and "non_acgt 1" in printed and "too_long 1" in printed and "ref_mismatch 1" in printed
    table = [ln.rstrip("\n").split("\t") for ln in open(tmp_path / "out.allele_footprint.tsv")]
    assert table[0] == ["chrom", "variant_pos", "ref", "alt", "site_pos", "strand", "focal"] + [f"delta_logp{c}" for c in (1, 2, 3, 4)]
    # the same four alleles through allele_footprint
    sub_alt = "ACGT"[("ACGT".index(s[30]) + 1) % 4]
    kept = [(1001, 0, "ACG", 1001, s[1000], s[1000] + "ACG"), (1501, 3, "", 1501, s[1500:1504], s[1500]),
            Alleles.from_vcf_fields(2001, s[2000:2002], "TTT") + (2001, s[2000:2002], "TTT"), (30, 1, sub_alt, 31, s[30], sub_alt)]
    both = [(a, st) for a in kept for st in (0, 1)]
    alleles = Alleles.from_host([a[0] for a, _ in both], [a[1] for a, _ in both], [a[2] for a, _ in both], "cuda")
    genome = PackedGenome.from_sequence(seq, "cuda")
    fp, focal = allele_footprint(model, genome, alleles, torch.tensor([st for _, st in both], dtype=torch.uint8, device="cuda"), r, order)
    fp, focal = fp.cpu().numpy(), focal.cpu().numpy()
    e = np.arange(-R, R)
    want = []
    for i, ((p, d, _, pos1, ref, alt), st) in enumerate(both):
        site = np.where(e < 0, p + e, p + d + e)
        for c in range(2 * R):
            if 0 <= site[c] < len(seq):
                want.append(["chrT", str(pos1), ref, alt, str(site[c]), "-" if st else "+", "ACGTNRYMSWKBDHV"[focal[i, c]]] + ["%.4g" % v for v in fp[i, c]])
    assert summary["rows"] == len(want) == len(table) - 1 and len(want) < 8 * 2 * R        # (the substitution's reach leaves the chromosome)
    assert table[1:] == want
