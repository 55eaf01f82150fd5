"""GPU tests of the saturation-mutagenesis path (csrc/mutagenesis.hip, mural_amd/mutagenesis.py): the substitution encoder bit for bit
against the plain encoders on a patched genome, the enumerator against its numpy twin, the map against the float64 oracle on patched
windows and against its own contracts (one subtraction, +0.0, NaN, chunk independence), the footprint against the map, the errors."""
import numpy as np
import pytest
import torch

from oracle import encode_ref, snv_ref, synth
from tests import _mutagenesis_data as D

pytestmark = pytest.mark.gpu

NAN_BITS = 0x7FC00000


def _bits(t):
    return t.contiguous().view(torch.int32)


# ----------------------------------------------------------------------------------------------------------------------------------
# encoder
# ----------------------------------------------------------------------------------------------------------------------------------
def check_encoder(cfg):
    from mural_amd.data import PackedGenome
    from mural_amd.mutagenesis import _encode_subst_into, encode_subst_windows_host
    radius, lr, order = cfg
    seq = D.sequence()
    genome = PackedGenome.from_sequence(seq, "cuda")
    before = [t.clone() for t in (genome.packed2, genome.nmask, genome.amb_pos, genome.amb_sym)]
    pos, strand, sub_pos, sub_base = D.substitution_cases(*D.sites(), radius, lr, order)
    got_sym, got_cat = genome.encode_subst_windows(pos, strand, sub_pos, sub_base, radius, lr, order)
    assert got_sym.dtype == torch.uint8 and got_sym.shape == (len(pos), 2 * radius + 1)
    assert got_cat.dtype == torch.int64 and got_cat.shape == (len(pos), 2 * lr + 1 - (order - 1))
    # the plain encoders on PackedGenome.from_sequence(patched), the rows grouped by their patched text
    groups = {}
    for i, (sp, sb) in enumerate(zip(sub_pos.tolist(), sub_base.tolist())):
        groups.setdefault(D.patched(seq, sp, sb), []).append(i)
    assert len(groups) > 50
    want_sym, want_cat = torch.empty_like(got_sym), torch.empty_like(got_cat)
    for text, rows in groups.items():
        g2 = PackedGenome.from_sequence(text, "cuda")
        idx = torch.tensor(rows, device="cuda")
        want_sym[idx] = g2.encode_symbols(pos[rows], strand[rows], radius).sym
        want_cat[idx] = g2.encode_kmer(pos[rows], strand[rows], lr, order)
    assert torch.equal(got_sym, want_sym)
    assert torch.equal(got_cat, want_cat)
    # ... and the numpy twin the CPU tests pin against the oracle encoders
    host_sym, host_cat = encode_subst_windows_host(seq, pos, strand, sub_pos, sub_base, radius, lr, order)
    assert np.array_equal(got_sym.cpu().numpy(), host_sym) and np.array_equal(got_cat.cpu().numpy(), host_cat)
    # either output alone
    dev = dict(device="cuda")
    t = [torch.as_tensor(pos, **dev), torch.as_tensor(strand, **dev), torch.as_tensor(sub_pos, **dev), torch.as_tensor(sub_base, **dev)]
    only_sym, only_cat = torch.zeros_like(got_sym), torch.zeros_like(got_cat)
    _encode_subst_into(genome, *t, radius, lr, order, only_sym, None)
    _encode_subst_into(genome, *t, radius, lr, order, None, only_cat)
    assert torch.equal(only_sym, got_sym) and torch.equal(only_cat, got_cat)
    # no rows: nothing launched, empty outputs
    e_sym, e_cat = genome.encode_subst_windows(pos[:0], strand[:0], sub_pos[:0], sub_base[:0], radius, lr, order)
    assert e_sym.shape == (0, 2 * radius + 1) and e_cat.shape[0] == 0
    torch.cuda.synchronize()
    for b, t in zip(before, (genome.packed2, genome.nmask, genome.amb_pos, genome.amb_sym)):
        assert torch.equal(b, t)                                                      # the genome's device buffers are unchanged


@pytest.mark.parametrize("cfg", D.CONFIGS)
def test_subst_encoder_equals_the_plain_encoders_on_the_patched_genome(cfg):
    check_encoder(cfg)


# ----------------------------------------------------------------------------------------------------------------------------------
# enumerator
# ----------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("radius,chunk", [(6, 1), (6, 64), (6, 97), (6, None), (100, 1009), (100, None)])
def test_enumerator_matches_the_host_twin(radius, chunk):
    from mural_amd.data import PackedGenome
    from mural_amd.mutagenesis import mutagenesis_rows, mutagenesis_rows_host
    seq = D.sequence()
    genome = PackedGenome.from_sequence(seq, "cuda")
    pos, strand = D.sites()
    total = len(pos) * (2 * radius + 1) * 3
    want = mutagenesis_rows_host(seq, pos, strand, radius, 0, total)
    assert (want[3] == 255).any() and (want[3] != 255).any()
    step = total if chunk is None else chunk
    parts = [mutagenesis_rows(genome, pos, strand, radius, first, min(step, total - first)) for first in range(0, total, step)]
    got = [torch.cat([p[k] for p in parts]).cpu().numpy() for k in range(4)]
    for g, w in zip(got, want):
        assert g.dtype == w.dtype and np.array_equal(g, w)
    with pytest.raises(ValueError):
        mutagenesis_rows(genome, pos, strand, radius, total - 1, 2)


# ----------------------------------------------------------------------------------------------------------------------------------
# map
# ----------------------------------------------------------------------------------------------------------------------------------
MAP_LENGTH = 5000
MAP_N_RUN = (2400, 2420)
MAP_IUPAC = 2500


def map_sequence():
    rng = np.random.default_rng(11)
    raw = rng.choice(np.frombuffer(b"ACGT", np.uint8), size=MAP_LENGTH)
    raw[MAP_N_RUN[0]:MAP_N_RUN[1]] = ord("N")
    raw[MAP_IUPAC] = ord("Y")
    return raw.tobytes().decode()


def build_models(r, R, model_no, seed=77):
    from tests.test_gpu_snv import product_from_hp
    orc = snv_ref.build(model_no, local_radius=r, distal_radius=R)
    sd = synth.synth_state_dict(orc.state_dict(), seed)
    orc.load_state_dict(sd)
    orc.eval()
    model, _ = product_from_hp(np.array([r, 3, R, 150, 75, 32, 3, 4, model_no]))
    model.load_state_dict(sd)
    return model.cuda().eval(), orc


def _variant(codes, p, neg, j, a, R):
    """(genomic position, '+'-strand alternative, window-orientation alternative) of id (site at p, column j, a), or None where the
    column has no substitutions -- worked out here from the definition, not through the twins."""
    g = p - (j - R) if neg else p + (j - R)
    plus = int(codes[g]) if 0 <= g < len(codes) else 4
    if plus > 3:
        return None
    ref_w = 3 - plus if neg else plus
    alt_w = [b for b in range(4) if b != ref_w][a]
    return g, (3 - alt_w if neg else alt_w), alt_w


def check_map(r, R, model_no, chunks=(64, 1000), oracle_sample=None):
    from mural_amd.data import PackedGenome
    from mural_amd.mutagenesis import mutagenesis_rows, saturation_mutagenesis
    from tests.test_gpu_snv import assert_probs_close
    seq = map_sequence()
    codes = encode_ref.seq_to_codes(seq)
    genome = PackedGenome.from_sequence(seq, "cuda")
    model, orc = build_models(r, R, model_no)
    pos_h, strand_h = np.array([2, 2395, 2503, MAP_LENGTH - 2], np.int64), np.array([0, 1, 0, 1], np.uint8)
    pos, strand = torch.from_numpy(pos_h).cuda(), torch.from_numpy(strand_h).cuda()
    n, W = len(pos_h), 2 * R + 1
    res = saturation_mutagenesis(model, genome, pos, strand, local_radius=r, local_order=3, return_logp=True)
    assert res.delta.shape == (n, W, 4, 4) and res.delta.dtype == torch.float32 and res.var_logp.shape == res.delta.shape
    assert res.ref_logp.shape == (n, 4) and res.ref_symbols.shape == (n, W) and res.ref_symbols.dtype == torch.uint8
    assert torch.equal(res.ref_symbols, genome.encode_symbols(pos, strand, R).sym)

    # 1. exp(var_logp) against the float64 oracle on the patched windows
    def live(v):
        return _variant(codes, int(pos_h[v // 3 // W]), bool(strand_h[v // 3 // W]), v // 3 % W, v % 3, R) is not None

    if oracle_sample is None:
        ids = np.arange(n * W * 3)                                                     # every variant
    else:                                                                             # a seeded sample of live ids + all edge columns
        rng = np.random.default_rng(R + model_no)
        drawn = [v for v in rng.permutation(n * W * 3).tolist()[:8 * oracle_sample] if live(v)][:oracle_sample]
        assert len(drawn) == oracle_sample
        edge_cols = [0, 1, W - 2, W - 1, R - 1, R, R + 1, R - r - 1, R - r, R - r + 2, R + r - 2, R + r, R + r + 1]
        edge = [(s * W + j) * 3 + a for s in range(n) for j in edge_cols for a in range(3)]
        ids = np.unique(np.concatenate([drawn, edge]))
    cats, xs, picks = [], [], []
    for v in ids.tolist():
        s, j, a = v // 3 // W, v // 3 % W, v % 3
        neg = bool(strand_h[s])
        var = _variant(codes, int(pos_h[s]), neg, j, a, R)
        if var is None:
            continue
        g, alt_plus, alt_w = var
        patched = codes.copy()
        patched[g] = alt_plus
        st = ["-" if neg else "+"]
        cats.append(encode_ref.kmer_encode(patched, [pos_h[s]], st, r, 3)[0])
        xs.append(encode_ref.onehot_encode(patched, [pos_h[s]], st, R)[0])
        picks.append((s, j, alt_w))
    assert len(picks) >= (oracle_sample if oracle_sample else n * W)
    with torch.no_grad():
        want = orc((torch.zeros(len(picks), 1, dtype=torch.float64), torch.from_numpy(np.stack(cats))), torch.from_numpy(np.stack(xs))).numpy()
    s_i, j_i, b_i = (torch.tensor(c, device="cuda") for c in zip(*picks))
    got = res.var_logp[s_i, j_i, b_i].cpu().numpy()
    err = np.abs(np.exp(got.astype(np.float64)) - np.exp(want)).max()
    print(f"mutagenesis map r={r} R={R} Network{model_no}: {len(picks)} variants, max prob err {err:.3e}")
    assert_probs_close(got, want, model_no, f"map r={r} R={R} Network{model_no}")
    # the variants are not the reference: a substitution of the focal base always changes the prediction
    focal = np.array([j == R for _, j, _ in picks])
    assert focal.any() and (got != res.ref_logp[s_i].cpu().numpy()).any(axis=1)[focal].all()

    # 2. delta == var_logp - ref_logp bit for bit; +0.0 at the reference base; NaN in all four entries of a non-A/C/G/T column
    plain = (res.ref_symbols < 4)[:, :, None, None].expand_as(res.delta)
    at_ref = (torch.arange(4, device="cuda")[None, None, :] == res.ref_symbols[:, :, None].long())[..., None].expand_as(res.delta)
    sub = _bits(res.var_logp - res.ref_logp[:, None, None, :])
    d_bits, l_bits = _bits(res.delta), _bits(res.var_logp)
    alt_cells = plain & ~at_ref
    assert int(alt_cells.sum()) > 0 and int((~plain).sum()) > 0
    assert torch.equal(d_bits[alt_cells], sub[alt_cells])
    assert bool((d_bits[plain & at_ref] == 0).all())                                  # +0.0, not -0.0
    assert torch.equal(res.var_logp[plain & at_ref].reshape(-1, 4), res.ref_logp[:, None, :].expand(n, W, 4)[(res.ref_symbols < 4)])
    assert bool((d_bits[~plain] == NAN_BITS).all()) and bool((l_bits[~plain] == NAN_BITS).all())
    assert bool(torch.isfinite(res.delta[plain]).all())

    # 3. the whole map bit-identical however the ids are chunked (64 and 1000 cut sites and columns; the default is one chunk here)
    for chunk in chunks:
        other = saturation_mutagenesis(model, genome, pos, strand, local_radius=r, local_order=3, chunk_windows=chunk, return_logp=True)
        assert torch.equal(_bits(other.delta), d_bits) and torch.equal(_bits(other.var_logp), l_bits), chunk
        assert torch.equal(other.ref_logp, res.ref_logp)
    assert saturation_mutagenesis(model, genome, pos, strand, local_radius=r, local_order=3).var_logp is None

    # 4. var_logp bit-identical to forward_symbols on the encoder's rows; a 255 row equals the reference row
    total = n * W * 3
    row_pos, row_strand, sub_pos, sub_base = mutagenesis_rows(genome, pos, strand, R, 0, total)
    sym, cat = genome.encode_subst_windows(row_pos, row_strand, sub_pos, sub_base, R, r, 3)
    with torch.no_grad():
        rows = model.forward_symbols(cat if model_no == 2 else None, sym)
    v = torch.arange(total, device="cuda")
    site, col, a = v // 3 // W, v // 3 % W, v % 3
    ref = res.ref_symbols[site, col].long()
    live = sub_base != 255
    assert torch.equal(live, ref < 4)
    alt = a + (a >= ref).long()
    assert torch.equal(res.var_logp[site[live], col[live], alt[live]], rows[live])
    assert torch.equal(rows[~live], res.ref_logp[site[~live]])

    # 5. the accessors
    gp = res.genomic_positions().cpu().numpy()
    off = np.arange(-R, R + 1)
    assert np.array_equal(gp, pos_h[:, None] + np.where(strand_h[:, None] != 0, -off[None, :], off[None, :]))
    imp = res.importance().cpu().numpy()
    mag = np.abs(res.delta.cpu().numpy()).reshape(n, W, -1)
    dead = np.isnan(mag).all(axis=2)
    assert np.array_equal(dead, (res.ref_symbols >= 4).cpu().numpy()) and np.isnan(imp[dead]).all()
    assert np.array_equal(imp[~dead], mag[~dead].max(axis=1))
    return res


@pytest.mark.parametrize("r,R,model_no,sample", [(5, 100, 2, None), (5, 100, 1, None), (10, 1000, 2, 200), (10, 1000, 1, 200)])
def test_saturation_map(r, R, model_no, sample):
    check_map(r, R, model_no, oracle_sample=sample)


# ----------------------------------------------------------------------------------------------------------------------------------
# footprint
# ----------------------------------------------------------------------------------------------------------------------------------
def test_variant_footprint_is_the_transposed_map():
    from mural_amd.data import PackedGenome
    from mural_amd.mutagenesis import saturation_mutagenesis, variant_footprint
    r, R = 5, 100
    seq = map_sequence()
    codes = encode_ref.seq_to_codes(seq)
    genome = PackedGenome.from_sequence(seq, "cuda")
    model, _ = build_models(r, R, 2)
    W = 2 * R + 1
    var_pos = np.array([1000, 1000, 30, MAP_LENGTH - 40, MAP_N_RUN[0] - 5, 3000], np.int64)
    strand = np.array([0, 1, 1, 0, 1, 0], np.uint8)
    var_base = (codes[var_pos] + np.array([1, 2, 3, 1, 2, 0])) % 4                   # the last one names the reference base itself
    assert (codes[var_pos] < 4).all()
    fp, focal = variant_footprint(model, genome, torch.from_numpy(var_pos).cuda(), torch.from_numpy(var_base.astype(np.uint8)).cuda(),
                                  torch.from_numpy(strand).cuda(), local_radius=r, local_order=3)
    assert fp.shape == (len(var_pos), W, 4) and fp.dtype == torch.float32 and focal.shape == (len(var_pos), W) and focal.dtype == torch.uint8
    small = variant_footprint(model, genome, torch.from_numpy(var_pos).cuda(), torch.from_numpy(var_base.astype(np.uint8)).cuda(),
                              torch.from_numpy(strand).cuda(), local_radius=r, local_order=3, chunk_windows=333)
    assert torch.equal(_bits(small[0]), _bits(fp)) and torch.equal(small[1], focal)
    for i, (vp, vb, s) in enumerate(zip(var_pos.tolist(), var_base.tolist(), strand.tolist())):
        d = np.arange(-R, R + 1)
        site = vp + d
        inside = (site >= 0) & (site < MAP_LENGTH)
        keep = inside & (d != 0)
        assert bool(torch.isnan(fp[i][torch.from_numpy(~keep).cuda()]).all())         # d = 0 and beyond the chromosome ends
        if i in (2, 3):
            assert (~inside).any()
        sites = torch.from_numpy(site[keep]).cuda()
        res = saturation_mutagenesis(model, genome, sites, torch.full_like(sites, s, dtype=torch.uint8), local_radius=r, local_order=3)
        col = torch.from_numpy((R + d[keep]) if s else (R - d[keep])).cuda()          # the column of site var_pos + d that is var_pos
        assert bool((res.genomic_positions()[torch.arange(len(sites), device="cuda"), col] == vp).all())
        want = res.delta[torch.arange(len(sites), device="cuda"), col, (3 - vb) if s else vb]
        got = fp[i][torch.from_numpy(keep).cuda()]
        assert torch.equal(_bits(got), _bits(want)), i
        assert bool(torch.isfinite(got).all())
        if i == 5:
            assert bool((_bits(got) == 0).all())                                      # the reference base: exactly +0.0
        else:
            assert float(got.abs().max()) > 0
        assert torch.equal(focal[i][torch.from_numpy(keep).cuda()], res.ref_symbols[:, R])
        assert bool((focal[i][torch.from_numpy(~inside).cuda()] == 4).all())


# ----------------------------------------------------------------------------------------------------------------------------------
# errors
# ----------------------------------------------------------------------------------------------------------------------------------
def test_unsupported_models_and_inputs_raise_with_the_reason():
    from mural_amd.data import PackedGenome
    from mural_amd.mutagenesis import saturation_mutagenesis, variant_footprint
    genome = PackedGenome.from_sequence(map_sequence(), "cuda")
    pos, strand = torch.tensor([1000, 2000], device="cuda"), torch.tensor([0, 1], dtype=torch.uint8, device="cuda")
    base = torch.tensor([1, 2], dtype=torch.uint8, device="cuda")
    net0, _ = build_models(5, 100, 0)
    with pytest.raises(RuntimeError, match="Network0"):
        saturation_mutagenesis(net0, genome, pos, strand)
    with pytest.raises(RuntimeError, match="Network0"):
        variant_footprint(net0, genome, pos, base, strand)
    model, _ = build_models(5, 100, 2)
    model.train()
    with pytest.raises(RuntimeError, match="eval mode"):
        saturation_mutagenesis(model, genome, pos, strand)
    with pytest.raises(RuntimeError, match="eval mode"):
        variant_footprint(model, genome, pos, base, strand)
    model.eval()
    with pytest.raises(RuntimeError, match="HIP device"):
        saturation_mutagenesis(model, genome, pos.cpu(), strand.cpu())
    with pytest.raises(RuntimeError, match="HIP device"):
        variant_footprint(model, genome, pos, base.cpu(), strand)
    on_cpu = build_models(5, 100, 1)[0].cpu()
    with pytest.raises(RuntimeError, match="HIP device"):
        saturation_mutagenesis(on_cpu, genome, pos, strand)
    with pytest.raises(ValueError):
        saturation_mutagenesis(model, genome, pos, strand, chunk_windows=0)
    empty = saturation_mutagenesis(model, genome, pos[:0], strand[:0])
    assert empty.delta.shape == (0, 201, 4, 4) and empty.importance().shape == (0, 201)
