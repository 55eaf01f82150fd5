"""GPU tests of saturation mutagenesis for the INDEL model: ``mural_indel_forward_symbols`` against the dense
and packed entries and the oracle, the window-generic encoder / enumerator / reduce against their numpy twins, the log-softmax of the
scores against float64, the map against the oracle on patched windows, the footprint against the map."""
import ctypes as C
import functools

import numpy as np
import pytest
import torch

from oracle import encode_ref, indel_ref, synth
from tests import _mutagenesis_data as D
from tests import _util as U
from tests._parity import _loose, _Stats

pytestmark = pytest.mark.gpu

NAN_BITS = 0x7FC00000
SCORE_BAR = 1e-4                  # the INDEL forward's bar against the oracle: 1e-4 * max(1, |want|) (tests/test_gpu_indel.py)


def _bits(t):
    return t.contiguous().view(torch.int32)


@functools.lru_cache(maxsize=None)
def models(name):
    """(product model on the device in eval mode, oracle, distal radius) of a golden INDEL fixture, or of "unfused": random weights on
    down_list [2, 2, 5, 5, 5, 2] (L = 1000), a geometry the fused first level does not serve."""
    from mural_amd.model import model_choice
    if name == "unfused":
        R, down = 500, [2, 2, 5, 5, 5, 2]
        orc = indel_ref.build(n_class=8, channels=8, ksize=7, down_list=down, use_reverse=True)
        sd = synth.synth_state_dict(orc.state_dict(), 41)
        model = model_choice(0, dict(CNN_out_channels=8, CNN_kernel_size=7, down_list=down, use_reverse=True), dict(n_class=8), "indel")
    else:
        from tests.test_gpu_indel import product_from
        fx = U.load(name)
        R = int(fx["hp"][0])
        model = product_from(fx)
        orc = U.indel_oracle_from_hp(fx["hp"], fx["down"])
        sd = U.indel_state_for(fx, orc)
    model.load_state_dict(sd)
    orc.load_state_dict(sd)
    orc.eval()
    return model.cuda().eval(), orc, R


def sites_case(R):
    """The 32 sites of test_packed_entry_decodes_inside_the_first_level: every IUPAC code, an N run, both chromosome ends, both strands."""
    rng = np.random.default_rng(R)
    n = 6 * R + 1000
    alphabet, p = b"ACGTNRYMSWKBDHV", [.2455] * 4 + [.008] + [.001] * 10
    raw = rng.choice(np.frombuffer(alphabet, np.uint8), size=n, p=np.array(p) / sum(p))
    raw[n // 2:n // 2 + 40] = ord("N")
    seq = raw.tobytes().decode()
    pos = np.r_[[0, 3, R - 1, n - 1, n - R, n // 2 + 7], rng.integers(0, n, size=26)]
    strand = (np.arange(len(pos)) % 2).astype(np.uint8)
    return seq, pos, strand


def poison_workspace(model, monkeypatch):
    """the model's next workspace and outputs come pre-filled with 0xFF bytes (NaN): whatever a kernel reads, it must have written"""
    from mural_amd.model import model_indel as MI
    from tests.test_gpu_snv import _PoisonedTorch
    monkeypatch.setattr(MI, "torch", _PoisonedTorch())
    model._ws = None


# ----------------------------------------------------------------------------------------------------------------------------------
# 1. forward_symbols
# ----------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["indel_synth_small.npz", "indel_synth_c2.npz", "unfused"])
def test_forward_symbols_equals_the_dense_and_packed_entries(name, monkeypatch):
    from mural_amd.data import PackedGenome
    from mural_amd.data.genome import SymbolWindows
    model, orc, R = models(name)
    seq, pos, strand = sites_case(R)
    codes = encode_ref.seq_to_codes(seq)
    x = torch.from_numpy(encode_ref.onehot_encode(codes, pos, ["-" if v else "+" for v in strand], R, "indel"))
    genome = PackedGenome.from_sequence(seq, "cuda")
    tp, ts = torch.from_numpy(pos).cuda(), torch.from_numpy(strand).cuda()
    poison_workspace(model, monkeypatch)
    with torch.no_grad():
        want = orc(x).numpy()
        windows = genome.encode_symbols(tp, ts, R, "indel")
        assert isinstance(windows, SymbolWindows) and windows.sym.shape == (len(pos), 2 * R) and int(windows.sym.max()) > 4
        got = model.forward_symbols(windows)
        again = model.forward_symbols(windows.sym)
        packed = model.forward_packed(genome, tp, ts, R)
        dense = model(genome.encode_onehot(tp, ts, R, "indel"))
        detour = model(windows)
        empty = model.forward_symbols(windows.sym[:0])
    assert got.shape == (len(pos), model.n_class) and got.dtype == torch.float32 and empty.shape == (0, model.n_class)
    assert torch.equal(_bits(got), _bits(again))
    assert torch.equal(_bits(got), _bits(dense)), float((got - dense).abs().max())
    assert torch.equal(_bits(got), _bits(packed)), float((got - packed).abs().max())
    assert torch.equal(_bits(got), _bits(detour))
    err, tol = np.abs(got.cpu().numpy() - want).max(), SCORE_BAR * max(1.0, np.abs(want).max())
    print(f"forward_symbols {name}: max score err {err:.3e} (bar {tol:.3e})")
    assert err <= tol


@pytest.mark.parametrize("name", ["indel_synth_small.npz", "unfused"])
def test_forward_symbols_in_two_lanes_and_with_bytes_that_are_no_symbol(name, monkeypatch):
    """300 rows with MURAL_INDEL_CHUNK = 256: two chunks, one per stream, each on its half of the workspace.  In one row a few bytes are
    200: they read as N, in the fused first level and in the expanding fallback alike."""
    from mural_amd.data import PackedGenome
    model, _, R = models(name)
    seq, pos, strand = sites_case(R)
    genome = PackedGenome.from_sequence(seq, "cuda")
    rng = np.random.default_rng(9)
    idx = torch.from_numpy(rng.integers(0, len(pos), size=300)).cuda()
    tp, ts = torch.from_numpy(pos).cuda()[idx], torch.from_numpy(strand).cuda()[idx]
    poison_workspace(model, monkeypatch)
    with torch.no_grad():
        sym = genome.encode_symbols(tp, ts, R, "indel").sym
        monkeypatch.setenv("MURAL_INDEL_CHUNK", "256")
        model._ws = None
        got = model.forward_symbols(sym)
        dense = model(genome.encode_onehot(tp, ts, R, "indel"))
        assert torch.isfinite(got).all() and torch.equal(_bits(got), _bits(dense))
        cols = torch.tensor([0, 1, 2, 3, R - 1, R, 2 * R - 2, 2 * R - 1, 417], device="cuda")
        bad, as_n = sym[280:290].clone(), sym[280:290].clone()
        assert bool((bad[3, cols] < 4).any())
        bad[3, cols] = 200
        bad[5, 7] = 15
        as_n[3, cols] = 4
        as_n[5, 7] = 4
        a, b, c = model.forward_symbols(bad), model.forward_symbols(as_n), model.forward_symbols(sym[280:290])
    assert torch.equal(_bits(a), _bits(b))
    # (calls of one size: the untouched rows keep their bits, the touched ones do not)
    keep = torch.tensor([0, 1, 2, 4, 6, 7, 8, 9], device="cuda")
    assert torch.equal(_bits(a[keep]), _bits(c[keep])) and not torch.equal(_bits(a[3]), _bits(c[3]))


def test_forward_symbols_refuses_what_it_cannot_serve():
    model, _, R = models("indel_synth_small.npz")
    sym = torch.zeros((2, 2 * R), dtype=torch.uint8, device="cuda")
    with pytest.raises(RuntimeError, match="HIP device"):
        model.forward_symbols(sym.cpu())
    with pytest.raises(TypeError):
        model.forward_symbols(sym.float())
    with pytest.raises(TypeError):
        model.forward_symbols(sym[0])
    with pytest.raises(ValueError):                                 # a length down_list cannot serve (reported by the library)
        model.forward_symbols(sym[:, :999].contiguous())
    model.train()
    try:
        with pytest.raises(RuntimeError, match="eval mode"):
            model.forward_symbols(sym)
    finally:
        model.eval()
    from mural_amd import _lib
    assert _lib.lib().mural_abi_version() == 4


# ----------------------------------------------------------------------------------------------------------------------------------
# 2. encoder / enumerator / reduce against their twins
# ----------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("radius", [6, 100, 500])
def test_indel_subst_encoder_matches_its_twin_and_the_plain_encoder(radius):
    from mural_amd.data import PackedGenome
    from mural_amd.mutagenesis import encode_subst_windows_host
    from tests.test_mutagenesis_indel_host import _cases
    seq = D.sequence()
    genome = PackedGenome.from_sequence(seq, "cuda")
    pos, strand, sub_pos, sub_base = _cases(*D.sites(), radius)
    got, cat = genome.encode_subst_windows(pos, strand, sub_pos, sub_base, radius, model_type="indel")
    assert cat is None and got.dtype == torch.uint8 and got.shape == (len(pos), 2 * radius)
    want, _ = encode_subst_windows_host(seq, pos, strand, sub_pos, sub_base, radius, model_type="indel")
    assert np.array_equal(got.cpu().numpy(), want)
    none = np.full_like(sub_base, 255)
    plain = genome.encode_subst_windows(pos, strand, sub_pos, none, radius, model_type="indel")[0]
    assert torch.equal(plain, genome.encode_symbols(pos, strand, radius, "indel").sym)
    assert int((got != plain).any(dim=1).sum()) > 50
    # the plain encoder on the patched genome, for the rows of three patched texts
    for i in (0, 1, 2, 3 * 14 + 5):
        g2 = PackedGenome.from_sequence(D.patched(seq, int(sub_pos[i]), int(sub_base[i])), "cuda")
        assert torch.equal(got[i], g2.encode_symbols(pos[i:i + 1], strand[i:i + 1], radius, "indel").sym[0])
    e, _ = genome.encode_subst_windows(pos[:0], strand[:0], sub_pos[:0], sub_base[:0], radius, model_type="indel")
    assert e.shape == (0, 2 * radius)


@pytest.mark.parametrize("radius,chunk", [(6, 1), (6, 97), (100, 1009), (500, 4099), (500, None)])
def test_indel_enumerator_matches_the_host_twin(radius, chunk):
    from mural_amd.data import PackedGenome
    from mural_amd.mutagenesis import mutagenesis_rows, mutagenesis_rows_host
    seq = D.sequence()
    genome = PackedGenome.from_sequence(seq, "cuda")
    pos, strand = D.sites()
    total = len(pos) * 2 * radius * 3
    want = mutagenesis_rows_host(seq, pos, strand, radius, 0, total, "indel")
    assert (want[3] == 255).any() and (want[3] != 255).any()
    step = total if chunk is None else chunk                       # (97, 1009, 4099: ranges that start and end mid-site and mid-column)
    parts = [mutagenesis_rows(genome, pos, strand, radius, first, min(step, total - first), "indel") for first in range(0, total, step)]
    got = [torch.cat([p[k] for p in parts]).cpu().numpy() for k in range(4)]
    for g, w in zip(got, want):
        assert g.dtype == w.dtype and np.array_equal(g, w)
    with pytest.raises(ValueError):
        mutagenesis_rows(genome, pos, strand, radius, total - 1, 2, "indel")


@pytest.mark.parametrize("radius", [6, 100, 500])
def test_indel_reduce_matches_the_host_twin(radius):
    from mural_amd.data import PackedGenome
    from mural_amd.mutagenesis import mutagenesis_reduce, mutagenesis_reduce_host
    seq, n_class = D.sequence(), 3
    genome = PackedGenome.from_sequence(seq, "cuda")
    pos, strand = D.sites()
    W = 2 * radius
    ref_symbols = genome.encode_symbols(pos, strand, radius, "indel").sym
    rng = np.random.default_rng(radius)
    ref_logp = rng.normal(size=(len(pos), n_class)).astype(np.float32)
    var_logp = rng.normal(size=(len(pos) * W * 3, n_class)).astype(np.float32)
    want, want_l = (np.full((len(pos), W, 4, n_class), 7.0, np.float32) for _ in range(2))
    mutagenesis_reduce_host(ref_logp, var_logp, ref_symbols.cpu().numpy(), 0, want, want_l)
    delta, logp = (torch.full((len(pos), W, 4, n_class), 7.0, device="cuda") for _ in range(2))
    total = len(var_logp)
    cuts = [0, 1, 5, 3 * W + 2, 3 * W * 5 + 1, total // 2 + 1, total]
    rl, vl = torch.from_numpy(ref_logp).cuda(), torch.from_numpy(var_logp).cuda()
    for lo, hi in zip(cuts[:-1], cuts[1:]):
        mutagenesis_reduce(rl, vl[lo:hi].contiguous(), ref_symbols, lo, delta, logp)
    assert np.array_equal(delta.cpu().numpy().view(np.int32), want.view(np.int32))
    assert np.array_equal(logp.cpu().numpy().view(np.int32), want_l.view(np.int32))
    assert np.isnan(want).any() and (want.view(np.int32) == 0).any()


@pytest.mark.parametrize("radius", [6, 100])
def test_window_entries_with_indel_0_are_the_snv_entries(radius):
    """mural_encode_subst_symbols / mural_mutagenesis_rows_window / mural_mutagenesis_reduce_window with indel = 0 (W = 2 R + 1) against
    the three entries they generalise, on the same rows: the same bytes."""
    from mural_amd import _lib
    from mural_amd.data import PackedGenome
    from mural_amd.mutagenesis import _encode_subst_symbols_into, mutagenesis_reduce, mutagenesis_rows
    seq = D.sequence()
    genome = PackedGenome.from_sequence(seq, "cuda")
    pos_h, strand_h = D.sites()
    pos, strand = genome._prep(pos_h, strand_h)
    W = 2 * radius + 1
    total = len(pos_h) * W * 3
    first, count = 7, total - 12
    old = mutagenesis_rows(genome, pos, strand, radius, first, count)
    new = (torch.empty(count, dtype=torch.int64, device="cuda"), torch.empty(count, dtype=torch.uint8, device="cuda"),
           torch.empty(count, dtype=torch.int64, device="cuda"), torch.empty(count, dtype=torch.uint8, device="cuda"))
    g = genome.as_struct()
    stream = _lib.current_stream_ptr(genome.device)
    _lib.check(_lib.lib().mural_mutagenesis_rows_window(C.byref(g), pos.data_ptr(), strand.data_ptr(), len(pos_h), radius, 0, first, count,
                                                       *[t.data_ptr() for t in new], stream))
    for o, n in zip(old, new):
        assert torch.equal(o, n)
    old_sym, _ = genome.encode_subst_windows(*old, radius, 5, 3)
    new_sym = torch.empty_like(old_sym)
    _encode_subst_symbols_into(genome, *old, radius, 0, new_sym)
    assert new_sym.shape[1] == W and torch.equal(old_sym, new_sym)
    rng = np.random.default_rng(1)
    ref_symbols = genome.encode_symbols(pos, strand, radius).sym
    rl = torch.from_numpy(rng.normal(size=(len(pos_h), 4)).astype(np.float32)).cuda()
    vl = torch.from_numpy(rng.normal(size=(count, 4)).astype(np.float32)).cuda()
    d_old, l_old, d_new, l_new = (torch.full((len(pos_h), W, 4, 4), 7.0, device="cuda") for _ in range(4))
    mutagenesis_reduce(rl, vl, ref_symbols, first, d_old, l_old)
    _lib.check(_lib.lib().mural_mutagenesis_reduce_window(rl.data_ptr(), vl.data_ptr(), ref_symbols.data_ptr(), len(pos_h), W, 4, first, count,
                                                         d_new.data_ptr(), l_new.data_ptr(), stream))
    assert torch.equal(_bits(d_old), _bits(d_new)) and torch.equal(_bits(l_old), _bits(l_new))
    assert bool((_bits(d_new) == NAN_BITS).any())


# ----------------------------------------------------------------------------------------------------------------------------------
# 3. log-softmax of the scores
# ----------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n_class", [2, 8])
def test_scores_log_softmax_against_float64(n_class):
    from mural_amd.mutagenesis import log_softmax_host, scores_log_softmax
    rng = np.random.default_rng(n_class)
    n = 5000
    s = np.abs(rng.normal(size=(n, n_class))).astype(np.float32)            # Softplus scores: positive
    s[1000:2000] *= 8.0
    s[2000:2100] += 30.0                                                   # (above Softplus's linear threshold)
    s[2100] = 0.5                                                          # a row of equal scores
    s[2101, 0] = 90.0                                                      # one class far above the others: exp of the rest underflows
    scores = torch.from_numpy(s).cuda()
    got = scores_log_softmax(scores)
    assert got.shape == scores.shape and got.dtype == torch.float32 and torch.equal(scores.cpu(), torch.from_numpy(s))
    want = torch.from_numpy(log_softmax_host(s))
    ref32 = torch.log_softmax(torch.from_numpy(s), dim=1)
    stats = _Stats("log_softmax", "mutagenesis_indel")
    _loose(got, want, ref32, f"log_softmax C={n_class}", f"n={n}", stats)
    stats.show()
    # a row's bits do not depend on n or on its neighbours
    for i in (0, 1, 1500, 2100, 2101, n - 1):
        assert torch.equal(_bits(scores_log_softmax(scores[i:i + 1].contiguous()))[0], _bits(got)[i])
    assert scores_log_softmax(scores[:0]).shape == (0, n_class)
    with pytest.raises(ValueError):
        scores_log_softmax(scores.double())


# ----------------------------------------------------------------------------------------------------------------------------------
# 4. the map
# ----------------------------------------------------------------------------------------------------------------------------------
MAP_LENGTH = 3000
MAP_N_RUN = (1400, 1420)
MAP_IUPAC = 1500
MAP_SITES = (np.array([1399, 1600], np.int64), np.array([1, 0], np.uint8))      # one per strand; the first next to the N run


def map_sequence():
    rng = np.random.default_rng(13)
    raw = rng.choice(np.frombuffer(b"ACGT", np.uint8), size=MAP_LENGTH)
    raw[MAP_N_RUN[0]:MAP_N_RUN[1]] = ord("N")
    raw[MAP_IUPAC] = ord("Y")
    return raw.tobytes().decode()


def _column_pos(p, neg, j, R):
    return p + R - j if neg else p - R + 1 + j


def _oracle_logp(orc, codes, rows, R):
    """float64 (scores, log-softmax) of the oracle on the windows of rows (site, strand, patched position or None, '+'-strand base)"""
    xs = []
    for p, neg, g, b in rows:
        patched = codes
        if g is not None:
            patched = codes.copy()
            patched[g] = b
        xs.append(encode_ref.onehot_encode(patched, [p], ["-" if neg else "+"], R, "indel")[0])
    with torch.no_grad():
        scores = orc(torch.from_numpy(np.stack(xs))).double()
    return scores.numpy(), torch.log_softmax(scores, dim=1).numpy()


def check_map(name="indel_synth_small.npz", chunks=(1000, 4096)):
    from mural_amd.data import PackedGenome
    from mural_amd.mutagenesis import saturation_mutagenesis
    model, orc, R = models(name)
    seq = map_sequence()
    codes = encode_ref.seq_to_codes(seq)
    genome = PackedGenome.from_sequence(seq, "cuda")
    pos_h, strand_h = MAP_SITES
    pos, strand = torch.from_numpy(pos_h).cuda(), torch.from_numpy(strand_h).cuda()
    n, W, n_class = len(pos_h), 2 * R, model.n_class
    maps = [saturation_mutagenesis(model, genome, pos, strand, distal_radius=R, chunk_windows=c, return_logp=True) for c in chunks]
    res = maps[0]
    assert res.delta.shape == (n, W, 4, n_class) and res.delta.dtype == torch.float32 and res.var_logp.shape == res.delta.shape
    assert res.ref_logp.shape == (n, n_class) and res.ref_symbols.shape == (n, W) and res.model_type == "indel" and res.radius == R
    assert torch.equal(res.ref_symbols, genome.encode_symbols(pos, strand, R, "indel").sym)
    gp = res.genomic_positions().cpu().numpy()
    for s in range(n):
        assert np.array_equal(gp[s], [_column_pos(int(pos_h[s]), bool(strand_h[s]), j, R) for j in range(W)])

    # the oracle on a fixed column set
    rng = np.random.default_rng(R)
    rows, picks, dead = [(int(pos_h[s]), bool(strand_h[s]), None, 0) for s in range(n)], [], []
    for s in range(n):
        p, neg = int(pos_h[s]), bool(strand_h[s])
        special = [j for j in range(W) if MAP_N_RUN[0] <= _column_pos(p, neg, j, R) < MAP_N_RUN[1] or _column_pos(p, neg, j, R) == MAP_IUPAC]
        assert len(special) == MAP_N_RUN[1] - MAP_N_RUN[0] + 1
        cols = sorted(set([0, 1, R - 2, R - 1, R, R + 1, W - 2, W - 1] + special + rng.choice(W, size=20, replace=False).tolist()))
        for j in cols:
            g = _column_pos(p, neg, j, R)
            plus = int(codes[g])
            if plus > 3:
                dead.append((s, j))
                continue
            ref_w = 3 - plus if neg else plus
            for alt_w in range(4):
                if alt_w != ref_w:
                    rows.append((p, neg, g, 3 - alt_w if neg else alt_w))
                    picks.append((s, j, alt_w))
            picks.append((s, j, ref_w))                           # the reference base itself: +0.0
            rows.append((p, neg, None, 0))
    scores, logp = _oracle_logp(orc, codes, rows, R)
    bar = 4.0 * SCORE_BAR * max(1.0, float(np.abs(scores).max()))
    s_i, j_i, b_i = (torch.tensor(c, device="cuda") for c in zip(*picks))
    site = np.array([p[0] for p in picks])
    want_delta = logp[n:] - logp[site]
    got = res.delta[s_i, j_i, b_i].cpu().numpy().astype(np.float64)
    err = float(np.abs(got - want_delta).max())
    err_ref = float(np.abs(res.ref_logp.cpu().numpy() - logp[:n]).max())
    print(f"INDEL map {name}: {len(rows)} oracle rows, max |delta - oracle| {err:.3e}, ref_logp err {err_ref:.3e}, bar {bar:.3e}, "
          f"largest |delta| {np.abs(want_delta).max():.3e}")
    assert err <= bar and err_ref <= bar
    assert np.abs(want_delta).max() > 10 * bar                    # (the substitutions do move the rates: the comparison is not of zeros)

    # +0.0 at the reference base, NaN in all four entries of a non-A/C/G/T column, finite elsewhere, delta = var - ref in one subtraction
    plain = (res.ref_symbols < 4)[:, :, None, None].expand_as(res.delta)
    at_ref = (torch.arange(4, device="cuda")[None, None, :] == res.ref_symbols[:, :, None].long())[..., None].expand_as(res.delta)
    d_bits, l_bits = _bits(res.delta), _bits(res.var_logp)
    assert len(dead) == n * (MAP_N_RUN[1] - MAP_N_RUN[0] + 1) and int((~plain).sum()) == len(dead) * 4 * n_class
    for s, j in dead:
        assert bool((d_bits[s, j] == NAN_BITS).all()) and bool((l_bits[s, j] == NAN_BITS).all())
    assert bool((d_bits[~plain] == NAN_BITS).all()) and bool((d_bits[plain & at_ref] == 0).all())
    assert bool(torch.isfinite(res.delta[plain]).all())
    alt_cells = plain & ~at_ref
    assert torch.equal(d_bits[alt_cells], _bits(res.var_logp - res.ref_logp[:, None, None, :])[alt_cells])
    assert torch.equal(res.var_logp[plain & at_ref].reshape(-1, n_class), res.ref_logp[:, None, :].expand(n, W, n_class)[res.ref_symbols < 4])

    # the map for another chunk_windows: within the bar (the INDEL forward picks kernels by the size of a call)
    for other, c in zip(maps[1:], chunks[1:]):
        diff = (other.delta - res.delta)[plain]
        same = torch.equal(_bits(other.delta), d_bits)
        print(f"INDEL map chunk_windows {chunks[0]} vs {c}: max |difference| {float(diff.abs().max()):.3e}, bit-equal: {same}")
        assert float(diff.abs().max()) <= bar and torch.equal(_bits(other.delta)[~plain], d_bits[~plain])
        assert float((other.ref_logp - res.ref_logp).abs().max()) <= bar
    assert saturation_mutagenesis(model, genome, pos, strand, distal_radius=R, chunk_windows=chunks[-1]).var_logp is None
    return res


def test_indel_saturation_map():
    check_map()


def test_indel_map_inputs():
    from mural_amd.data import PackedGenome
    from mural_amd.mutagenesis import saturation_mutagenesis, variant_footprint
    model, _, R = models("indel_synth_small.npz")
    genome = PackedGenome.from_sequence(map_sequence(), "cuda")
    pos, strand = torch.tensor([1000, 2000], device="cuda"), torch.tensor([0, 1], dtype=torch.uint8, device="cuda")
    base = torch.tensor([1, 2], dtype=torch.uint8, device="cuda")
    with pytest.raises(ValueError, match="distal_radius"):
        saturation_mutagenesis(model, genome, pos, strand)
    with pytest.raises(RuntimeError, match="HIP device"):
        saturation_mutagenesis(model, genome, pos.cpu(), strand.cpu(), distal_radius=R)
    with pytest.raises(ValueError):
        variant_footprint(model, genome, pos, base, strand, distal_radius=R, chunk_windows=0)
    model.train()
    try:
        with pytest.raises(RuntimeError, match="eval mode"):
            saturation_mutagenesis(model, genome, pos, strand, distal_radius=R)
    finally:
        model.eval()
    empty = saturation_mutagenesis(model, genome, pos[:0], strand[:0], distal_radius=R, local_radius=3, local_order=5)
    assert empty.delta.shape == (0, 2 * R, 4, model.n_class) and empty.importance().shape == (0, 2 * R)


# ----------------------------------------------------------------------------------------------------------------------------------
# 5. footprint
# ----------------------------------------------------------------------------------------------------------------------------------
def test_indel_variant_footprint_is_the_transposed_map():
    from mural_amd.data import PackedGenome
    from mural_amd.mutagenesis import footprint_offsets, saturation_mutagenesis, variant_footprint
    model, orc, R = models("indel_synth_small.npz")
    seq = map_sequence()
    codes = encode_ref.seq_to_codes(seq)
    genome = PackedGenome.from_sequence(seq, "cuda")
    W = 2 * R
    var_pos = np.array([1000, 1000, 30, MAP_LENGTH - 40, 2000], np.int64)
    strand = np.array([0, 1, 1, 0, 0], np.uint8)
    var_base = ((codes[var_pos] + np.array([1, 2, 3, 1, 0])) % 4).astype(np.uint8)     # the last one names the reference base itself
    assert (codes[var_pos] < 4).all()
    args = (torch.from_numpy(var_pos).cuda(), torch.from_numpy(var_base).cuda(), torch.from_numpy(strand).cuda())
    fp, focal = variant_footprint(model, genome, *args, distal_radius=R)
    assert fp.shape == (len(var_pos), W, model.n_class) and fp.dtype == torch.float32 and focal.shape == (len(var_pos), W)
    d = footprint_offsets(R, "indel").numpy()
    assert np.array_equal(d, np.arange(-R, R)) and len(footprint_offsets(R)) == 2 * R + 1
    rng = np.random.default_rng(4)
    score_max = 1.0
    for i, (vp, vb, s) in enumerate(zip(var_pos.tolist(), var_base.tolist(), strand.tolist())):
        site = vp + d
        inside = (site >= 0) & (site < MAP_LENGTH)
        assert bool(torch.isnan(fp[i][torch.from_numpy(~inside).cuda()]).all())        # beyond either chromosome end
        assert bool(torch.isfinite(fp[i][torch.from_numpy(inside).cuda()]).all())      # d = 0 included: the site survives the substitution
        assert inside[R] and (i not in (2, 3) or (~inside).any())
        assert bool((focal[i][torch.from_numpy(~inside).cuda()] == 4).all())
        # the map of a few of the neighbours: both ends of the reach, d = 0 and its neighbours, seeded others
        take = np.unique(np.r_[[0, 1, R - 1, R, R + 1, W - 2, W - 1], rng.choice(W, size=5, replace=False)])
        take = take[inside[take]]
        sites = torch.from_numpy(site[take]).cuda()
        res = saturation_mutagenesis(model, genome, sites, torch.full_like(sites, s, dtype=torch.uint8), distal_radius=R)
        # site v + d holds v in column R - 1 - d on '+', R + d on '-'
        col = torch.from_numpy((R + d[take]) if s else (R - 1 - d[take])).cuda()
        rows = torch.arange(len(sites), device="cuda")
        assert bool((res.genomic_positions()[rows, col] == vp).all())
        want = res.delta[rows, col, (3 - vb) if s else vb]
        got = fp[i][torch.from_numpy(take).cuda()]
        ref_scores = _oracle_logp(orc, codes, [(int(p), bool(s), None, 0) for p in site[take]], R)[0]
        score_max = max(score_max, float(np.abs(ref_scores).max()))
        bar = 4.0 * SCORE_BAR * score_max
        diff = float((got - want).abs().max())
        print(f"INDEL footprint variant {i}: max |footprint - map| {diff:.3e} (bar {bar:.3e}), bit-equal: {torch.equal(_bits(got), _bits(want))}")
        assert diff <= bar
        if i == 4:
            assert bool((_bits(got) == 0).all()) and bool((_bits(fp[i]) == 0).all())   # the reference base: exactly +0.0 everywhere
        else:
            assert float(got.abs().max()) > 0
        site_col = R if s else R - 1
        assert torch.equal(focal[i][torch.from_numpy(take).cuda()], res.ref_symbols[:, site_col])
    small = variant_footprint(model, genome, *args, distal_radius=R, chunk_windows=333)
    assert torch.equal(small[1], focal) and torch.equal(torch.isnan(small[0]), torch.isnan(fp))
    assert float((small[0] - fp).nan_to_num().abs().max()) <= 4.0 * SCORE_BAR * score_max
