"""UNet_Small's input unit from symbol bytes (csrc/indel_first.hip: mural_op_indel_first_fwd / _bwd) against torch in float64.

The reference is F.conv1d over the dense (B, 4, L) tensor the symbols stand for (tests/_loader_data.ONEHOT: the columns of
dense_symbol.h, written out independently), and over x.flip([1, 2]) for the flipped application of the strand-symmetrising conv.
Tolerances are the summation bound of tests/_parity.py, element by element: 2 (n + 2) 2^-24 sum |terms|, n = the number of terms
of the element's sum (4 K + 1 for an output; B * Lout, or twice that with both applications, for a weight gradient).

Geometry comes from the committed fixtures (tests/golden/indel_train_{rev,norev}.npz): the strand-symmetrising conv 4 -> 4, k = 7,
stride 1, and uplblocks[0] 4 -> out_channels = 8, k = 7, stride down_list[0] = 1.  Lengths: 1000 (the smallest the fixtures' down_list
admits: 4 * 5 * 5 * 5 * 2) = three tiles of 256 positions + a remainder of 232, and the fixtures' own 2000 (seven tiles + 208)."""
import ctypes as C

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from mural_amd import _lib
from tests import _util as U
from tests._loader_data import ONEHOT
from tests._parity import _Stats, _sum_check

pytestmark = pytest.mark.gpu

_COMP = np.array([3, 2, 1, 0, 4, 6, 5, 10, 8, 9, 7, 14, 13, 12, 11], np.uint8)      # A<->T C<->G N R<->Y M<->K S W B<->V D<->H


def _geoms():
    out = []
    for tag in ("rev", "norev"):
        fx = U.load(f"indel_train_{tag}.npz")
        R, ch, k, n_class, rev = [int(v) for v in fx["hp"]]
        down = [int(d) for d in fx["down"]]
        Lmin = int(np.prod(down[1:])) * down[0]
        # (name, Cout, K, stride, pad, both applications)
        out.append((("sym4" if rev else "up_l0"), 4 if rev else ch, k, 1 if rev else down[0], (k - 1) // 2, bool(rev), (Lmin, 2 * R)))
    # the strided form of uplblocks[0] (down_list[0] = 4: the reference's other shipped geometry), same lengths
    out.append(("up_l0_s4", out[-1][1], out[-1][2], 4, out[-1][4], False, out[-1][6]))
    return out


def _rows(rng, B, L):
    """B symbol rows: all 15 codes with IUPAC / N at both ends; all N; a reverse-complement palindrome; plain bases with N / R at the ends"""
    all15 = rng.integers(0, 15, size=L).astype(np.uint8)
    all15[[0, 1, 2, L - 3, L - 2, L - 1]] = [11, 4, 5, 13, 4, 14]
    half = rng.integers(0, 15, size=L // 2).astype(np.uint8)
    pal = np.concatenate([half, _COMP[half[::-1]]])
    plain = rng.integers(0, 4, size=L).astype(np.uint8)
    plain[0], plain[L - 1] = 4, 5
    pool = [all15, np.full(L, 4, np.uint8), pal, plain]
    return np.stack(pool[:B] if B == 2 else [pool[0], pool[2], pool[3]])


def _run_fwd(sym, W, b, stride, pad, rev):
    B, L = sym.shape
    Cout, _, K = W.shape
    Lout = (L + 2 * pad - K) // stride + 1
    y = torch.full((B, Cout, Lout), float("nan"), device="cuda")
    yr = torch.full((B, Cout, Lout), float("nan"), device="cuda") if rev else None
    _lib.check(_lib.lib().mural_op_indel_first_fwd(sym.data_ptr(), W.data_ptr(), b.data_ptr() if b is not None else None, B, L, Cout, K, stride,
                                                   pad, y.data_ptr(), yr.data_ptr() if rev else None, None))
    torch.cuda.synchronize()
    return y, yr


def _run_bwd(sym, dz, dzr, Cout, K, stride, pad, db=True):
    """db = False: db = NULL is passed; the tensor returned in its place keeps its NaN fill"""
    B, L = sym.shape
    n = int(_lib.lib().mural_op_indel_first_scratch(B, L, Cout, K, stride, pad, int(dzr is not None)))
    assert n > 0
    part = torch.full((n,), float("nan"), device="cuda")
    dW = torch.full((Cout, 4, K), float("nan"), device="cuda")
    dbv = torch.full((Cout,), float("nan"), device="cuda")
    _lib.check(_lib.lib().mural_op_indel_first_bwd(sym.data_ptr(), dz.data_ptr(), dzr.data_ptr() if dzr is not None else None, B, L, Cout, K,
                                                   stride, pad, dW.data_ptr(), dbv.data_ptr() if db else None, part.data_ptr(), C.c_size_t(n), None))
    torch.cuda.synchronize()
    return dW, dbv


@pytest.mark.parametrize("geom", _geoms(), ids=lambda g: g[0])
@pytest.mark.parametrize("B", [2, 3])
def test_indel_first_layer_against_torch_float64(geom, B):
    name, Cout, K, stride, pad, rev, lengths = geom
    stats = _Stats(name, tag="indel_first")
    for L in lengths:
        rng = np.random.default_rng(100 * B + L)
        tg = torch.Generator().manual_seed(7 * B + L)
        sym_h = _rows(rng, B, L)
        W = torch.randn((Cout, 4, K), generator=tg) / (4 * K) ** 0.5
        b = torch.randn(Cout, generator=tg)
        x64 = torch.from_numpy(ONEHOT[sym_h].transpose(0, 2, 1).copy()).double()
        W64, b64 = W.double(), b.double()
        case = f"{name} B{B} L{L}"
        sym = torch.from_numpy(sym_h).cuda()
        y, yr = _run_fwd(sym, W.cuda(), b.cuda(), stride, pad, rev)
        apps = [(x64, y)] + ([(x64.flip([1, 2]), yr)] if rev else [])
        Lout = y.shape[2]
        dzs, want_dW, want_db, S_dW, S_db = [], 0.0, 0.0, 0.0, 0.0
        for a, (xa, got) in enumerate(apps):
            want = F.conv1d(xa, W64, b64, stride=stride, padding=pad)
            S = F.conv1d(xa.abs(), W64.abs(), b64.abs(), stride=stride, padding=pad)
            _sum_check(got, want, S, 4 * K + 1, f"y app{a}", case, stats)
            dz = torch.randn(want.shape, generator=tg)
            dzs.append(dz.cuda())
            Wl = W64.clone().requires_grad_()
            bl = b64.clone().requires_grad_()
            gW, gb = torch.autograd.grad(F.conv1d(xa, Wl, bl, stride=stride, padding=pad), (Wl, bl), dz.double())
            sW, sb = torch.autograd.grad(F.conv1d(xa.abs(), Wl, bl, stride=stride, padding=pad), (Wl, bl), dz.double().abs())
            want_dW, want_db, S_dW, S_db = want_dW + gW, want_db + gb, S_dW + sW, S_db + sb
        dW, db = _run_bwd(sym, dzs[0], dzs[1] if rev else None, Cout, K, stride, pad)
        n = len(apps) * B * Lout
        _sum_check(dW, want_dW, S_dW, n, "dW", case, stats)
        _sum_check(db, want_db, S_db, n, "db", case, stats)
        # a second call gives the same bits (fixed summation order)
        dW2, db2 = _run_bwd(sym, dzs[0], dzs[1] if rev else None, Cout, K, stride, pad)
        assert torch.equal(dW, dW2) and torch.equal(db, db2), case
        if B == 3:
            # bytes above 14 count as N: the row with such bytes equals the row with N there, bit for bit
            bad = sym_h.copy()
            cols = rng.choice(L, size=40, replace=False)
            cols[:2] = [0, L - 1]
            bad[1, cols] = rng.choice(np.array([15, 16, 77, 200, 255], np.uint8), size=40)
            asn = bad.copy()
            asn[1, cols] = 4
            outs = []
            for s in (bad, asn):
                st = torch.from_numpy(s).cuda()
                outs.append(_run_fwd(st, W.cuda(), b.cuda(), stride, pad, rev) + _run_bwd(st, dzs[0], dzs[1] if rev else None, Cout, K, stride, pad))
            for g0, g1 in zip(*outs):
                assert (g0 is None and g1 is None) or torch.equal(g0, g1), case
            assert torch.isfinite(outs[0][0]).all()
    stats.show()


def test_indel_first_layer_refuses_what_it_does_not_cover():
    sym = torch.zeros((2, 1000), dtype=torch.uint8, device="cuda")
    W, b = torch.zeros((4, 4, 7), device="cuda"), torch.zeros(4, device="cuda")
    with pytest.raises(ValueError):      # the flipped application needs stride 1
        _run_fwd(sym, W, b, 2, 3, True)
    with pytest.raises(ValueError):      # output channels in groups of four
        _run_fwd(sym, torch.zeros((6, 4, 7), device="cuda"), torch.zeros(6, device="cuda"), 1, 3, False)


# ------------------------------------------------------------------------------------------------- beyond the capped grids, at the edges
# Both kernels cap their grid and walk on (csrc/indel_first.hip): the weight gradient at IF_MAX_CHUNKS = 256 workgroups per application,
# each of which then takes tile, tile + 256, ... with its 16 register bins carried from tile to tile; the forward at 4096 workgroups.
# The workload (B = 128, L = 8000: 4096 tiles) gives every gradient workgroup 16 tiles and puts the forward on its cap; the cases above
# stop at 24 tiles.  Same reference and same bounds as above.
def _random_rows(rng, B, L):
    """B rows of all 15 codes; row 1 all N; N / IUPAC at both ends of row 0; a few bytes above 14 (they count as N) in the last row"""
    sym = rng.integers(0, 15, size=(B, L)).astype(np.uint8)
    if B > 1:
        sym[1] = 4
    sym[0, [0, L - 1]] = [11, 14]
    sym[B - 1, rng.integers(0, L, size=3)] = [15, 200, 255]
    return sym


def _check(stats, case, sym_h, W, b, stride, pad, rev, tg, fwd=True, bwd=True, db=True):
    """forward (b = None: bias = NULL) and / or backward (db = False: db = NULL) of one case against the float64 conv, element by element"""
    Cout, _, K = W.shape
    B = sym_h.shape[0]
    x64 = torch.from_numpy(ONEHOT[np.where(sym_h > 14, 4, sym_h)].transpose(0, 2, 1).copy()).double()
    W64 = W.double()
    b64 = None if b is None else b.double()
    sym = torch.from_numpy(sym_h).cuda()
    apps = [x64] + ([x64.flip([1, 2])] if rev else [])
    Lout = (sym_h.shape[1] + 2 * pad - K) // stride + 1
    if fwd:
        got = _run_fwd(sym, W.cuda(), None if b is None else b.cuda(), stride, pad, rev)
        for a, xa in enumerate(apps):
            want = F.conv1d(xa, W64, b64, stride=stride, padding=pad)
            S = F.conv1d(xa.abs(), W64.abs(), None if b is None else b64.abs(), stride=stride, padding=pad)
            assert want.shape == got[a].shape == (B, Cout, Lout), case
            _sum_check(got[a], want, S, 4 * K + 1, f"y app{a}", case, stats)
    if bwd:
        dzs, want_dW, want_db, S_dW, S_db = [], 0.0, 0.0, 0.0, 0.0
        for xa in apps:
            dz = torch.randn((B, Cout, Lout), generator=tg)
            dzs.append(dz.cuda())
            Wl = W64.clone().requires_grad_()
            bl = torch.zeros(Cout, dtype=torch.float64, requires_grad=True)
            gW, gb = torch.autograd.grad(F.conv1d(xa, Wl, bl, stride=stride, padding=pad), (Wl, bl), dz.double())
            sW, sb = torch.autograd.grad(F.conv1d(xa, Wl, bl, stride=stride, padding=pad), (Wl, bl), dz.double().abs())      # (x >= 0)
            want_dW, want_db, S_dW, S_db = want_dW + gW, want_db + gb, S_dW + sW, S_db + sb
        dW, dbv = _run_bwd(sym, dzs[0], dzs[1] if rev else None, Cout, K, stride, pad, db=db)
        n = len(apps) * B * Lout
        _sum_check(dW, want_dW, S_dW, n, "dW", case, stats)
        if db:
            _sum_check(dbv, want_db, S_db, n, "db", case, stats)
        else:
            assert torch.isnan(dbv).all(), case          # db = NULL: nothing written through it
        dW2, db2 = _run_bwd(sym, dzs[0], dzs[1] if rev else None, Cout, K, stride, pad, db=db)
        assert torch.equal(dW, dW2) and (not db or torch.equal(dbv, db2)), case          # fixed summation order: the same bits again


def _weights(tg, Cout, K):
    return torch.randn((Cout, 4, K), generator=tg) / (4 * K) ** 0.5, torch.randn(Cout, generator=tg)


def _length_for(Lout, K, stride, pad):
    """the largest L with that many output positions"""
    return (Lout - 1) * stride + K - 2 * pad + stride - 1


@pytest.mark.parametrize("geom", _geoms(), ids=lambda g: g[0])
def test_indel_first_weight_gradient_beyond_its_256_chunks(geom):
    """tiles = 256 (no workgroup wraps), 257 (one does), 300 (some), 2 * 256 + 5 (all take two tiles, five take three) with one tile per
    row, a full one (Lout = 256) and a cut one (Lout = 200: the last 56 positions of the staged dz row are zero fill); then rows of
    two tiles (Lout = 300) with an odd B: a workgroup's next tile, 256 further, lies 128 rows on in the same half of the row (256 is a
    multiple of 2), so rows of three tiles (Lout = 600) follow, where the next tile also changes its place in the row.  dW and db
    with n = applications * B * Lout terms (the any-order bound: it covers the float32 bins carried across tiles), same bits on a
    second call.
    Observed on an MI355X, kernel error / bound at the element nearest its bound: dW 2.2e-5 / 1.5e+2, db 2.8e-5 / 5.9e+2 (sym4, B = 131,
    two tiles a row): a dropped or doubled tile is of the order of the bound / (B Lout), 4e-3."""
    name, Cout, K, stride, pad, rev, _ = geom
    stats = _Stats(name, tag="indel_first")
    cases = [(Lout, tiles) for Lout in (256, 200) for tiles in (256, 257, 300, 2 * 256 + 5)] + [(300, 131), (600, 87)]
    for Lout, B in cases:
        L = _length_for(Lout, K, stride, pad)
        assert (L + 2 * pad - K) // stride + 1 == Lout
        tiles = B * -(-Lout // 256)
        assert (Lout > 256 and tiles > 256) or tiles == B
        rng = np.random.default_rng(1000 * B + L)
        tg = torch.Generator().manual_seed(3 * B + L)
        W, b = _weights(tg, Cout, K)
        _check(stats, f"{name} B{B} L{L} tiles{tiles}", _random_rows(rng, B, L), W, b, stride, pad, rev, tg, fwd=False)
    stats.show()


@pytest.mark.parametrize("tiles", [4096, 4097, 4096 + 300])
@pytest.mark.parametrize("geom", _geoms()[:2], ids=lambda g: g[0])
def test_indel_first_forward_beyond_its_4096_tiles(geom, tiles):
    """one tile per row (L = 200), tiles on the cap, one beyond and 300 beyond; Cout 4 with both applications and Cout 8; every output
    element against the float64 conv"""
    name, Cout, K, stride, pad, rev, _ = geom
    stats = _Stats(name, tag="indel_first")
    B, L = tiles, 200
    rng = np.random.default_rng(tiles)
    tg = torch.Generator().manual_seed(tiles + Cout)
    W, b = _weights(tg, Cout, K)
    _check(stats, f"{name} B{B} L{L}", _random_rows(rng, B, L), W, b, stride, pad, rev, tg, bwd=False)
    stats.show()


# (name, Cout, K, stride, pad, both applications, B, L)
EDGES = [("K1 pad0", 4, 1, 1, 0, True, 2, 300),
         ("K63: 252 threads, one slice", 4, 63, 1, 31, True, 2, 300),
         ("K33: one slice, 124 idle", 4, 33, 1, 16, True, 2, 300),
         ("K5: 12 slices, 16 idle", 4, 5, 1, 2, True, 2, 300),
         ("Lout1: L + 2 pad = K", 4, 7, 1, 3, True, 2, 1),
         ("Lout1 stride4", 8, 7, 4, 3, False, 2, 3),
         ("Lout255", 4, 7, 1, 3, True, 2, 255),
         ("Lout256", 4, 7, 1, 3, True, 2, 256),
         ("Lout257", 4, 7, 1, 3, True, 2, 257),
         ("Lout257 stride4", 8, 7, 4, 3, False, 2, 4 * 256 + 1),
         ("L < pad", 4, 7, 1, 3, True, 2, 2),
         ("Cout12 both", 12, 7, 1, 3, True, 2, 300),
         ("Cout12 stride3", 12, 5, 3, 1, False, 3, 1000),
         ("stride172: the widest span the backward stages", 4, 7, 172, 3, False, 2, 172 * 299)]


@pytest.mark.parametrize("edge", EDGES, ids=lambda e: e[0].split(":")[0].replace(" ", "_"))
def test_indel_first_geometry_edges(edge):
    """forward and backward at the ends of the geometry the entry accepts; each once more with bias = NULL (forward) and db = NULL
    (backward), which the code accepts: y is then the bare sum, dW is unchanged and nothing is written through db"""
    name, Cout, K, stride, pad, rev, B, L = edge
    stats = _Stats(name.split(":")[0], tag="indel_first")
    rng = np.random.default_rng(K * 1000 + L)
    tg = torch.Generator().manual_seed(K + L + Cout)
    W, b = _weights(tg, Cout, K)
    sym_h = _random_rows(rng, B, L)
    case = f"{name} B{B} L{L}"
    _check(stats, case, sym_h, W, b, stride, pad, rev, tg)
    _check(stats, case + " bias=NULL db=NULL", sym_h, W, None, stride, pad, rev, tg, db=False)
    stats.show()


def test_indel_first_forward_at_its_widest_span():
    """stride 249, K = 7: 65294 bytes of LDS, the largest stride the forward accepts (250 asks for 65549)"""
    stats = _Stats("stride249", tag="indel_first")
    tg = torch.Generator().manual_seed(249)
    W, b = _weights(tg, 4, 7)
    _check(stats, "stride249 B2 L70000", _random_rows(np.random.default_rng(249), 2, 70000), W, b, 249, 3, False, tg, bwd=False)
    stats.show()


def test_indel_first_layer_refuses_a_span_beyond_64_kb_of_lds():
    """refused with a ValueError before any launch: the outputs keep their fill"""
    B, L, Cout, K, pad = 2, 1000, 4, 7, 3
    sym = torch.zeros((B, L), dtype=torch.uint8, device="cuda")
    W, b = torch.zeros((Cout, 4, K), device="cuda"), torch.zeros(Cout, device="cuda")
    lib = _lib.lib()
    for stride, fwd_ok in ((250, False), (173, True)):      # forward: 16 K * 16 + 255 stride + K bytes; backward: 21536 + 255 stride + K
        Lout = (L + 2 * pad - K) // stride + 1
        y = torch.full((B, Cout, Lout), float("nan"), device="cuda")
        if fwd_ok:
            _lib.check(lib.mural_op_indel_first_fwd(sym.data_ptr(), W.data_ptr(), b.data_ptr(), B, L, Cout, K, stride, pad, y.data_ptr(), None, None))
            torch.cuda.synchronize()
            assert torch.equal(y, torch.zeros_like(y))
        else:
            with pytest.raises(ValueError, match="LDS"):
                _lib.check(lib.mural_op_indel_first_fwd(sym.data_ptr(), W.data_ptr(), b.data_ptr(), B, L, Cout, K, stride, pad, y.data_ptr(), None, None))
            torch.cuda.synchronize()
            assert torch.isnan(y).all()
        n = int(lib.mural_op_indel_first_scratch(B, L, Cout, K, stride, pad, 0))
        assert n > 0
        part = torch.full((n,), float("nan"), device="cuda")
        dW, db = torch.full((Cout, 4, K), float("nan"), device="cuda"), torch.full((Cout,), float("nan"), device="cuda")
        with pytest.raises(ValueError, match="LDS"):
            _lib.check(lib.mural_op_indel_first_bwd(sym.data_ptr(), y.data_ptr(), None, B, L, Cout, K, stride, pad, dW.data_ptr(), db.data_ptr(),
                                                    part.data_ptr(), C.c_size_t(n), None))
        torch.cuda.synchronize()
        assert torch.isnan(dW).all() and torch.isnan(db).all() and torch.isnan(part).all()


# ------------------------------------------------------------------------------------------------- symbols -> dense
@pytest.mark.parametrize("n,L", [(1, 1), (5, 51), (1, 257), (-(-(16384 * 256 + 77) // 7), 7)], ids=["1", "255", "257", "beyond_the_grid"])
def test_symbols_to_dense_equals_the_host_gather(n, L):
    """x[b][c][l] = ONEHOT[sym[b][l]][c] bit for bit, bytes above 14 as N; 1, 255 and 257 elements (one workgroup less one thread, one
    workgroup plus one), and the first multiple of 7 from 16384 * 256 + 77 on: every thread of the capped grid takes a second element
    or not, and with L = 7 a round of the grid ends inside a row"""
    rng = np.random.default_rng(n + L)
    sym = rng.integers(0, 15, size=(n, L)).astype(np.uint8)
    over = rng.integers(0, n * L, size=max(1, n * L // 50))
    sym.reshape(-1)[over] = rng.choice(np.array([15, 16, 77, 200, 255], np.uint8), size=len(over))
    sym.reshape(-1)[-1] = 14 if n * L > 1 else 255
    assert n * L in (1, 255, 257) or 16384 * 256 + 77 <= n * L < 16384 * 256 + 77 + 7
    x = torch.full((n, 4, L), float("nan"), device="cuda")
    sd = torch.from_numpy(sym).cuda()
    _lib.check(_lib.lib().mural_op_symbols_to_dense(sd.data_ptr(), n, L, x.data_ptr(), None))
    torch.cuda.synchronize()
    want = torch.from_numpy(ONEHOT[np.where(sym > 14, 4, sym)].transpose(0, 2, 1).copy())
    assert torch.equal(x.cpu().view(torch.int32), want.view(torch.int32)), (n, L)


def test_symbols_to_dense_of_no_rows_returns_cleanly():
    x = torch.full((4,), float("nan"), device="cuda")
    _lib.check(_lib.lib().mural_op_symbols_to_dense(None, 0, 7, None, None))
    _lib.check(_lib.lib().mural_op_symbols_to_dense(x.data_ptr(), 0, 7, x.data_ptr(), None))
    torch.cuda.synchronize()
    assert torch.isnan(x).all()
    with pytest.raises(ValueError):
        _lib.check(_lib.lib().mural_op_symbols_to_dense(x.data_ptr(), -1, 7, x.data_ptr(), None))
