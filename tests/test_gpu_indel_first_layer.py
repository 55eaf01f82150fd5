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
    _lib.check(_lib.lib().mural_op_indel_first_fwd(sym.data_ptr(), W.data_ptr(), b.data_ptr(), B, L, Cout, K, stride, pad, y.data_ptr(),
                                                   yr.data_ptr() if rev else None, None))
    torch.cuda.synchronize()
    return y, yr


def _run_bwd(sym, dz, dzr, Cout, K, stride, pad):
    B, L = sym.shape
    n = int(_lib.lib().mural_op_indel_first_scratch(B, L, Cout, K, stride, pad, int(dzr is not None)))
    assert n > 0
    part = torch.full((n,), float("nan"), device="cuda")
    dW = torch.full((Cout, 4, K), float("nan"), device="cuda")
    db = torch.full((Cout,), float("nan"), device="cuda")
    _lib.check(_lib.lib().mural_op_indel_first_bwd(sym.data_ptr(), dz.data_ptr(), dzr.data_ptr() if dzr is not None else None, B, L, Cout, K,
                                                   stride, pad, dW.data_ptr(), db.data_ptr(), part.data_ptr(), C.c_size_t(n), None))
    torch.cuda.synchronize()
    return dW, db


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
