"""The ``mural_op_*`` training building blocks of include/mural_hip.h one by one against the same operation in float64 torch on the
CPU (``torch.nn.functional`` + autograd): every code path of csrc/train_ops.hip that the model fixtures never reach (pool windows on
both sides of 16 / 64, overlapping windows, the dense tile and its scalar fall-backs, ragged weight-gradient waves, the float4 and
scalar BatchNorm sums, run-time class counts, embedding tables beyond the LDS budget).

Tolerances are derived, never tuned:
  * operations without rounding (pool values / indices, gathers, relayouts, masks, dropout's kept values) are compared with
    ``torch.equal``;
  * float32 sums of n terms may differ from float64 by 2 (n + 2) 2^-24 sum|a_k b_k| per output element: the forward error bound of
    any summation order, doubled for fma / non-fma products and the final rounding (``_sum_check``).  A dropped or doubled term is
    of the order sum|a_k b_k| / n;
  * everything else (BatchNorm chain, Head, SiLU / Softplus) may be 8 times as far from float64 as torch's own float32 CPU result
    on the same inputs, at least 4 ulp of the output's largest magnitude (``_loose``): expf / logf / rsqrt differ by a few ulp
    between libraries.  The measured quantity is the reference, never the kernel.  BatchNorm's mean, dgamma and dbeta are sums, but
    the kernels accumulate them in double and round once, so the summation bound (n + 2 roundings) would be the looser of the two
    for them: they are judged by this rule like the rest of the chain.
Each test prints the worst reference error / kernel error / bound per output (``pytest -s``)."""
import ctypes as C
import math

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from mural_amd import _lib
from mural_amd.model import train_ops as T
from tests._parity import EPS, MOMENTUM, NAN, _Stats, _loose, _sum_check

pytestmark = pytest.mark.gpu


def _cuda(t):
    return None if t is None else t.cuda()


# ------------------------------------------------------------------------------------------------------------------ max-pool
# (k, s, p, L): both sides of the 16-load window (k <= 16), the serial loop (17..63) and the wave-per-window kernel (k >= 64); s = k,
# s > k (gather backward), s < k (overlapping windows: atomics into a zeroed dx); p = 0 and k // 2; lengths that are no multiple of
# s (floor mode drops the tail) and lengths whose last window is cut by the right padding; the global form as (L, L, 0, L)
POOL_CASES = [(1, 1, 0, 7), (2, 2, 0, 101), (2, 2, 1, 100), (15, 15, 0, 250), (15, 15, 7, 230), (16, 16, 0, 250), (16, 16, 8, 241),
              (17, 17, 0, 250), (17, 17, 8, 251), (63, 63, 0, 300), (63, 63, 31, 280), (64, 64, 0, 300), (64, 64, 32, 280),
              (65, 65, 0, 300), (65, 65, 32, 333), (130, 130, 0, 400), (130, 130, 65, 400),
              (2, 3, 0, 100), (16, 20, 8, 250), (17, 19, 8, 250), (64, 70, 0, 300), (64, 70, 32, 300),
              (3, 2, 1, 101), (16, 5, 8, 250), (17, 5, 8, 250), (64, 16, 0, 300), (64, 16, 32, 301), (130, 7, 65, 400),
              (63, 63, 0, 63), (64, 64, 0, 64), (102, 102, 0, 102), (1000, 1000, 0, 1000)]


def _pool_input(rng, rows, L, kind):
    x = torch.randn((1, rows, L), generator=rng)
    if kind != "normal":        # one decimal of relu(randn): windows hold their maximum more than once, the narrow ones often at 0
        x = (torch.relu(x) * 10).round() / 10
    if kind == "capped ties":   # ... capped at 1.0, which a sixth of the values reach: wide windows hold their maximum in many lanes
        x = x.clamp(max=1.0)
    return x


def _pool_reference(x, k, s, p, g):
    """float64 torch: values, first-maximum indices, gradient, sum of |g| per input column, windows whose maximum is tied, windows
    whose maximum sits in two or more lanes of the wide kernel (lane = position in the window mod 64)"""
    x64 = x.double().requires_grad_()
    y, idx = F.max_pool1d(x64, k, s, p, return_indices=True)
    (dx,) = torch.autograd.grad(y, x64, g.double(), retain_graph=True)
    (S,) = torch.autograd.grad(y, x64, g.double().abs())
    win = F.pad(x64.detach(), (p, p), value=-math.inf).unfold(-1, k, s)
    hit = win == y.detach().unsqueeze(-1)
    tied = hit.sum(-1) >= 2
    lanes = F.pad(hit, (0, -k % 64)).unflatten(-1, (-1, 64)).any(-2).sum(-1) >= 2
    return y.detach(), idx, dx, S, tied, lanes


def test_maxpool_forward_and_backward_against_torch_float64():
    """y and the argmax bit for bit (first maximum wins, also across the lanes of the wide kernel), arg = NULL, dx with NaN (disjoint
    windows: fully written) or zero (overlapping windows) pre-fill, through the C entry and through train_ops.MaxPool.
    torch propagates a NaN input, these kernels skip it (documented at the declaration): no NaN inputs here.
    Observed on an MI355X: every exact comparison holds; dx of overlapping windows: kernel error 3.2e-7 against a summation bound of
    2.2e-6 at the element nearest its bound (k = 64, s = 16)."""
    rng = torch.Generator().manual_seed(21)
    stats = _Stats("maxpool")
    lib = _lib.lib()
    n_tied = n_out = n_cut = 0
    for k, s, p, L in POOL_CASES:
        Lout = (L + 2 * p - k) // s + 1
        n_cut += (Lout - 1) * s - p + k > L
        for rows in (1, 37):
            for kind in ("normal", "ties", "capped ties"):
                case = dict(k=k, s=s, p=p, L=L, rows=rows, input=kind)
                x = _pool_input(rng, rows, L, kind)
                g = torch.randn((1, rows, Lout), generator=rng)
                want_y, want_idx, want_dx, S, tied, lanes = _pool_reference(x, k, s, p, g)
                if kind == "capped ties":
                    n_tied, n_out = n_tied + int(tied.sum()), n_out + tied.numel()
                    # the wide kernel's first-maximum rule is decided between lanes: most of its windows must put it to the test
                    assert k < 64 or 2 * int(lanes.sum()) > lanes.numel(), ("too few maxima tied across lanes", case)
                xd, gd = x.cuda(), g.cuda()
                st = T._stream(xd)
                y = torch.full((1, rows, Lout), NAN, device="cuda")
                arg = torch.full((1, rows, Lout), -7, dtype=torch.int32, device="cuda")
                T._call("mural_op_maxpool_fwd", xd, rows, L, k, s, p, y, arg, st)
                assert torch.equal(y.cpu().double(), want_y), case
                assert torch.equal(arg.cpu().long(), want_idx), case
                y0 = torch.full((1, rows, Lout), NAN, device="cuda")
                T._call("mural_op_maxpool_fwd", xd, rows, L, k, s, p, y0, None, st)
                assert torch.equal(y0, y), ("arg = NULL", case)
                overlap = s < k
                assert lib.mural_op_maxpool_bwd_needs_zero(k, s) == int(overlap), case
                dx = torch.zeros((1, rows, L), device="cuda") if overlap else torch.full((1, rows, L), NAN, device="cuda")
                T._call("mural_op_maxpool_bwd", gd, arg, rows, L, Lout, k, s, p, dx, st)
                # through the autograd Function (global form: k = None, a (B, C) result)
                glob = k == L and s == L and p == 0
                xa = xd.clone().requires_grad_()
                ya = T.MaxPool.apply(xa, *((None, None, None) if glob else (k, s, p)))
                assert torch.equal(ya.reshape(y.shape), y), case
                ya.backward(gd.reshape(ya.shape))
                for got, name in ((dx, "dx"), (xa.grad, "dx (Function)")):
                    if overlap:
                        _sum_check(got, want_dx, S, -(-k // s), name + " overlapping", case, stats)
                    else:
                        assert torch.equal(got.cpu().double(), want_dx), (name, case)
    assert n_cut >= 4, "the case table lost its windows cut by the right padding"
    assert n_tied > n_out // 2, f"the capped ties input ties only {n_tied} of {n_out} windows"
    stats.show()


# ------------------------------------------------------------------------------------------------------------------ Linear
# (B, I, O): below / at / above the 64-row tile, the largest tile (256 x 256: 320 KB of operands, LDS above 64 KB), one side outside
# the tile (forward and dx take different kernels), 2 outputs, and a batch that gives every weight-gradient wave several 32-row
# steps plus a ragged tail
LINEAR_CASES = [(1, 1, 1), (2, 5, 3), (63, 40, 75), (64, 45, 16), (65, 95, 17), (130, 150, 75), (37, 256, 256), (37, 257, 8),
                (37, 8, 257), (19, 150, 2), (1024 + 5, 33, 4)]


def test_linear_forward_and_backward_against_torch_float64():
    """y, dx, dW, db of every case through train_ops.Linear and through the C entry with NaN-filled outputs; bias = NULL and
    dx = NULL once each (dW and db are still written).
    Observed on an MI355X, kernel error / summation bound at the element nearest its bound (torch's float32 is not measured for
    a summation bound): y 4.9e-7 / 3.5e-6 at (37, 8, 257), dx 6.8e-9 / 3.1e-8 at (19, 150, 2), dW 8.2e-8 / 6.9e-7 and db 3.0e-8 / 6.8e-7 at
    (2, 5, 3), y without bias 1.1e-6 / 7.7e-5.  No element uses more than a quarter of its bound."""
    rng = torch.Generator().manual_seed(22)
    stats = _Stats("linear")
    for B, I, O in LINEAR_CASES:
        case = dict(B=B, I=I, O=O)
        x = torch.randn((B, I), generator=rng)
        W = torch.randn((O, I), generator=rng) / I ** 0.5
        b = torch.randn(O, generator=rng)
        g = torch.randn((B, O), generator=rng)
        x64, W64, b64, g64 = x.double(), W.double(), b.double(), g.double()
        want = dict(y=x64 @ W64.T + b64, dx=g64 @ W64, dW=g64.T @ x64, db=g64.sum(0))
        Sy = x64.abs() @ W64.abs().T
        S = dict(y=Sy + b64.abs(), dx=g64.abs() @ W64.abs(), dW=g64.abs().T @ x64.abs(), db=g64.abs().sum(0))
        n = dict(y=I + 1, dx=O, dW=B, db=B)
        xa, Wa, ba = x.cuda().requires_grad_(), W.cuda().requires_grad_(), b.cuda().requires_grad_()
        ya = T.Linear.apply(xa, Wa, ba)
        ya.backward(g.cuda())
        for name, got in (("y", ya), ("dx", xa.grad), ("dW", Wa.grad), ("db", ba.grad)):
            _sum_check(got, want[name], S[name], n[name], name, case, stats)
        xd, Wd, bd, gd = x.cuda(), W.cuda(), b.cuda(), g.cuda()
        st = T._stream(xd)
        no_bias, no_dx = (B, I, O) == (65, 95, 17), (B, I, O) == (63, 40, 75)
        y = torch.full((B, O), NAN, device="cuda")
        T._call("mural_op_linear_fwd", xd, Wd, None if no_bias else bd, B, I, O, y, st)
        if no_bias:
            _sum_check(y, x64 @ W64.T, Sy, I, "y (bias = NULL)", case, stats)
        else:
            assert torch.equal(y, ya), case
        dx = None if no_dx else torch.full((B, I), NAN, device="cuda")
        dW, db = torch.full((O, I), NAN, device="cuda"), torch.full((O,), NAN, device="cuda")
        T._call("mural_op_linear_bwd", gd, xd, Wd, B, I, O, dx, dW, db, st)
        for name, got in (("dx", dx), ("dW", dW), ("db", db)):
            if got is not None:
                _sum_check(got, want[name], S[name], n[name], name + " (C entry)", case, stats)
    stats.show()


# ------------------------------------------------------------------------------------------------------------------ Embedding
@pytest.mark.parametrize("rows", [5, 65, 4097, 7680, 7681, 16385])
def test_embedding_forward_and_backward_against_torch_float64(rows):
    """Gather bit for bit, dE against the float64 index_add for tables of local_order 1, 3, 6 (82 KB of LDS: above the 64 KB a
    kernel gets without asking) and 7 (328 KB: no LDS staging, atomics straight into dE), and for 7680 / 7681 rows, the last table that
    is staged (150 KB exactly) and the first that is not; uniform indices, all indices equal (every
    atomic on the same five addresses) and indices that include the last (padding) row; the documented clamp of indices outside
    the table.
    Observed on an MI355X: the gather is exact; dE, kernel error / summation bound at the element nearest its bound:
    5 rows 4.1e-8 / 4.1e-7, 65 rows 6.0e-7 / 3.9e-6, 4097 rows 2.3e-7 / 1.3e-6, 7680 rows 2.4e-7 / 1.6e-6,
    7681 rows 1.2e-7 / 6.9e-7, 16385 rows 3.6e-7 / 2.5e-6."""
    rng = torch.Generator().manual_seed(23 + rows)
    stats = _Stats("embedding")
    E = torch.randn((rows, 5), generator=rng)
    Ed = E.cuda()
    for cols in (1, 9, 19):
        for B in (1, 40, 300, 700):          # 700 x 19 x 5 = 66 500 gradients: beyond one round of the staged kernel's 256 workgroups of 256
            for dist in ("uniform", "equal", "last row"):
                case = dict(rows=rows, cols=cols, B=B, indices=dist)
                cat = torch.randint(0, rows, (B, cols), generator=rng)
                if dist == "equal":
                    cat[:] = rows // 2
                elif dist == "last row":
                    cat[torch.rand((B, cols), generator=rng) < 0.3] = rows - 1
                    cat[0, 0] = rows - 1
                g = torch.randn((B, cols * 5), generator=rng)
                Ea = Ed.clone().requires_grad_()
                y = T.Embedding.apply(cat.cuda(), Ea)
                assert torch.equal(y.cpu(), E[cat].reshape(B, cols * 5)), case
                y.backward(g.cuda())
                flat = cat.flatten()
                want = torch.zeros((rows, 5), dtype=torch.float64).index_add_(0, flat, g.double().view(-1, 5))
                S = torch.zeros((rows, 5), dtype=torch.float64).index_add_(0, flat, g.double().abs().view(-1, 5))
                n = torch.bincount(flat, minlength=rows).double().unsqueeze(1)
                _sum_check(Ea.grad, want, S, n, "dE", case, stats)
    # indices outside the table read row 0 / the last row (mural_hip.h)
    cat = torch.randint(0, rows, (7, 9), generator=rng)
    cat[0, 0], cat[6, 8] = -3, rows + 7
    y = T.Embedding.apply(cat.cuda(), Ed)
    assert torch.equal(y.cpu(), E[cat.clamp(0, rows - 1)].reshape(7, 45)), rows
    stats.show()


# ------------------------------------------------------------------------------------------------------------------ BatchNorm
# (B, C, L, relu, input, misaligned): L = 1 runs as (B, C) through train_ops.Bn2d, the others as (B, C, L) through indel_train.BatchNorm;
# L on both sides of the float4 sums (L % 4 == 0); "offset": 100 + randn per channel (E[x^2] - mean^2 cancels seven digits) with one
# constant channel (variance 0: invstd = 1 / sqrt(eps)); misaligned: x starts one float into its storage
BN_CASES = [(2, 1, 1, 0, "plain", 0), (2, 75, 1, 1, "plain", 0), (2, 5, 1, 0, "offset", 0), (3, 5, 1, 1, "offset", 0),
            (3, 150, 1, 0, "plain", 0), (37, 32, 1, 1, "plain", 0), (37, 150, 1, 1, "offset", 0), (37, 75, 1, 0, "offset", 0),
            (2, 5, 3, 0, "plain", 0), (3, 75, 3, 1, "offset", 0), (3, 1, 4, 1, "plain", 0), (37, 5, 4, 0, "offset", 0),
            (37, 5, 4, 0, "offset", 1), (2, 150, 4, 1, "plain", 0), (2, 150, 4, 1, "plain", 1), (3, 32, 8, 1, "plain", 0),
            (3, 32, 8, 1, "plain", 1), (2, 75, 8, 0, "offset", 0), (2, 75, 8, 0, "offset", 1), (37, 1, 8, 0, "plain", 0),
            (37, 32, 250, 0, "offset", 0), (3, 150, 250, 1, "plain", 0), (2, 32, 251, 1, "offset", 0), (37, 5, 251, 0, "plain", 0),
            (37, 5, 251, 0, "plain", 1), (3, 75, 251, 1, "plain", 0),
            # 527 250 elements: beyond one round of bn_backward's apply launch (capped at 2048 workgroups of 256 elements)
            (37, 57, 250, 1, "plain", 0)]


def _bn_reference(x, gamma, beta, rm, rv, g, relu, dtype):
    """nn.BatchNorm1d in train mode (momentum 0.1, unbiased running variance) over act(x), and its autograd gradients"""
    x = x.detach().to(dtype).clone().requires_grad_()
    bn = torch.nn.BatchNorm1d(x.shape[1], eps=EPS, momentum=MOMENTUM).to(dtype).train()
    with torch.no_grad():
        bn.weight.copy_(gamma)
        bn.bias.copy_(beta)
        bn.running_mean.copy_(rm)
        bn.running_var.copy_(rv)
    a = torch.relu(x) if relu else x
    y = bn(a)
    y.backward(g.to(dtype))
    a = a.detach()
    mean, var = a.mean((0, 2)), a.var((0, 2), unbiased=False)
    invstd = (var + EPS).rsqrt()
    scale = bn.weight.detach() * invstd
    return dict(y=y.detach(), dx=x.grad, dgamma=bn.weight.grad, dbeta=bn.bias.grad, running_mean=bn.running_mean,
                running_var=bn.running_var, mean=mean, invstd=invstd, scale=scale, shift=bn.bias.detach() - mean * scale)


def test_batchnorm_chain_against_torch_float64():
    """bn_stats -> bn_finalize -> bn_apply -> bn_backward through the C entries (NaN-filled outputs; y, scale / shift / mean /
    invstd, running statistics, dx, dgamma, dbeta; add1 / add2; have_sums = 1) and through the autograd Functions.  At B = 2 the
    normalised values are +-1 up to eps / var and dx is a difference of nearly equal numbers: torch's own float32 error grows with
    the conditioning and the bound follows it.
    Observed on an MI355X, torch float32 / kernel error from float64 at the case nearest its bound: y 4.4e-6 / 6.2e-6, scale
    1.9e-5 / 1.9e-5, shift 9.2e-7 / 9.2e-7, mean 3.8e-6 / 3.8e-6, invstd 1.7e-5 / 1.7e-5, running_mean 6.2e-7 / 6.0e-7, running_var
    4.8e-8 / 4.2e-8, dx 1.3e-6 / 3.5e-6 (B = 2, C = 150, L = 4, relu), dgamma 2.1e-7 / 3.1e-7, dbeta 2.4e-7 / 2.4e-7; the Functions give
    the same figures.  have_sums = 1 against have_sums = 0: dx 1.4e-6, dgamma 4.8e-7, dbeta 0."""
    from mural_amd.model.indel_train import BatchNorm
    rng = torch.Generator().manual_seed(24)
    stats = _Stats("batchnorm")
    for B, Cn, L, relu, kind, misaligned in BN_CASES:
        case = dict(B=B, C=Cn, L=L, relu=relu, input=kind, misaligned=misaligned)
        x = torch.randn((B, Cn, L), generator=rng)
        if kind == "offset":
            x += 100.0
            if Cn >= 2:
                x[:, Cn // 2] = 0.5
        gamma = 1 + 0.3 * torch.randn(Cn, generator=rng)
        beta = 0.3 * torch.randn(Cn, generator=rng)
        rm, rv = 0.1 * torch.randn(Cn, generator=rng), 1 + 0.2 * torch.rand(Cn, generator=rng)
        g = torch.randn((B, Cn, L), generator=rng)
        a1, a2 = torch.randn((B, Cn, L), generator=rng), torch.randn((B, Cn, L), generator=rng)
        want = _bn_reference(x, gamma, beta, rm, rv, g, relu, torch.float64)
        ref = _bn_reference(x, gamma, beta, rm, rv, g, relu, torch.float32)
        if kind == "offset" and Cn >= 2:
            assert abs(float(want["invstd"][Cn // 2]) - EPS ** -0.5) <= 1e-9, case             # the constant channel: variance exactly 0

        if misaligned:
            buf = torch.empty(x.numel() + 1, device="cuda")
            xd = buf[1:].view(B, Cn, L)
            xd.copy_(x)
            assert xd.is_contiguous() and xd.data_ptr() % 16 == 4, case
        else:
            xd = x.cuda()
        gd, gam_d, bet_d = g.cuda(), gamma.cuda(), beta.cuda()
        st = T._stream(xd)
        acc = torch.zeros((T.BN_SLOTS, 2, Cn), dtype=torch.float64, device="cuda")
        T._call("mural_op_bn_stats", xd, B, Cn, L, relu, acc, st)
        got = {k: torch.full((Cn,), NAN, device="cuda") for k in ("scale", "shift", "mean", "invstd", "dgamma", "dbeta")}
        got["running_mean"], got["running_var"] = rm.cuda(), rv.cuda()
        T._call("mural_op_bn_finalize", acc, float(B * L), Cn, gam_d, bet_d, EPS, MOMENTUM, got["running_mean"], got["running_var"],
                got["scale"], got["shift"], got["mean"], got["invstd"], st)
        got["y"] = torch.full((B, Cn, L), NAN, device="cuda")
        T._call("mural_op_bn_apply", xd, B, Cn, L, relu, got["scale"], got["shift"], got["y"], st)

        def backward(add1, add2, sums):
            acc_b = torch.zeros((T.BN_SLOTS, 2, Cn), dtype=torch.float64, device="cuda")
            if sums is not None:            # split over two accumulator copies: the reader sums all of them
                acc_b[0], acc_b[T.BN_SLOTS - 1] = (0.25 * sums).cuda(), (0.75 * sums).cuda()
            out = [torch.full((B, Cn, L), NAN, device="cuda"), torch.full((Cn,), NAN, device="cuda"), torch.full((Cn,), NAN, device="cuda")]
            T._call("mural_op_bn_backward", gd, xd, B, Cn, L, relu, got["mean"], got["invstd"], gam_d, acc_b, int(sums is not None),
                    _cuda(add1), _cuda(add2), *out, st)
            return out

        got["dx"], got["dgamma"], got["dbeta"] = backward(None, None, None)
        for name in ("y", "scale", "shift", "mean", "invstd", "running_mean", "running_var", "dx", "dgamma", "dbeta"):
            _loose(got[name], want[name], ref[name], name, case, stats)
        dx_add, dgamma_add, dbeta_add = backward(a1, a2, None)
        assert torch.equal(dx_add, (got["dx"] + a1.cuda()) + a2.cuda()), ("add1 / add2", case)
        assert torch.equal(dgamma_add, got["dgamma"]) and torch.equal(dbeta_add, got["dbeta"]), ("add1 / add2", case)
        dx_one, _, _ = backward(a1, None, None)
        assert torch.equal(dx_one, got["dx"] + a1.cuda()), ("add1", case)
        # sum(dz) and sum(dz * xhat) handed in: the float64 sums are the reference's dbeta and dgamma
        sums = torch.stack([want["dbeta"], want["dgamma"]])
        for name, t in zip(("dx", "dgamma", "dbeta"), backward(None, None, sums)):
            _loose(t, want[name], ref[name], name + " (have_sums)", case, stats)
            # ... and next to the kernel's own sums (accumulated in double: they differ from these by the rounding of xhat alone),
            # within the same bound: a branch that ignored the accumulator does not pass by being near float64 on its own
            _loose(t, want[name], ref[name], name + " (have_sums against have_sums = 0)", case, stats, other=got[name])

        bn = torch.nn.BatchNorm1d(Cn, eps=EPS, momentum=MOMENTUM).cuda().train()
        with torch.no_grad():
            bn.weight.copy_(gamma)
            bn.bias.copy_(beta)
            bn.running_mean.copy_(rm)
            bn.running_var.copy_(rv)
        xa = xd.detach().requires_grad_() if misaligned else xd.clone().requires_grad_()
        if L == 1:
            ya = T.Bn2d.apply(xa.view(B, Cn), bn.weight, bn.bias, bn, bool(relu)).view(B, Cn, 1)
        else:
            ya = BatchNorm.apply(xa, bn.weight, bn.bias, bn, bool(relu))
        ya.backward(gd)
        T.flush_bn_ticks()
        assert int(bn.num_batches_tracked) == 1, case
        for name, t in (("y", ya), ("dx", xa.grad.view(B, Cn, L)), ("dgamma", bn.weight.grad), ("dbeta", bn.bias.grad),
                        ("running_mean", bn.running_mean), ("running_var", bn.running_var)):
            _loose(t, want[name], ref[name], name + " (Function)", case, stats)
    stats.show()


# ------------------------------------------------------------------------------------------------------------------ Head
def _head_prob(loc, mid, lar):
    p = (torch.softmax(mid, 1) + torch.softmax(lar, 1)) / 2
    return p if loc is None else (torch.softmax(loc, 1) + p) / 2


def _head_reference(loc, mid, lar, g, dtype):
    ts = [None if t is None else t.detach().to(dtype).clone().requires_grad_() for t in (loc, mid, lar)]
    out = torch.log(torch.clamp(_head_prob(*ts), min=1e-9))
    out.backward(g.to(dtype))
    return dict(out=out.detach(), dloc=None if loc is None else ts[0].grad, dmid=ts[1].grad, dlar=ts[2].grad)


def test_head_forward_and_backward_against_torch_float64():
    """log(clamp(mixture of the towers' softmaxes, 1e-9)) for 1..16 classes (the 4-class and the run-time-count kernels), with and
    without the local tower, batches around one 64-row workgroup; every third row carries a class 80 below the others in all
    towers: its probability is below the clamp, out = log(1e-9) there and that class passes no gradient.  The mixed probability
    stays a factor of 10 away from 1e-9 (checked on the float64 reference): the edge of the clamp is not under test.
    Observed on an MI355X, torch float32 / kernel error from float64 at the case nearest its bound: out 8.1e-7 / 1.9e-6, dloc
    4.7e-7 / 7.0e-7, dmid 2.2e-7 / 5.4e-7, dlar 2.9e-8 / 6.5e-8."""
    rng = torch.Generator().manual_seed(25)
    stats = _Stats("head")
    for nc in (1, 2, 3, 4, 5, 16):
        for B in (1, 63, 64, 65, 300):
            for with_loc in (True, False):
                case = dict(nc=nc, B=B, loc=with_loc)
                z = [3.0 * torch.randn((B, nc), generator=rng) for _ in range(3)]
                spread = torch.zeros((B, nc))
                if nc >= 2:
                    r = torch.arange(0, B, 3)
                    spread[r, r % nc] = -80.0

                def towers(zz):
                    loc, mid, lar = [t + spread for t in zz]
                    return (loc if with_loc else None), mid, lar

                p = _head_prob(*[None if t is None else t.double() for t in towers(z)])
                near = ((p > 1e-10) & (p < 1e-8)).any(1)
                z = [torch.where(near.unsqueeze(1), 0.25 * t, t) for t in z]       # rows that came near the clamp: a quarter of the spread
                loc, mid, lar = towers(z)
                p = _head_prob(*[None if t is None else t.double() for t in (loc, mid, lar)])
                assert not ((p > 1e-10) & (p < 1e-8)).any(), case
                assert nc == 1 or (p < 1e-10).any(), case
                g = torch.randn((B, nc), generator=rng)
                want = _head_reference(loc, mid, lar, g, torch.float64)
                ref = _head_reference(loc, mid, lar, g, torch.float32)
                assert nc == 1 or float((want["out"] - math.log(1e-9)).abs().min()) <= 1e-12, case
                la, ma, ra = [None if t is None else t.cuda().requires_grad_() for t in (loc, mid, lar)]
                out = T.Head.apply(la, ma, ra)
                out.backward(g.cuda())
                _loose(out, want["out"], ref["out"], "out", case, stats)
                for name, t in (("dloc", la), ("dmid", ma), ("dlar", ra)):
                    if t is not None:
                        _loose(t.grad, want[name], ref[name], name, case, stats)
    for nc in (0, 17):          # rejected before any launch
        t = torch.zeros((4, max(nc, 1)), device="cuda")
        with pytest.raises(ValueError):
            T._call("mural_op_head_fwd", t, t, t, 4, nc, torch.empty_like(t), T._stream(t))
        with pytest.raises(ValueError):
            T._call("mural_op_head_bwd", t, t, t, t, 4, nc, torch.empty_like(t), torch.empty_like(t), torch.empty_like(t), T._stream(t))
    stats.show()


# ------------------------------------------------------------------------------------------------------------------ activations
ACT_BANDS = [(-101.0, -20.0), (-20.0, -5.0), (-5.0, 5.0), (5.0, 20.0), (20.0, 101.0)]      # (lo, hi]: the bound is taken per band of x


def _act_reference(x, g, kind, dtype):
    x = x.detach().to(dtype).clone().requires_grad_()
    y = (torch.relu, F.silu, F.softplus)[kind - 1](x)
    y.backward(g.to(dtype))
    return y.detach(), x.grad


def test_activations_against_torch_float64():
    """ReLU exactly, SiLU and Softplus (beta 1, linear above 20) and their derivatives on [-100, 100] with 0, +-20 and +-88 among the
    points, the bound taken separately per band of x so that the small outputs of the tails are not judged by the scale of the
    large ones; 1, 1023 and 1024 * 4 * 4096 + 3 elements (the last: every thread of the capped grid takes a second round), the long
    one as repetitions of a 1021-element base whose reference is computed once.
    Observed on an MI355X, torch float32 / kernel error from float64 in the band nearest its bound: SiLU y 9.3e-7 / 9.3e-7 on
    (5, 20], dx 2.6e-7 / 4.4e-7 on (-5, 5]; Softplus y 2.5e-7 / 2.5e-7 on (-5, 5], dx 7.6e-8 / 2.7e-7 on (-5, 5]; in the tails
    (|x| > 20) both sit at the same 1e-15 or below, and Softplus above 20 is exact.  ReLU is exact."""
    from mural_amd.model.indel_train import Act
    rng = torch.Generator().manual_seed(26)
    stats = _Stats("activations")
    special = torch.tensor([0.0, -0.0, 20.0, -20.0, 88.0, -88.0, 100.0, -100.0, 19.999998, 20.000002])
    base = torch.cat([special, 200.0 * torch.rand(1021 - len(special), generator=rng) - 100.0])
    base = base[torch.randperm(1021, generator=rng)]
    gbase = torch.randn(1021, generator=rng)
    n_long = 1024 * 4 * 4096 + 3
    reps, tail = divmod(n_long, 1021)
    for kind in (1, 2, 3):
        want_y, want_dx = _act_reference(base, gbase, kind, torch.float64)
        ref_y, ref_dx = _act_reference(base, gbase, kind, torch.float32)
        for n in (1, 1023, n_long):
            case = dict(kind=kind, n=n)
            if n == 1:
                x, g = base[6:7].clone(), gbase[6:7].clone()
                xd, gd = x.cuda(), g.cuda()
            elif n == 1023:
                x, g = torch.cat([base, base[:2]]), torch.cat([gbase, gbase[:2]])
                xd, gd = x.cuda(), g.cuda()
            else:
                xd = torch.cat([base.cuda().repeat(reps), base[:tail].cuda()])
                gd = torch.cat([gbase.cuda().repeat(reps), gbase[:tail].cuda()])
            xa = xd.requires_grad_()
            ya = Act.apply(xa, kind)
            ya.backward(gd)
            assert ya.shape == (n,), case
            for name, got, want, ref in (("y", ya.detach(), want_y, ref_y), ("dx", xa.grad, want_dx, ref_dx)):
                if n == 1:
                    folded, idx = got.view(1, 1), slice(6, 7)
                elif n == 1023:
                    assert torch.equal(got[1021:], got[:2]), case
                    folded, idx = got[:1021].view(1, 1021), slice(0, 1021)
                else:
                    assert torch.equal(got[reps * 1021:], got[:tail]), case
                    folded, idx = got[:reps * 1021].view(reps, 1021), slice(0, 1021)
                    assert torch.equal(folded, folded[:1].expand_as(folded)), (name, case)     # every repetition: the same bits
                    folded = folded[:1]
                got0 = folded[0].cpu()
                if kind == 1:
                    assert torch.equal(got0, ref[idx]) and torch.equal(got0.double(), want[idx]), (name, case)
                    continue
                xs = base[idx]
                for lo, hi in ACT_BANDS:
                    m = (xs > lo) & (xs <= hi)
                    if m.any():
                        _loose(got0[m], want[idx][m], ref[idx][m], f"{('', 'relu', 'silu', 'softplus')[kind]} {name} ({lo:g}, {hi:g}]", case, stats)
    t = torch.zeros(8, device="cuda")
    for kind in (0, 4):
        with pytest.raises(ValueError):
            T._call("mural_op_act_fwd", t, 8, kind, torch.empty_like(t), T._stream(t))
        with pytest.raises(ValueError):
            T._call("mural_op_act_bwd", t, t, 8, kind, torch.empty_like(t), T._stream(t))
    stats.show()


# ------------------------------------------------------------------------------------------------------------------ dropout
def test_dropout_values_mask_and_keep_rate():
    """p = 0 is the identity; a kept element is x * (1 / (1 - p)) in float32 exactly; the backward with the same seed zeroes exactly
    the forward's positions; the keep rate over 2^20 elements lies within 5 standard deviations of 1 - p."""
    rng = torch.Generator().manual_seed(27)
    n = 1 << 20
    x = (0.5 + torch.rand(n, generator=rng)).cuda()             # no zeros: a zero output is a dropped element
    g = (0.5 + torch.rand(n, generator=rng)).cuda()
    assert torch.equal(T.Dropout.apply(x, 0.0, 99), x)
    for p in (0.1, 0.5):
        xa = x.clone().requires_grad_()
        y = T.Dropout.apply(xa, p, 4321)
        y.backward(g)
        keep = y != 0
        scale = torch.tensor(1.0, device="cuda") / (torch.tensor(1.0, device="cuda") - torch.tensor(p, dtype=torch.float32, device="cuda"))
        assert torch.equal(y, torch.where(keep, x * scale, torch.zeros_like(x))), p
        assert torch.equal(xa.grad != 0, keep), p
        assert torch.equal(xa.grad, torch.where(keep, g * scale, torch.zeros_like(g))), p
        rate, sigma = float(keep.double().mean()), math.sqrt(p * (1 - p) / n)
        print(f"[train_ops] dropout      p {p}: keep rate {rate:.6f}, {abs(rate - (1 - p)) / sigma:.2f} sigma from {1 - p}")
        assert abs(rate - (1 - p)) <= 5 * sigma, (p, rate)


# ------------------------------------------------------------------------------------------------------------------ relayout, ReLU mask
def test_relayout_and_relu_mask_are_exact():
    rng = torch.Generator().manual_seed(28)
    for Cout, Cin, K in ((1, 1, 1), (16, 4, 5), (24, 24, 4), (64, 32, 3)):
        W = torch.randn((Cout, Cin, K), generator=rng)
        Wd = W.cuda()
        for dgrad, want in ((0, W.permute(1, 2, 0)), (1, W.flip(2).permute(0, 2, 1))):          # [Cin][K][Cout] | [Cout][K flipped][Cin]
            wt = torch.full((W.numel(),), NAN, device="cuda")
            T._call("mural_op_relayout", Wd, wt, Cout, Cin, K, dgrad, T._stream(Wd))
            assert torch.equal(wt.cpu(), want.contiguous().flatten()), (Cout, Cin, K, dgrad)
    for n in (1, 1023, 16384 * 256 + 77):          # the last: beyond one round of the capped grid
        ref = torch.randn(n, generator=rng)
        ref[::7] = 0.0
        ref[3::11] = -0.0
        g = torch.randn(n, generator=rng)
        y = torch.full((n,), NAN, device="cuda")
        T._call("mural_op_relu_mask", g.cuda(), ref.cuda(), n, y, T._stream(y))
        assert torch.equal(y.cpu(), torch.where(ref > 0, g, torch.zeros_like(g))), n


# ------------------------------------------------------------------------------------------------------------------ dense -> symbols
@pytest.mark.parametrize("L", [1, 201, 2001])
def test_dense_to_symbols_matches_its_host_twin(L):
    """every one-hot and IUPAC-fraction column: the device op and mural_host_dense_to_symbols give the same symbols for the same
    tensor; a column that is no encoding sets the status word (the host twin marks it 255 and counts it)"""
    from tests import _util as U
    rng = np.random.default_rng(29)
    n = 23
    codes = rng.integers(0, 15, size=(n, L)).astype(np.uint8)
    codes[0, 0], codes[-1, -1] = 14, 11
    x = U.onehot(codes).contiguous()
    lib = _lib.lib()

    def host(t):
        out = np.full((n, L), 77, np.uint8)
        bad = C.c_int64(-1)
        _lib.check(lib.mural_host_dense_to_symbols((C.c_void_p * 1)(t.data_ptr()), (C.c_int64 * 1)(n), 1, L, out.ctypes.data, C.byref(bad)))
        return out, bad.value

    def device(t):
        td = t.cuda()
        sym = torch.full((n, L), 77, dtype=torch.uint8, device="cuda")
        status = torch.zeros(1, dtype=torch.int32, device="cuda")
        T._call("mural_op_dense_to_symbols", td, n, L, sym, status, T._stream(td))
        return sym.cpu().numpy(), int(status)

    want, bad = host(x)
    got, status = device(x)
    assert bad == 0 and status == 0 and np.array_equal(want, codes) and np.array_equal(got, want), L
    assert torch.equal(T.dense_to_symbols(x.cuda()).cpu(), torch.from_numpy(codes))
    T.flush_input_checks()
    r, j = n // 2, L // 2
    x[r, :, j] = torch.tensor([1.0, 1.0, 0.0, 0.0])
    want, bad = host(x)
    got, status = device(x)
    assert bad == 1 and want[r, j] == 255 and status != 0, L
    keep = np.ones((n, L), bool)
    keep[r, j] = False
    assert np.array_equal(got[keep], want[keep]) and np.array_equal(got[keep], codes[keep]), L
    T.dense_to_symbols(x.cuda())
    with pytest.raises(ValueError):
        T.flush_input_checks()
