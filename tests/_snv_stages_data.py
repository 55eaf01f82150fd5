"""Inputs, float64 references and the region reader of the per-stage parity tests of the fused SNV forward
(tests/test_gpu_snv_stages.py; the checker itself is tested without a device in tests/test_snv_stages_host.py).

A forward call leaves its intermediates in the model's workspace; ``mural_debug_last_ws_layout`` lists the regions of the call's
carve (csrc/snv_model.hip: carve(); csrc/snv_reuse.hip: carve_reuse()) in the order the carver handed them out.  ``forward_regions``
/ ``reuse_regions`` identify each region by that position, assert its byte size and return plain channel-last views -- a carve that
changes makes them fail instead of misreading.  ``reference`` runs oracle/snv_ref.py twice on the windows of oracle/encode_ref.py: in
float64 (the truth) and in float32 (the yardstick of tests/_parity.py::_loose: the kernel may be 8 times as far from float64 as the
float32 oracle is, at least 4 ulp of the largest magnitude).

The checked quantities (``QUANTITIES``), all [site][...]:
  x0            stage-1 output, channel-last: the large tower's pooled first-layer columns, then the mid tower's (taps pool1_2, pool1)
  s3_0, s3_1    input of the second conv stage of the large / mid tower: eval BatchNorm of conv2{sfx}.0 on tap pool2{sfx}
  xlogit        the large tower's logits (tap fc_2): the large tower's short-stage launch hands them to the mid tower's, which runs the head
  mid_logits    tap fc: never leaves LDS in any launch shape (host test of the checker only)
  local_logits  the local branch (Network2)
  out           log-probabilities
"""
import copy
import ctypes as C
import functools

import numpy as np
import torch

from oracle import encode_ref, snv_ref, synth
from tests._parity import _loose

PROB_TOL = 1e-5                       # the end check of tests/test_gpu_snv.py
QUANTITIES = ("x0", "s3_0", "s3_1", "xlogit", "mid_logits", "local_logits", "out")
N_CLASS = 4
MAXCLASS = 16                         # csrc/snv.h: SNV_MAXCLASS, the row stride of xlogit
UNIT_STRIDE = 2048                    # units (waves / workgroup tiles) a tower launch strides by: 512 workgroups x 4 waves
                                      # (launch_snv_tower_wave), min(tiles, 2048) workgroups (launch_snv_towers)
# '-' strand symbol of each MURAL_SYM_* / encode_ref.IUPAC code: ACGTN RYMSWK BDHV -> TGCAN YRKSWM VHDB
_COMP = np.array([3, 2, 1, 0, 4, 6, 5, 10, 8, 9, 7, 14, 13, 12, 11], np.uint8)


# ------------------------------------------------------------------------------------------------------------ geometry
def pool_len(L, k, s, p):
    return (L + 2 * p - k) // s + 1


def tower_lengths(R):
    """((L2, L3, L4) of the large tower, the same of the mid tower): columns after each max-pool (csrc/snv_model.hip: fill_tower_lengths)"""
    out = []
    for L, pools in ((2 * R + 1, snv_ref.POOLS_LARGE), (2 * snv_ref.MID_HALF + 1, snv_ref.POOLS_MID)):
        Ls = []
        for k, s, p in pools:
            L = pool_len(L, k, s, p)
            Ls.append(L)
        out.append(tuple(Ls))
    return tuple(out)


def wave_sites(R):
    """Sites per wave of the two wave-private first-stage launches (large, mid): plan_wave_geometry admits a first-stage geometry only
    with exactly nine 16-column blocks per wave, (1 + Pw (L2 + 1) + 15) // 16 == 9, and create() takes the largest such Pw <= 31."""
    res = []
    for L2 in (tower_lengths(R)[0][0], tower_lengths(R)[1][0]):
        fit = [pw for pw in range(1, 32) if (1 + pw * (L2 + 1) + 15) // 16 == 9]
        res.append(max(fit) if fit else 0)
    return tuple(res)


def short_stage_sites(R):
    """Sites per unit of the two short-stage launches (large, mid) and their kind.  plan_wave_geometry admits the wave-private
    short-stage kernel for the shipped window only (Lwin == SHIP_LWIN = 2001) with 6 / 5 sites per wave.  Every other window keeps
    workgroup tiles (plan_part over plan_geometry in csrc/snv_model.hip): the most sites <= 32 whose stages stay within
    2 x SNV_NB2MAX = 18 sixteen-column blocks and whose LDS stays within 80 KB, then among that count and the two below it the first
    whose second-stage block count is a multiple of four.  (run_towers shrinks a tile to ceil(n / 512) sites in calls of fewer sites.)"""
    if 2 * R + 1 == 2001:
        return (6, 5), "wave"
    res = []
    for Ls in tower_lengths(R):
        def plan(P):      # -> (LDS bytes or 0, blocks of the second stage)
            nb = [(1 + P * (L + 1) + 15) // 16 for L in Ls[1:]]
            if any((b + 1) // 2 > 9 for b in nb):
                return 0, nb[0]
            nbuf = (16 * max(nb) + 2) * 32
            par = 2 * (2 * 4 * 32 + N_CLASS * 32 + MAXCLASS)
            return 2 * nbuf * 4 + (2 * P * 32 + 3 * P * MAXCLASS) * 4 + par * 4, nb[0]
        P = max(p for p in range(1, 33) if 0 < plan(p)[0] <= 80 * 1024)
        for cand in range(P, max(P - 3, 0), -1):
            if plan(cand)[0] and plan(cand)[1] % 4 == 0:
                P = cand
                break
        res.append(P)
    return tuple(res), "tile"


def longwin_plan(R):
    """The segment plan of a long window (csrc/snv_model.hip, mural_snv_model_create): lw_nj, lw_nA, lw_SB, pooled columns of an equal
    segment and of the last one; None where the large tower's pooled row fits a wave (no segments)."""
    L2 = tower_lengths(R)[0][0]
    nj, LA = 19, 7 * 19 + 8
    if L2 <= LA:
        return None
    nA = 0
    while 7 * nj * nA + LA <= L2:
        nA += 1
    SB = 7 * ((L2 - 142 + 6) // 7)
    LB = L2 - SB
    return dict(nj=nj, nA=nA, SB=SB, LpA=pool_len(LA, 7, 7, 3), LpB=pool_len(LB, 7, 7, 3))


def segment_of(R, j):
    """which segment launch produced pooled column j of s3[0] (lw_scatter_kernel)"""
    plan = longwin_plan(R)
    if plan is None:
        return "whole row"
    nj, nA = plan["nj"], plan["nA"]
    if j < nA * nj + 1:
        k = 0 if j <= nj else min((j - 1) // nj, nA - 1)
        return f"equal segment {k} of lw_nA={nA} (lw_nj={nj})"
    return f"last segment (start column {plan['SB']} of the pooled first-stage row, lw_nj={nj}, lw_nA={nA})"


# ------------------------------------------------------------------------------------------------------------ inputs
def sequence(seed, length=20_000):
    """~20 kb over ACGTNRY with N / IUPAC codes at the 1 % level"""
    rng = np.random.default_rng(seed)
    raw = rng.choice(np.frombuffer(b"ACGTNRY", np.uint8), size=length, p=[.2475, .2475, .2475, .2475, .005, .0025, .0025])
    seq = raw.tobytes().decode()
    return seq, encode_ref.seq_to_codes(seq)


def edge_sites(length, R, n, seed, long_windows=False):
    """n sites on both strands; the first eight are positions 0, 3, length - 1, length - R on either strand (conv zero padding, crop edge
    and off-chromosome N inside checked columns) -- for `long_windows` 0, 5, length - 1, length // 2, the sites of
    tests/test_gpu_snv.py::test_long_windows_match_oracle"""
    rng = np.random.default_rng(seed)
    pos = rng.integers(0, length, size=n)
    strand = rng.integers(0, 2, size=n).astype(np.uint8)
    edge = [0, 5, length - 1, length // 2] if long_windows else [0, 3, length - 1, length - R]
    k = min(n, 8)
    pos[:k] = (edge + edge)[:k]
    strand[:k] = ([0] * 4 + [1] * 4)[:k]
    return pos.astype(np.int64), strand


def strand_symbols(strand):
    return ["-" if s else "+" for s in strand]


def symbol_windows(codes, pos, strand, R):
    """uint8 (n, 2 R + 1) MURAL_SYM_* bytes of the windows, strand-oriented and complemented (what ``forward_symbols`` takes)"""
    win = encode_ref.gather_windows(codes, pos, R, "snv")
    neg = np.asarray(strand, dtype=bool)
    return np.ascontiguousarray(np.where(neg[:, None], _COMP[win][:, ::-1], win)).astype(np.uint8)


def model_pair(model_no, r, R, seed):
    """(float32 oracle, float64 oracle, state dict) with synthetic weights"""
    orc = snv_ref.build(model_no, local_radius=r, distal_radius=R, n_class=N_CLASS)
    sd = synth.synth_state_dict(orc.state_dict(), seed)
    orc.load_state_dict(sd)
    orc.eval()
    return orc, copy.deepcopy(orc).double().eval(), sd


def product_model(model_no, r, R, sd):
    from tests.test_gpu_snv import product_from_hp
    model, _ = product_from_hp(np.array([r, 3, R, 150, 75, 32, 3, N_CLASS, model_no]))
    model.load_state_dict(sd)
    return model.cuda().eval()


# ------------------------------------------------------------------------------------------------------------ reference
def _bn_eval(bn, v):
    """eval-mode BatchNorm1d of `bn` on v [n][C][L] in v's precision"""
    s = bn.weight / torch.sqrt(bn.running_var + bn.eps)
    t = bn.bias - bn.running_mean * s
    return v * s[None, :, None] + t[None, :, None]


def _stages(orc, model_no, cat, x):
    """QUANTITIES of one oracle (in its own precision) for windows x [n][4][W] and k-mer ids cat, channel-last like the workspace"""
    taps = {}
    with torch.no_grad():
        out = orc((torch.zeros(len(x), 1, dtype=x.dtype), cat), x, taps=taps)
        q = {"x0": torch.cat([taps["pool1_2"], taps["pool1"]], dim=2).permute(0, 2, 1).contiguous(),
             "s3_0": _bn_eval(orc.conv2_2[0], taps["pool2_2"]).permute(0, 2, 1).contiguous(),
             "s3_1": _bn_eval(orc.conv2[0], taps["pool2"]).permute(0, 2, 1).contiguous(),
             "xlogit": taps["fc_2"], "mid_logits": taps["fc"], "out": out}
        if model_no == 2:
            q["local_logits"] = taps["local_logits"]
    return q


def reference(orc32, orc64, model_no, codes, pos, strand, r, R, batch=64):
    """(float64 quantities, float32-oracle quantities) of the sites, both as dicts of CPU tensors; evaluated in batches (the first-layer
    taps of a batch of long windows are large)"""
    sym = strand_symbols(strand)
    parts64, parts32 = [], []
    for b0 in range(0, len(pos), batch):
        p, s = pos[b0:b0 + batch], sym[b0:b0 + batch]
        cat = torch.from_numpy(encode_ref.kmer_encode(codes, p, s, r, 3))
        x = torch.from_numpy(encode_ref.onehot_encode(codes, p, s, R))
        parts64.append(_stages(orc64, model_no, cat, x.double()))
        parts32.append(_stages(orc32, model_no, cat, x))
    join = lambda parts: {k: torch.cat([q[k] for q in parts]) for k in parts[0]}      # noqa: E731
    return join(parts64), join(parts32)


@functools.lru_cache(maxsize=None)
def cached_case(model_no, r, R, n, seed, length=20_000):
    """One configuration of the tests: oracles, weights, sequence, n edge sites and their references -- computed once per session and
    shared (nobody writes into it; per-site results do not depend on the batch, so a test of fewer sites slices it)"""
    orc32, orc64, sd = model_pair(model_no, r, R, seed)
    seq, codes = sequence(seed + 1, length)
    pos, strand = edge_sites(len(seq), R, n, seed + 2, long_windows=R > 1000)
    want64, ref32 = reference(orc32, orc64, model_no, codes, pos, strand, r, R)
    return dict(model_no=model_no, r=r, R=R, sd=sd, seq=seq, codes=codes, pos=pos, strand=strand, want64=want64, ref32=ref32,
                orc32=orc32, orc64=orc64)


@functools.lru_cache(maxsize=None)
def reuse_case(r, R, seed, runs=(200, 300, 200)):
    """The reuse path's configuration: Network2, a 12 kb sequence, dense runs of sites on both strands at the chromosome's start (`runs[0]`
    sites from position 0), in its middle and at its end (sites within R of both ends), in a shuffled order, with their references"""
    orc32, orc64, sd = model_pair(2, r, R, seed)
    seq, codes = sequence(seed + 1, 12_000)
    n = len(seq)
    pos = np.r_[np.arange(0, runs[0]), np.arange(5000, 5000 + runs[1]), np.arange(n - runs[2], n)].astype(np.int64)
    strand = (np.arange(len(pos)) % 2).astype(np.uint8)
    strand[runs[0] // 2:runs[0] + runs[1] // 5] = 1
    perm = np.random.default_rng(R).permutation(len(pos))
    pos, strand = pos[perm], strand[perm]
    want64, ref32 = reference(orc32, orc64, 2, codes, pos, strand, r, R)
    return dict(model_no=2, r=r, R=R, sd=sd, seq=seq, codes=codes, pos=pos, strand=strand, want64=want64, ref32=ref32, orc32=orc32,
                orc64=orc64)


def rest_of_tower(orc, sfx, s3, with_feature_row=False):
    """the tower's logits from its second-stage input s3 [n][L3][32] (channel-last, BatchNorm of conv2{sfx}.0 already applied): what
    follows the checked quantity in oracle/snv_ref.py::_run_tower; `with_feature_row`: (logits, the last conv's output [n][32][L4], the
    row the global max is taken over)"""
    g = lambda name: getattr(orc, name + sfx)      # noqa: E731
    with torch.no_grad():
        skip = h = g("conv2")[1](s3.permute(0, 2, 1))
        h = g("RBs2")(h)
        h = h + skip[:, :, : h.shape[2]]
        h = g("conv3")(g("maxpool3")(h))
        logits = (orc.distal_fc1 if sfx == "" else orc.distal_fc2)(h.max(dim=2).values)
        return (logits, h) if with_feature_row else logits


def head(model_no, large, mid, local=None):
    """per-class probabilities from the three logit sets (oracle/snv_ref.py: Network1 / Network2 forward)"""
    p = (torch.softmax(mid, dim=1) + torch.softmax(large, dim=1)) / 2
    if model_no == 2:
        p = (torch.softmax(local, dim=1) + p) / 2
    return p


# ------------------------------------------------------------------------------------------------------------ the check
def check_stage(got, want64, ref32, what, case, stats, other=None, column_label=None, row_label=None):
    """tests/_parity.py::_loose on one quantity, all sites at once; a failure also names the worst element (site, column, channel) and,
    with `column_label` / `row_label`, where that column / row comes from"""
    got = torch.as_tensor(np.ascontiguousarray(got) if isinstance(got, np.ndarray) else got)
    assert tuple(got.shape) == tuple(want64.shape), f"{what} at {case}: region read as {tuple(got.shape)}, reference is {tuple(want64.shape)}"
    assert bool(torch.isfinite(got).all()), f"{what} at {case}: non-finite values"
    try:
        _loose(got, want64, ref32, what, case, stats, other=None if other is None else torch.as_tensor(other))
    except AssertionError as e:
        target = want64 if other is None else torch.as_tensor(other).double()
        err = (got.double() - target).abs()
        idx = tuple(int(i) for i in np.unravel_index(int(err.argmax()), err.shape))
        where = f"; worst element {what}[{', '.join(str(i) for i in idx)}] = {float(got[idx]):.9g}, expected {float(target[idx]):.9g}"
        if column_label is not None and len(idx) == 3:
            where += f" ({column_label(idx[1])})"
        if row_label is not None:
            where += f" ({row_label(idx[0])})"
        raise AssertionError(str(e) + where) from None


# ------------------------------------------------------------------------------------------------------------ workspace regions
def last_layout(max_pairs=64):
    """(offset, bytes) of the regions of this thread's latest workspace carve"""
    from mural_amd import _lib
    buf = (C.c_size_t * (2 * max_pairs))()
    n = _lib.lib().mural_debug_last_ws_layout(buf, max_pairs)
    return [(int(buf[2 * i]), int(buf[2 * i + 1])) for i in range(n)]


def _f32(ws, region, shape):
    """float32 view of a region of `ws` (a numpy or torch uint8 array; regions start at 256-byte offsets)"""
    off, size = region
    return ws[off:off + size].view(torch.float32 if isinstance(ws, torch.Tensor) else np.float32).reshape(shape)


def forward_regions(ws, layout, n, model_no, ncol, R, dense):
    """Views of a per-window forward's workspace (numpy uint8 `ws`, `layout` of that call).  carve() hands out, in this order:
    local_logits, cat, symbols, x0, xlogit, s3[0], s3[1], counters and, for long windows, the segments' pooled outputs of both kinds;
    no region of a tower model is empty.  n is at most one chunk here, so every region holds n sites."""
    (L2l, L3l, _), (L2m, L3m, _) = tower_lengths(R)
    plan = longwin_plan(R)
    want = [("local_logits", n * N_CLASS * 4), ("cat", n * max(ncol if model_no == 2 else 0, 1) * 8),
            ("symbols", n * (2 * R + 1) if dense else 16), ("x0", n * (L2l + L2m) * 32 * 4), ("xlogit", n * MAXCLASS * 4),
            ("s3_0", n * L3l * 32 * 4), ("s3_1", n * L3m * 32 * 4), ("counters", 64)]
    if plan is not None:
        want += [("vs3A", n * plan["nA"] * plan["LpA"] * 32 * 4), ("vs3B", n * plan["LpB"] * 32 * 4)]
    assert len(layout) == len(want), f"the forward's carve has {len(layout)} regions, expected {len(want)}"
    reg = {}
    for (name, size), (off, have) in zip(want, layout):
        assert have == size, f"region {name}: {have} bytes in the carve, expected {size}"
        reg[name] = (off, have)
    return {"x0": _f32(ws, reg["x0"], (n, L2l + L2m, 32)), "s3_0": _f32(ws, reg["s3_0"], (n, L3l, 32)),
            "s3_1": _f32(ws, reg["s3_1"], (n, L3m, 32)), "xlogit": _f32(ws, reg["xlogit"], (n, MAXCLASS))[:, :N_CLASS],
            "local_logits": _f32(ws, reg["local_logits"], (n, N_CLASS))}


def reuse_regions(ws, layout, n, model_no, ncol, R, strands):
    """Views of the reuse entry's workspace: carve_reuse() hands out eleven per-base row arrays per strand in use, then cat, local_logits,
    xlogit, s3[0], s3[1], counters (n at most one super-chunk: every per-site region holds n sites)."""
    (_, L3l, _), (_, L3m, _) = tower_lengths(R)
    k = 11 * bin(strands & 3).count("1")
    want = [("cat", n * max(ncol if model_no == 2 else 0, 1) * 8), ("local_logits", n * N_CLASS * 4), ("xlogit", n * MAXCLASS * 4),
            ("s3_0", n * L3l * 32 * 4), ("s3_1", n * L3m * 32 * 4), ("counters", 64)]
    assert len(layout) == k + len(want), f"the reuse carve has {len(layout)} regions, expected {k} + {len(want)}"
    assert len({size for _, size in layout[:k]}) == 1, "the per-base row arrays of the reuse carve differ in size"
    reg = {}
    for (name, size), (off, have) in zip(want, layout[k:]):
        assert have == size, f"region {name}: {have} bytes in the reuse carve, expected {size}"
        reg[name] = (off, have)
    return {"s3_0": _f32(ws, reg["s3_0"], (n, L3l, 32)), "s3_1": _f32(ws, reg["s3_1"], (n, L3m, 32)),
            "xlogit": _f32(ws, reg["xlogit"], (n, MAXCLASS))[:, :N_CLASS], "local_logits": _f32(ws, reg["local_logits"], (n, N_CLASS))}
