"""Float64 parity of every stage of the fused SNV forward (csrc/snv_stage1.hip, snv_tower.hip, snv_tower_wave.hip, the long-window
segment / scatter launches of snv_model.hip, the edge pyramid of snv_reuse.hip).  The end check (tests/test_gpu_snv.py: probabilities
within 1e-5) sits behind a global max, a softmax and a division by four; here the intermediates a forward call leaves in the model's
workspace are compared one by one with oracle/snv_ref.py in float64 on the windows of oracle/encode_ref.py:

  x0 (stage-1 output)  |  s3[0], s3[1] (input of the second conv stage of the large / mid tower)  |  xlogit (the large tower's logits)
  |  local_logits  |  out

The regions are found by their position in the call's carve and their byte sizes are asserted (tests/_snv_stages_data.py).  Tolerance:
tests/_parity.py::_loose -- 8 x the float32 oracle's own distance from float64 on the same inputs, at least 4 ulp of the largest
magnitude; nothing is excluded (every stage is continuous).  The workspace is filled with NaN bytes before every call, so a column no
kernel wrote fails as well.

Which launch writes what (read in the kernels): stage 1 writes x0; the first-stage tower launches pool and BatchNorm into s3[tower]; the
LARGE tower's short-stage launch stores its logits into xlogit (snv_tower_wave_body.inc / snv_tower.hip: `if (!do_head)`), the mid
tower's reads them and runs the head.  All of them still hold these values when the call returns.  What cannot be read back:
  * the mid tower's logits never leave LDS (every launch shape) -- `out` is their only witness;
  * small-batch launches (calls of <= 256 sites): s3[0] carries the mid tower's logits between the two workgroups of a site and
    s3[1] the arrival counters, the pooled rows stay in LDS -- x0, local_logits and out are checked there;
  * front-only models (R = 16000): the large tower's pooled row goes to the caller's s3_out (checked), its remaining layers run
    per layer outside the fused kernels; xlogit then holds what the caller handed to mural_snv_forward_finish.

Sites per unit the tail and wrap cases are built from (plan_wave_geometry admits a first-stage geometry with nine 16-column blocks per wave
only; tests/test_snv_stages_host.py pins the arithmetic): R = 100: 9 (large) and 2 (mid) sites per wave in the first-stage launches, short
stages on workgroup tiles of up to 32 (large) / 10 (mid) sites, one site per tile in calls of <= 512 sites (run_towers); R = 1000: 1 and 2
sites per wave in the first-stage launches, 6 and 5 in the short-stage launches.  Every launch strides its units by 2048 (512 workgroups
of four waves, or 2048 workgroup tiles)."""
import functools

import numpy as np
import pytest
import torch

from tests import _snv_stages_data as D
from tests._parity import _Stats

pytestmark = pytest.mark.gpu

SEED = 40


def _case(model_no, R, n=700):
    r = 5 if R == 100 else 7
    length = 20_000 if R <= 1000 else (40_000 if R <= 4000 else 90_000)
    return D.cached_case(model_no, r, R, n, SEED + R + model_no, length)


@functools.lru_cache(maxsize=None)
def _model(model_no, R, n=700):
    case = _case(model_no, R, n)
    return D.product_model(model_no, case["r"], R, case["sd"])


@functools.lru_cache(maxsize=None)
def _genome(model_no, R, n=700):
    from mural_amd.data import PackedGenome
    return PackedGenome.from_sequence(_case(model_no, R, n)["seq"], "cuda")


def _poison(model):
    if model._ws is not None:
        model._ws.fill_(255)


def _forward(model, case, genome, sel, entry):
    """one forward call of the sites `sel` through `entry` on a NaN-filled workspace -> (out, workspace regions), CPU tensors"""
    pos, strand, r, R, model_no = case["pos"][sel], case["strand"][sel], case["r"], case["R"], case["model_no"]
    n = len(pos)
    sym = D.strand_symbols(strand)
    cat = torch.from_numpy(D.encode_ref.kmer_encode(case["codes"], pos, sym, r, 3)).cuda()
    cont = torch.zeros(n, 1, dtype=torch.float64, device="cuda")
    _poison(model)
    with torch.no_grad():
        if entry == "dense":
            x = torch.from_numpy(D.encode_ref.onehot_encode(case["codes"], pos, sym, R)).cuda()
            out = model((cont, cat), x)
        elif entry == "symbols":
            out = model.forward_symbols(cat, torch.from_numpy(D.symbol_windows(case["codes"], pos, strand, R)).cuda())
        else:
            out = model.forward_packed(genome, torch.from_numpy(pos).cuda(), torch.from_numpy(strand).cuda(), local_radius=r, local_order=3)
    torch.cuda.synchronize()
    reg = D.forward_regions(model._ws, D.last_layout(), n, model_no, 2 * r - 1, R, dense=entry == "dense")
    return out.cpu(), {k: v.cpu() for k, v in reg.items()}


def _check(case, sel, out, reg, what, where, stats, other=None):
    """the named quantities of a call against the case's references, sliced to the call's sites"""
    R = case["R"]
    for q in what:
        got = out if q == "out" else reg[q]
        D.check_stage(got, case["want64"][q][sel], case["ref32"][q][sel], q, where, stats, other=None if other is None else other[q],
                      column_label=(lambda j: D.segment_of(R, j)) if q == "s3_0" else None)


ALL = ("x0", "s3_0", "s3_1", "xlogit", "local_logits", "out")


def _quantities(model_no, names=ALL):
    return tuple(q for q in names if q != "local_logits" or model_no == 2)


# ------------------------------------------------------------------------------------------------ 1: throughput launches
@pytest.mark.parametrize("entry", ["dense", "symbols", "packed"])
@pytest.mark.parametrize("R", [100, 200, 1000])
@pytest.mark.parametrize("model_no", [2, 1])
def test_throughput_launches(model_no, R, entry, monkeypatch):
    """700 sites on both strands of a 20 kb sequence with N / R / Y at the 1 % level, positions 0, 3, len - 1 and len - R among them,
    through the stage-split launches: every quantity of every site, for the dense, the symbols and the packed entry."""
    monkeypatch.setenv("MURAL_DEBUG_NO_SMALL_BATCH", "1")
    case, model = _case(model_no, R), _model(model_no, R)
    stats = _Stats("throughput", tag="snv_stages")
    sel = slice(0, 700)
    out, reg = _forward(model, case, _genome(model_no, R), sel, entry)
    try:
        _check(case, sel, out, reg, _quantities(model_no), f"net{model_no} R={R} {entry} n=700", stats)
    finally:
        stats.show()


# ------------------------------------------------------------------------------------------------ 2: unit tails
TAIL_N = list(range(1, 41)) + [255, 256, 257]
TAIL_WHAT = ("s3_0", "s3_1", "xlogit", "out")
# (R, n, quantity) of the sweep that miss the rule applied call by call, with the measured figures: checked in a test of their own
# (strict xfail), every other quantity of the same call in test_unit_tails
TAIL_BEYOND = {
    (100, 1, "s3_0"): "kernel 8.376e-06 from float64, allowed 8.056e-06 (float32 oracle 1.007e-06, one ulp of the 11.97 at the worst element "
                      "s3_0[0, 1, 20]; 64 elements compared); the same element within the rule in every call of n >= 2",
}


def _tail_call(R, n, what, monkeypatch):
    monkeypatch.setenv("MURAL_DEBUG_NO_SMALL_BATCH", "1")
    case, model, genome = _case(2, R), _model(2, R), _genome(2, R)
    if model._ws is None:      # (sized once for the largest call, so that every call runs on a workspace poisoned beforehand)
        _forward(model, case, genome, slice(0, max(TAIL_N)), "packed")
    stats = _Stats("unit tails", tag="snv_stages")
    sel = slice(0, n)
    out, reg = _forward(model, case, genome, sel, "packed")
    try:
        _check(case, sel, out, reg, what, f"R={R} n={n}", stats)
    finally:
        stats.show()


@pytest.mark.parametrize("n", TAIL_N)
@pytest.mark.parametrize("R", [100, 1000])
def test_unit_tails(R, n, monkeypatch):
    """Every n from 1 to 40 and 255, 256, 257 through the throughput launches (packed entry): more than twice the largest number of
    sites per unit of any launch of these calls (9 at R = 100, where the short-stage tiles hold one site in calls this small; 6 at
    R = 1000; the module's docstring), so that the last site of a partly filled unit and the block behind it are checked at every fill.
    s3, xlogit and out of all n sites of the call, the rule applied to that call's rows alone."""
    first, (short, kind) = D.wave_sites(R), D.short_stage_sites(R)
    assert 2 * max(first + (short if kind == "wave" else (1, 1))) + 1 <= 40
    _tail_call(R, n, tuple(q for q in TAIL_WHAT if (R, n, q) not in TAIL_BEYOND), monkeypatch)


@pytest.mark.parametrize("R,n,q", [pytest.param(*k, marks=pytest.mark.xfail(strict=True, reason=v)) for k, v in TAIL_BEYOND.items()])
def test_unit_tails_beyond_the_rule(R, n, q, monkeypatch):
    """The comparisons of the sweep that miss the rule as it stands.  Its yardstick is the float32 oracle's largest distance from
    float64 over the compared tensor; the call of one site at R = 100 compares 64 elements of s3[0], and that maximum then falls to one
    ulp while the kernel's error on the same elements is what it is in every larger call, where the same elements pass (per-site
    results do not depend on the batch).  The cause was not traced further in the kernel; the rule is not widened."""
    _tail_call(R, n, (q,), monkeypatch)


# ------------------------------------------------------------------------------------------------ 3: more units than waves
WRAP_N = 2048 * 10 + 10 * 13 + 7      # 20617 sites


@functools.lru_cache(maxsize=None)
def _wrap_case():
    base = _case(2, 100)
    pos, strand = D.edge_sites(len(base["seq"]), 100, WRAP_N, 77)
    # first 64, 64 around each wrap (site 2048 x sites per unit of a launch: 4096, 18432, 20480), last 64
    idx = np.unique(np.concatenate([np.arange(0, 64)] + [np.arange(w - 32, w + 32) for w in (2 * 2048, 9 * 2048, 10 * 2048)]
                                   + [np.arange(WRAP_N - 64, WRAP_N)]))
    want64, ref32 = D.reference(base["orc32"], base["orc64"], 2, base["codes"], pos[idx], strand[idx], base["r"], 100)
    return dict(base, pos=pos, strand=strand, idx=idx, want64=want64, ref32=ref32)


@pytest.mark.parametrize("dynamic", [False, True])
def test_more_units_than_waves(dynamic, monkeypatch):
    """R = 100, 20617 sites = 2048 x 10 + 13 x 10 + 7: the large tower's first-stage launch (9 sites per wave) walks 2291 units on 2048
    waves, the mid tower's (2 per wave) 10309, the mid tower's short-stage launch 2062 tiles of 10 sites on 2048 workgroups -- each a full
    round and a partial one with a partly filled last unit.  Float64 for the first 64 sites, 64 around each wrap and the last 64; once
    with the fixed stride and once with the ticket counter (MURAL_TOWER_DYNAMIC_UNITS=1: the mid first-stage launch has enough units
    to take it)."""
    assert D.wave_sites(100) == (9, 2) and WRAP_N > D.UNIT_STRIDE * 10 and WRAP_N % 9 and WRAP_N % 2 and WRAP_N % 10
    if dynamic:
        monkeypatch.setenv("MURAL_TOWER_DYNAMIC_UNITS", "1")
    else:
        monkeypatch.delenv("MURAL_TOWER_DYNAMIC_UNITS", raising=False)
    case, model, genome = _wrap_case(), _model(2, 100), _genome(2, 100)
    idx = torch.from_numpy(case["idx"]).cuda()
    _poison(model)
    with torch.no_grad():
        out = model.forward_packed(genome, torch.from_numpy(case["pos"]).cuda(), torch.from_numpy(case["strand"]).cuda(), local_radius=case["r"],
                                   local_order=3)
    torch.cuda.synchronize()
    assert bool(torch.isfinite(out).all())
    reg = D.forward_regions(model._ws, D.last_layout(), WRAP_N, 2, 2 * case["r"] - 1, 100, dense=False)
    stats = _Stats("unit wrap", tag="snv_stages")
    try:
        for q in ALL:
            got = (out if q == "out" else reg[q])[idx].cpu()
            D.check_stage(got, case["want64"][q], case["ref32"][q], q, f"R=100 n={WRAP_N} dynamic={int(dynamic)}", stats)
    finally:
        stats.show()


# ------------------------------------------------------------------------------------------------ 4: small-batch launches
@pytest.mark.parametrize("entry", ["dense", "packed"])
@pytest.mark.parametrize("n", [1, 16, 256])
def test_small_batch_launches(n, entry, monkeypatch):
    """Calls of up to 256 sites: one workgroup per (site, tower), the dense window and the local branch inside the first-stage launch.
    x0, local_logits and out (the module's docstring says why not the pooled rows)."""
    monkeypatch.delenv("MURAL_DEBUG_NO_SMALL_BATCH", raising=False)
    case, model = _case(2, 1000), _model(2, 1000)
    stats = _Stats("small batch", tag="snv_stages")
    sel = slice(0, n)
    out, reg = _forward(model, case, _genome(2, 1000), sel, entry)
    try:
        _check(case, sel, out, reg, ("x0", "local_logits", "out"), f"R=1000 {entry} n={n}", stats)
    finally:
        stats.show()


# ------------------------------------------------------------------------------------------------ 5: long windows
@pytest.mark.parametrize("entry", ["packed", "dense"])
@pytest.mark.parametrize("R", [2000, 3000])
def test_long_windows(R, entry):
    """R = 2000 / 3000: the large tower's pooled first-stage row (267 / 401 columns) runs its first conv stage on segments with halo
    columns; the scatter launches assemble s3[0] from the segments' pooled columns.  Every column of every site; a failure names the
    segment (lw_nj, lw_nA of the plan) the worst column came from."""
    case, model = _case(2, R, 24), _model(2, R, 24)
    assert model._fused_ok() and D.longwin_plan(R) is not None
    stats = _Stats("long windows", tag="snv_stages")
    sel = slice(0, 24)
    out, reg = _forward(model, case, _genome(2, R, 24), sel, entry)
    try:
        _check(case, sel, out, reg, ALL, f"R={R} {entry} n=24", stats)
    finally:
        stats.show()


def test_front_only_long_window():
    """R = 16000 (front-only handle with a fused mid tower): the s3_out of mural_snv_forward_front, and what that call leaves in the
    workspace for mural_snv_forward_finish -- x0, the mid tower's pooled row s3[1], the local branch's logits; then the whole packed
    forward: xlogit (the large tower's logits, here computed per layer from s3_out and handed to the finish call) and out.  The mid
    tower's logits stay in LDS."""
    import ctypes as C
    from mural_amd import _lib
    R, n = 16000, 6
    case, model, genome = _case(2, R, n), _model(2, R, n), _genome(2, R, n)
    assert model._front_ok() and model._front_mid
    dev = torch.device("cuda", torch.cuda.current_device())
    pos, strand = torch.from_numpy(case["pos"]).cuda(), torch.from_numpy(case["strand"]).cuda()
    L3 = D.tower_lengths(R)[0][1]
    assert model._front_L3 == L3
    stats = _Stats("front only", tag="snv_stages")
    sel = slice(0, n)
    try:
        with torch.cuda.device(dev):
            ws = model._workspace(n, dev, dense=False)
            _poison(model)
            s3_out = torch.full((n, L3, 32), float("nan"), dtype=torch.float32, device=dev)
            g = genome.as_struct(dev)
            _lib.check(_lib.lib().mural_snv_forward_front(model._get_handle(), C.byref(g), pos.data_ptr(), strand.data_ptr(), n, case["r"], 3,
                                                         s3_out.data_ptr(), ws.data_ptr(), ws.numel(), _lib.current_stream_ptr(dev)))
            torch.cuda.synchronize()
        reg = D.forward_regions(model._ws, D.last_layout(), n, 2, 2 * case["r"] - 1, R, dense=False)
        reg = {k: v.cpu() for k, v in reg.items()}
        reg["s3_0"] = s3_out.cpu()
        _check(case, sel, None, reg, ("x0", "s3_0", "s3_1", "local_logits"), f"R={R} front n={n}", stats)
        _poison(model)
        with torch.no_grad():
            out = model.forward_packed(genome, pos, strand, local_radius=case["r"], local_order=3)
        torch.cuda.synchronize()
        reg = D.forward_regions(model._ws, D.last_layout(), n, 2, 2 * case["r"] - 1, R, dense=False)
        _check(case, sel, out.cpu(), {k: v.cpu() for k, v in reg.items()}, ("s3_1", "xlogit", "local_logits", "out"), f"R={R} packed n={n}", stats)
    finally:
        stats.show()


# ------------------------------------------------------------------------------------------------ 6: reuse path
@pytest.mark.parametrize("cfg", [(7, 300), (10, 1000)])
def test_reuse_path(cfg):
    """Cross-position reuse: the pooled rows s3[0] / s3[1] come from per-base rows shared by all sites plus the edge pyramid's
    window-specific columns (the zero-padded last column -- right_pad -- at R = 1000).  700 sites in dense runs on both strands, both
    chromosome ends included: the regions of the reuse carve against float64, and against the per-window path's regions under the
    same rule."""
    from mural_amd import _lib
    from mural_amd.data import PackedGenome
    r, R = cfg
    case = D.reuse_case(r, R, SEED + 300 + R)
    model = D.product_model(2, r, R, case["sd"])
    genome = PackedGenome.from_sequence(case["seq"], "cuda")
    n = len(case["pos"])
    sel = slice(0, n)
    what = ("s3_0", "s3_1", "xlogit", "local_logits", "out")
    stats = _Stats("reuse", tag="snv_stages")
    try:
        out_w, reg_w = _forward(model, case, genome, sel, "packed")
        reg_w["out"] = out_w
        _check(case, sel, out_w, reg_w, what, f"r={r} R={R} per-window n={n}", stats)
        assert _lib.lib().mural_snv_reuse_supported(model._get_handle())
        tp, ts = torch.from_numpy(case["pos"]).cuda(), torch.from_numpy(case["strand"]).cuda()
        _poison(model)
        with torch.no_grad():
            out, used = model.forward_packed_reuse(genome, tp, ts, local_radius=r, local_order=3, return_reuse_count=True)
        torch.cuda.synchronize()
        assert used == n
        reg = {k: v.cpu() for k, v in D.reuse_regions(model._ws, D.last_layout(), n, 2, 2 * r - 1, R, strands=3).items()}
        _check(case, sel, out.cpu(), reg, what, f"r={r} R={R} reuse n={n}", stats)
        _check(case, sel, out.cpu(), reg, what, f"r={r} R={R} reuse vs per-window", stats, other=reg_w)
    finally:
        stats.show()
