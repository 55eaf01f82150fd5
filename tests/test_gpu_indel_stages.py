"""Float64 parity of every level of the fused INDEL forward (eval-mode UNet_Small: csrc/indel_level0.hip, conv1d.hip, convblock_mfma.hip,
convblock_deep.hip, the polyphase up-convs, sequenced by indel_forward_impl in csrc/indel_model.hip).  The end checks of
tests/test_gpu_indel.py (scores within 1e-4 * max(1, |want|max)) sit behind out_conv, a global maximum over all columns and the head;
tests/test_indel_stages_host.py shows a wrong enc0 element on a tile border that they cannot see.  Here the intermediates a forward call
leaves in the model's workspace are compared one by one with oracle/indel_ref.py in float64 on the windows of oracle/encode_ref.py (or on
the very dense tensor the call was given).

The regions are found by their position in the call's carve (S | E0..E5 | T1 | T2 | H | SP | M | X per lane, recorded for the first
chunk of each lane) and their byte sizes are asserted (tests/_indel_stages_data.py).  Tolerance: tests/_parity.py::_loose -- 8 x the
float32 oracle's own distance from float64 on the same inputs, at least 4 ulp of the largest magnitude; nothing is excluded.  The
workspace is filled with 0xFF bytes before every call (after a first call that sizes it), so a column no kernel wrote fails as NaN.

What a call leaves behind (read in indel_forward_impl and the kernels it launches; all regions [B][C][L] float32 from the region's start):
  enc0..enc5  E[0..5]: always -- the skips are never overwritten.
  sym         S: only when the input layer runs as a launch of its own (indel_model.hip: `if (sh.use_reverse && !gs.g && !gs.sym)`):
              use_reverse and either the dense entry with MURAL_INDEL_DENSE_SYMBOLS=0 or the packed entry with
              MURAL_DEBUG_INDEL_NO_GENOME_FRONT=1.  In every other form the persistent first-level kernel evaluates it per symbol
              (ConvBlockArgs::symtab / e0_t3) and S must still hold the poison -- asserted.
  dec2        level 2, prefix of T2; dec3: level 1, prefix of SP.  The decoder ping-pongs T2, SP, T2, SP, T2 (`dec = (cur == T2) ? SP : T2`);
              the last block carries the fused tail in every geometry here (level 0 has >= 128 columns: block_fusable) and then stores no
              `out` (indel_dec0_kernel: `if (a.tail_max == nullptr)` guards its only store of the block's output; convblock_kernel:
              `if constexpr (!TAIL)` / `if (!TAIL)` in conv1d.hip), so T2 keeps dec2 and SP keeps dec3.
  tail_max    M as [B][parts][C0]; parts = ceil(L0 / 248) in every form here: the persistent decoder (indel_level0.hip: D0_OUT) and
              the polyphase split form that MURAL_INDEL_DEC0=0 falls back to (convblock_tiles_of: CB_FRONT_OUT_POLY) tile alike, and M is
              sized for exactly that many, so no slot lies behind them (the reader asserts poison there for any smaller `parts`).  The
              split form stores every tile's own maximum; the persistent decoder carries the maximum across a workgroup's run of tiles
              and stores it at the run's last tile of the row, 0 in the run's other slots (`seg_end = nb != b || tix + 1 == last`).
              Every slot is checked against the float64 maxima of the tiles of its run (D.run_maxima): a slot is 0 or a run's maximum,
              never poison, and the last tile of a row always ends a run.
  gmax        the maximum of tail_max over parts.
  out         the call's result.
What cannot be read back: dec0 and dec1 are overwritten by the ping-pong (dec2 is a continuous function of them); dec4 is never stored
(tail_max, gmax and out are its witnesses); T1 holds the level-1 strided conv that the level-0 launch emits (ConvBlockArgs::d_out) only
until level 2 reuses it -- every enc1 column depends on it; H and X are scratch.
The switches of test_launch_forms_behind_switches change which kernel writes a region, not which regions survive: MURAL_INDEL_ENC0_DOWN=0
(252-column encoder tiles, the strided conv a launch of its own into T1), MURAL_INDEL_ENC0=0 + MURAL_INDEL_DEC0=0 (convblock_kernel<8> with
the genome source and with the polyphase front + tail: every slot of M a tile's own maximum), MURAL_INDEL_DEEP=0 (levels 3..5 and their
decoder blocks as two convs through H), MURAL_INDEL_DEEP_FRONT=0 (level 3's strided conv through T1).

Measured on an MI355X (256 CUs): every level, tail_max and gmax within 0.08 .. 0.34 of their bounds in every case.  `out` of the
human-insertion checkpoint is at 0.66 of its bound (9.6e-5 from float64, float32 oracle 1.8e-5) in every launch form alike: the
head's BatchNorm folded into the Linear in float32 (mural_indel_model_create: fc_w, fc_b) gives 7.6e-5 on the exact gmax already."""
import functools

import numpy as np
import pytest
import torch

from tests import _indel_stages_data as D
from tests._parity import _Stats

pytestmark = pytest.mark.gpu

SEED = 60
INSERTION, DELETION = "indel_pretrained_human_insertion.npz", "indel_pretrained_human_deletion_start.npz"
SMALL = "indel_synth_small.npz"
BASE = D.ENC + ("dec2", "dec3", "tail_max", "out")
CHUNK_DEFAULT = 4096      # csrc/indel_model.hip: INDEL_CHUNK_DEFAULT


@functools.lru_cache(maxsize=None)
def _model(name, use_reverse=None):
    _, _, sd, geo = D.model_pair(name, use_reverse)
    return D.product_model(geo, sd)


@functools.lru_cache(maxsize=None)
def _genome(name, n, seed, use_reverse=None):
    from mural_amd.data import PackedGenome
    return PackedGenome.from_sequence(D.cached_case(name, n, seed, use_reverse=use_reverse)["seq"], "cuda")


def _call(model, case, genome, sel, entry):
    pos, strand = case["pos"][sel], case["strand"][sel]
    with torch.no_grad():
        if entry == "dense":
            return model(torch.from_numpy(case["x"][sel]).cuda())
        return model.forward_packed(genome, torch.from_numpy(pos).cuda(), torch.from_numpy(strand).cuda(), case["R"])


def _forward(model, case, genome, sel, entry, chunk=CHUNK_DEFAULT, regions=True):
    """one forward call of the sites `sel` through `entry` on a workspace full of 0xFF -> (out, one dict of views per lane), on the device"""
    from mural_amd import _lib
    geo = case["geo"]
    n = len(case["pos"][sel])
    need = int(_lib.lib().mural_indel_workspace_bytes(model._get_handle(geo.L), n))
    if model._ws is None or model._ws.numel() < need:
        _call(model, case, genome, sel, entry)      # (sizes the workspace: the next call must not allocate a fresh one)
    model._ws.fill_(255)
    ws_ptr = model._ws.data_ptr()
    out = _call(model, case, genome, sel, entry)
    torch.cuda.synchronize()
    assert model._ws.data_ptr() == ws_ptr and bool(torch.isfinite(out).all())
    if not regions:
        return out.cpu(), None
    lanes = max(1, min(2, -(-n // chunk)))
    B_per_lane = [min(chunk, n - lane * chunk) for lane in range(lanes)]
    return out.cpu(), D.forward_regions(model._ws, D.last_layout(), lanes, B_per_lane, geo, geo.tail_parts())


def _check(case, sel, out, views, what, where, stats, own_input_layer=False):
    """the quantities of one lane of a call against the case's references, sliced to the lane's sites"""
    geo = case["geo"]
    want64 = {k: v[sel] for k, v in case["want64"].items()}
    ref32 = {k: v[sel] for k, v in case["ref32"].items()}
    if own_input_layer and geo.use_reverse:
        what = ("sym",) + tuple(what)
    else:
        assert bool((views["sym"].view(torch.uint8) == 255).all()), f"{where}: region S was written, though no launch of this form owns it"
    host = {k: views[k].cpu() for k in what if k != "out"}
    D.check_call(host, out, want64, ref32, what, where, stats, geo)
    return host


# ------------------------------------------------------------------------------------------------ 1: shipped routing
N_SHIPPED = 40
FORMS = {"packed": ("packed", {}, False), "dense": ("dense", {}, False),
         "dense, own input layer": ("dense", {"MURAL_INDEL_DENSE_SYMBOLS": "0"}, True),
         "packed, one-hot window": ("packed", {"MURAL_DEBUG_INDEL_NO_GENOME_FRONT": "1"}, True)}


@pytest.mark.parametrize("form", list(FORMS))
@pytest.mark.parametrize("name", [INSERTION, DELETION])
def test_shipped_routing(name, form, monkeypatch):
    """The shipped human-insertion (use_reverse) and deletion-start (no input layer) checkpoints at L = 8000: 40 sites on both strands of
    a 50 kb sequence over ACGTNRYMSWKBDHV (N and IUPAC codes at the 1 % level), positions 0, 3, R - 1, n - 1, n - R on either strand, six
    windows with N runs and single IUPAC codes on window columns 245..255, 493..505 and the last 8 (the borders of the 248- and the
    252-column tiles; tests/test_indel_stages_host.py checks the windows).  Every readable quantity through the packed entry, the dense
    entry, and both with the input layer and the first level as launches of their own -- which also leave `sym`."""
    entry, env, own = FORMS[form]
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    case, model, genome = D.cached_case(name, N_SHIPPED, SEED + 1), _model(name), _genome(name, N_SHIPPED, SEED + 1)
    stats = _Stats("shipped", tag="indel_stages")
    sel = slice(0, N_SHIPPED)
    out, lanes = _forward(model, case, genome, sel, entry)
    try:
        _check(case, sel, out, lanes[0], BASE, f"{name[6:-4]} {form} n={N_SHIPPED}", stats, own_input_layer=own)
    finally:
        stats.show()


# ------------------------------------------------------------------------------------------------ 2: columns that are no symbol
@pytest.mark.parametrize("name", [INSERTION, DELETION])
def test_dense_columns_that_are_no_symbol(name):
    """Case 1's windows with random-float, scaled one-hot and all-zero columns at columns 0, L - 1, 247..253 and in a run of 40, and one
    window without a single symbol (D.odd_columns): the dense entry classifies the other columns into symbol bytes and evaluates these
    from their floats inside the persistent first-level launch; the float64 oracle is fed the same tensor."""
    case, model = D.cached_case(name, N_SHIPPED, SEED + 1, odd=True), _model(name)
    stats = _Stats("no symbol", tag="indel_stages")
    sel = slice(0, N_SHIPPED)
    out, lanes = _forward(model, case, None, sel, "dense")
    try:
        _check(case, sel, out, lanes[0], BASE, f"{name[6:-4]} dense, odd columns n={N_SHIPPED}", stats)
    finally:
        stats.show()


# ------------------------------------------------------------------------------------------------ 3: persistent segments
ENC0_WG_PER_CU = 7      # launch_indel_enc0: wg_per_cu capped at 7; the decoder launch takes what the occupancy query answers (<= 7 here: LDS)


def _persistent_n(geo):
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    tiles = geo.tail_parts()
    n = -(-3 * ENC0_WG_PER_CU * cus // tiles) + 3
    assert tiles * n >= 3 * ENC0_WG_PER_CU * cus and n <= CHUNK_DEFAULT, (n, cus)
    return n, cus


@pytest.mark.parametrize("entry", ["packed", "dense"])
@pytest.mark.parametrize("use_reverse", [True, False])
def test_persistent_segments(use_reverse, entry):
    """L = 1000 (the geometry of indel_synth_small.npz, synthetic weights, with and without the input layer): both level-0 launches size
    their grid by occupancy x CUs and hand each workgroup a contiguous run of (row, tile) pairs.  With at least 3 x 7 x CUs row tiles
    in one chunk (5 tiles per row: n = ceil(21 CUs / 5) + 3, 1079 sites on 256 CUs) every workgroup walks a run of three or more tiles
    that crosses rows: the prefetch of the next row's first tile, the running maximum and its `nb != b` bookkeeping.  All quantities;
    M slot by slot: runs that end inside a row exist, and so do slots inside a run (exactly 0)."""
    geo = D.model_pair(SMALL, use_reverse)[3]
    n, cus = _persistent_n(geo)
    print(f"[indel_stages] persistent segments: n = {n} sites from {cus} CUs, {geo.tail_parts()} tiles per row")
    case, model, genome = D.cached_case(SMALL, n, SEED + 2, use_reverse=use_reverse), _model(SMALL, use_reverse), \
        _genome(SMALL, n, SEED + 2, use_reverse)
    stats = _Stats("persistent", tag="indel_stages")
    sel = slice(0, n)
    out, lanes = _forward(model, case, genome, sel, entry)
    try:
        host = _check(case, sel, out, lanes[0], BASE, f"L=1000 rev={int(use_reverse)} {entry} n={n}", stats)
        ends = (host["tail_max"].numpy() != 0).any(axis=2)
        assert ends[:, :-1].any() and (~ends).any(), "no workgroup's run of tiles ends inside a row / no slot lies inside a run"
    finally:
        stats.show()


# ------------------------------------------------------------------------------------------------ 4: other row lengths
@pytest.mark.parametrize("name", ["indel_synth_c2.npz", "indel_synth_c2_rev.npz", SMALL])
def test_other_row_lengths_of_the_deep_kernels(name):
    """n_class 2 at L = 4000 (levels 4000 / 1000 / 200 / 40 / 8 / 4: other block counts of convblock_deep.hip, rows the tiny kernels
    do not serve) and L = 1000 (1000 / 250 / 50 / 10 / 2 / 1: the 50-column level is below the 128 columns of block_fusable, the
    deepest rows are 2 and 1 columns): 24 edge sites through the packed entry."""
    n = 24
    case, model, genome = D.cached_case(name, n, SEED + 3), _model(name), _genome(name, n, SEED + 3)
    geo = case["geo"]
    assert geo.len in ([4000, 1000, 200, 40, 8, 4], [1000, 250, 50, 10, 2, 1])
    stats = _Stats("row lengths", tag="indel_stages")
    sel = slice(0, n)
    out, lanes = _forward(model, case, genome, sel, "packed")
    try:
        _check(case, sel, out, lanes[0], BASE, f"{name[6:-4]} L={geo.L} packed n={n}", stats)
    finally:
        stats.show()


# ------------------------------------------------------------------------------------------------ 5: two lanes
def test_two_lanes(monkeypatch):
    """MURAL_INDEL_CHUNK=256 at L = 1000: 300 sites are two chunks on two streams with a workspace half each -- lane 0 holds 256 sites,
    lane 1 holds 44, every quantity of both.  556 sites: a third chunk reuses lane 0 with a carve of 44 sites at other offsets, so only
    `out` of all 556 is checked there."""
    monkeypatch.setenv("MURAL_INDEL_CHUNK", "256")
    n_all = 556
    case, model, genome = D.cached_case(SMALL, n_all, SEED + 4), _model(SMALL), _genome(SMALL, n_all, SEED + 4)
    stats = _Stats("two lanes", tag="indel_stages")
    try:
        _forward(model, case, genome, slice(0, n_all), "packed", chunk=256, regions=False)      # (sizes the workspace for both calls)
        out, lanes = _forward(model, case, genome, slice(0, 300), "packed", chunk=256)
        assert len(lanes) == 2
        _check(case, slice(0, 256), out[:256], lanes[0], BASE, "L=1000 packed n=300 lane 0", stats)
        _check(case, slice(256, 300), out[256:], lanes[1], BASE, "L=1000 packed n=300 lane 1", stats)
        out, _ = _forward(model, case, genome, slice(0, n_all), "packed", chunk=256, regions=False)
        D.check_tap(out, case["want64"]["out"], case["ref32"]["out"], "out", f"L=1000 packed n={n_all}", stats, case["geo"])
    finally:
        stats.show()


# ------------------------------------------------------------------------------------------------ 6: launch forms behind switches
SWITCHES = [{"MURAL_INDEL_ENC0_DOWN": "0"}, {"MURAL_INDEL_ENC0": "0", "MURAL_INDEL_DEC0": "0"}, {"MURAL_INDEL_DEEP": "0"},
            {"MURAL_INDEL_DEEP_FRONT": "0"}]


@pytest.mark.parametrize("env", SWITCHES, ids=lambda e: "+".join(f"{k[12:]}={v}" for k, v in e.items()))
def test_launch_forms_behind_switches(env, monkeypatch):
    """Case 1's packed inputs on the human-insertion checkpoint under each launch form that test_level0_kernels_and_wide_stores_...
    only compares with the default form: each against float64.  The same regions survive in every form (the module's docstring); with
    the persistent decoder off every slot of M holds its own tile's maximum."""
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    case, model, genome = D.cached_case(INSERTION, N_SHIPPED, SEED + 1), _model(INSERTION), _genome(INSERTION, N_SHIPPED, SEED + 1)
    stats = _Stats("switches", tag="indel_stages")
    sel = slice(0, N_SHIPPED)
    out, lanes = _forward(model, case, genome, sel, "packed")
    try:
        host = _check(case, sel, out, lanes[0], BASE, " ".join(f"{k}={v}" for k, v in env.items()), stats)
        if "MURAL_INDEL_DEC0" in env:
            assert bool((host["tail_max"] > 0).all()), "the split form stores a maximum for every tile"
    finally:
        stats.show()
