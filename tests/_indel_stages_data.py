"""Inputs, float64 references and the region reader of the per-stage parity tests of the fused INDEL forward
(tests/test_gpu_indel_stages.py; the reader and the checker are tested without a device in tests/test_indel_stages_host.py).

An eval-mode UNet_Small call leaves its intermediates in the model's workspace; ``mural_debug_last_ws_layout`` lists the regions of the
call's carve (csrc/indel_model.hip: indel_forward_impl, the `take` lambda), recorded for the first chunk of each lane, in the order
S | E0..E5 | T1 | T2 | H | SP | M | X.  ``forward_regions`` identifies each region by that position, asserts its byte size (the
`per_pos * B * 4` of the carve) and returns plain [site][channel][column] views -- a carve that changes makes it fail instead of
misreading.  ``reference`` runs oracle/indel_ref.py twice on the windows of oracle/encode_ref.py (or on a given dense tensor): in float64
(the truth) and in float32 (the yardstick of tests/_parity.py::_loose: the kernel may be 8 times as far from float64 as the float32
oracle is, at least 4 ulp of the largest magnitude).

The checked quantities, all [site][channel][column] unless noted:
  sym         the strand-symmetrising input layer (use_reverse only), region S
  enc0..enc5  the encoder levels (the decoder's skips), regions E0..E5
  dec2, dec3  decoder outputs of level 2 / level 1 (skip added), prefixes of T2 / SP
  tail_max    [site][tile][channel]: Softplus(out_conv) maxima per tile (or per run of tiles) of the launch that took the tail, region M
  gmax        [site][channel]: the maximum of tail_max over the tiles
  out         the call's result
"""
import copy
import functools

import numpy as np
import torch

from oracle import encode_ref, indel_ref, synth
from tests import _util as U
from tests._snv_stages_data import _f32, check_stage, last_layout, strand_symbols      # noqa: F401  (re-exported to the tests)

N_LEVELS = indel_ref.N_LEVELS
TILE_DOWN = 248      # csrc/indel_level0.hip: E0_OUT_DOWN (level-0 encoder tile that also emits the stride-4 conv), D0_OUT = CB_FRONT_OUT_POLY
TILE = 252           # E0_OUT = CB_FRONT_OUT: every other level-0 launch with a front
REGIONS = ("S",) + tuple(f"E{i}" for i in range(N_LEVELS)) + ("T1", "T2", "H", "SP", "M", "X")      # 13 per lane
ENC = tuple(f"enc{i}" for i in range(N_LEVELS))
END_TOL = 1e-4       # the end check of tests/test_gpu_indel.py: 1e-4 * max(1, |want|max) on the scores


# ------------------------------------------------------------------------------------------------------------ geometry
class Geometry:
    """level lengths and channel counts as in mural_indel_model_create, and the carve's per-position sizes"""

    def __init__(self, L, channels=8, ksize=7, down=(1, 4, 5, 5, 5, 2), use_reverse=False, n_class=8):
        self.L, self.C0, self.K, self.down, self.use_reverse, self.n_class = int(L), int(channels), int(ksize), tuple(int(d) for d in down), \
            bool(use_reverse), int(n_class)
        pad = (self.K - 1) // 2
        self.ch = [self.C0 * (i + 1) for i in range(N_LEVELS)]
        self.len, cur = [], self.L
        for d in self.down:
            cur = (cur + 2 * pad - self.K) // d + 1
            self.len.append(cur)
        for i in range(N_LEVELS - 1, 0, -1):
            assert self.len[i] * self.down[i] == self.len[i - 1], f"length {L} is not compatible with down_list {self.down}"
        self.parts_max = -(-self.len[0] // TILE_DOWN)      # convblock_tiles(len[0], true): what M is sized for

    def per_pos(self):
        """floats per position of the 13 regions, in carve order"""
        sizes = [c * n for c, n in zip(self.ch, self.len)]
        tmax, hmax = max(sizes), 2 * max(sizes)
        return [4 * self.L] + sizes + [tmax, tmax, hmax, self.C0 * self.len[0], self.C0 * self.parts_max, 4 * self.L]

    def tail_parts(self, poly=True):
        """tiles per row of the launch that took the fused tail: ceil(L0 / 248) for the persistent decoder and the polyphase split form
        (upsampling by 4 with the 3-column polyphase taps: convblock_poly_mfma), ceil(L0 / 252) otherwise (convblock_tiles_of)"""
        poly = poly and self.down[1] == 4 and self.K == 7 and self.C0 == 8
        return -(-self.len[0] // (TILE_DOWN if poly else TILE))


def tile_of(geo, level, column):
    """where a column of a level comes from, for failure messages"""
    if level == 0:
        edge = " (window start)" if column < 8 else (" (window end)" if column >= geo.len[0] - 8 else "")
        return (f"level 0 column {column}: column {column % TILE_DOWN} of tile {column // TILE_DOWN} of the 248-column tiles, "
                f"column {column % TILE} of tile {column // TILE} of the 252-column tiles{edge}")
    if level == 1:
        per = TILE_DOWN // 4
        return f"level 1 column {column}: column {column % per} of the {per} that level-0 tile {column // per} emits with the strided conv"
    return f"level {level} column {column} of {geo.len[level]}"


def level_of(what):
    return {"sym": 0, "dec2": 2, "dec3": 1}.get(what, int(what[3]) if what.startswith("enc") else None)


# ------------------------------------------------------------------------------------------------------------ inputs
ALPHABET = b"ACGTNRYMSWKBDHV"
PLANT_COLUMNS = (tuple(range(245, 256)), tuple(range(493, 506)))      # the borders of the first tiles of both widths


def sequence(seed, length=50_000):
    """`length` bases over ACGTNRYMSWKBDHV with N and the IUPAC codes at the 1 % level, as a mutable uint8 array of ASCII"""
    rng = np.random.default_rng(seed)
    p = np.array([.2475] * 4 + [.005] + [.0005] * 10)
    return rng.choice(np.frombuffer(ALPHABET, np.uint8), size=length, p=p / p.sum()).copy()


def edge_sites(length, R, n, seed, planted=6):
    """n sites on both strands: positions 0, 3, R - 1, length - 1, length - R on either strand first, then `planted` sites in the
    middle whose windows `plant` writes N runs and IUPAC codes into, then random ones"""
    rng = np.random.default_rng(seed)
    pos = rng.integers(0, length, size=n)
    strand = rng.integers(0, 2, size=n).astype(np.uint8)
    edge = [0, 3, R - 1, length - 1, length - R]
    k = min(n, 10)
    pos[:k] = (edge + edge)[:k]
    strand[:k] = ([0] * 5 + [1] * 5)[:k]
    planted = max(0, min(planted, n - 10))
    pos[10:10 + planted] = length // 3 + 1777 * np.arange(planted)
    strand[10:10 + planted] = np.arange(planted) % 2
    return pos.astype(np.int64), strand, list(range(10, 10 + planted))


def plant(raw, pos, strand, R, sites):
    """N runs and single IUPAC codes on window columns 245..255, 493..505 and the last 8 columns of the windows of `sites` (the tile
    borders of both level-0 tile widths, and the window end)"""
    W = 2 * R
    for k, i in enumerate(sites):
        cols = {}
        for block in PLANT_COLUMNS + (tuple(range(W - 8, W)),):
            run = block[k % 3:k % 3 + 4]                                        # an N run of four ...
            cols.update({c: ord("N") for c in run})
            for j, c in enumerate(block):                                       # ... single codes on every second column beside it
                if c not in cols and (c + k) % 2 == 0:
                    cols[c] = ALPHABET[5 + (c + j + k) % 10]
        for c, ch in cols.items():
            g = int(pos[i]) - R + 1 + (W - 1 - c if strand[i] else c)
            if 0 <= g < len(raw):
                raw[g] = ch
    return raw


def model_pair(name, use_reverse=None):
    """(float32 oracle, float64 oracle, state dict, Geometry) of a golden fixture's geometry: its own weights (the shipped checkpoints),
    or synthetic ones from its seed (oracle/synth.py), then also with `use_reverse` other than the fixture's"""
    fx = U.load(name)
    hp = [int(v) for v in fx["hp"]]
    if use_reverse is not None:
        assert "seed" in fx.files, "only synthetic weights exist for both input layers"
        hp[4] = int(bool(use_reverse))
    orc = U.indel_oracle_from_hp(hp, fx["down"])
    sd = synth.synth_state_dict(orc.state_dict(), int(fx["seed"])) if "seed" in fx.files else U.indel_state_for(fx, orc)
    orc.load_state_dict(sd)
    orc.eval()
    geo = Geometry(2 * hp[0], hp[1], hp[2], fx["down"], hp[4], hp[3])
    return orc, copy.deepcopy(orc).double().eval(), sd, geo


def product_model(geo, sd):
    from mural_amd.model import model_choice
    cfg = dict(CNN_out_channels=geo.C0, CNN_kernel_size=geo.K, down_list=list(geo.down), use_reverse=geo.use_reverse)
    model = model_choice(0, cfg, dict(n_class=geo.n_class), "indel")
    model.load_state_dict(sd, strict=True)
    return model.cuda().eval()


def odd_columns(x, seed):
    """case 2: columns that are no symbol in a copy of the dense windows x [n][4][L] (n >= 14): random floats (window 10), scaled
    one-hot columns (11) and all-zero columns (12) at columns 0, L - 1, 247..253 and in a run of 40; window 13 without a single symbol"""
    rng = np.random.default_rng(seed)
    x = np.array(x, dtype=np.float32, copy=True)
    L = x.shape[2]
    cols = np.r_[0, L - 1, np.arange(247, 254), np.arange(L // 2, L // 2 + 40)]
    x[10][:, cols] = rng.standard_normal((4, len(cols)))
    x[11][:, cols] *= 0.7
    x[12][:, cols] = 0.0
    x[13] = rng.standard_normal((4, L))
    return x, cols


# ------------------------------------------------------------------------------------------------------------ reference
def _tile_maxima(feat, width):
    """[n][C][L] -> [n][tiles][C]: maxima over tiles of `width` columns"""
    n, C, L = feat.shape
    tiles = -(-L // width)
    pad = feat.new_full((n, C, tiles * width - L), float("-inf"))
    return torch.cat([feat, pad], dim=2).reshape(n, C, tiles, width).max(dim=3).values.permute(0, 2, 1).contiguous()


def _stages(orc, x, tile):
    taps = {}
    with torch.no_grad():
        out = orc(x, taps=taps)
        q = {k: taps[k] for k in ENC + ("dec2", "dec3", "gmax") + (("sym",) if orc.use_reverse else ())}
        q["tile_max"] = _tile_maxima(orc.out_conv(taps["dec4"]), tile)      # what gmax is the maximum of, tile by tile
        q["out"] = out
    return q


def reference(orc32, orc64, x, tile=TILE_DOWN, batch=64):
    """(float64 quantities, float32-oracle quantities) of the dense windows x [n][4][L] (float32), as dicts of CPU tensors; evaluated in
    batches of 64 sites, only the taps a call leaves behind are kept"""
    x = torch.as_tensor(x, dtype=torch.float32)
    parts64, parts32 = [], []
    for b0 in range(0, len(x), batch):
        parts64.append(_stages(orc64, x[b0:b0 + batch].double(), tile))
        parts32.append(_stages(orc32, x[b0:b0 + batch], tile))
    join = lambda parts: {k: torch.cat([q[k] for q in parts]) for k in parts[0]}      # noqa: E731
    return join(parts64), join(parts32)


@functools.lru_cache(maxsize=None)
def cached_case(name, n, seed, length=50_000, use_reverse=None, odd=False):
    """One configuration of the tests: oracles, weights, sequence, n edge sites and their references -- computed once per session and
    shared (nobody writes into it; per-site results do not depend on the batch, so a test of fewer sites slices it).  `odd`: the
    dense windows with the columns of `odd_columns` in place of the one-hot windows."""
    orc32, orc64, sd, geo = model_pair(name, use_reverse)
    R = geo.L // 2
    raw = sequence(seed + 1, length)
    pos, strand, planted = edge_sites(length, R, n, seed + 2)
    seq = plant(raw, pos, strand, R, planted).tobytes().decode()
    codes = encode_ref.seq_to_codes(seq)
    x = encode_ref.onehot_encode(codes, pos, strand_symbols(strand), R, "indel")
    cols = None
    if odd:
        x, cols = odd_columns(x, seed + 3)
    want64, ref32 = reference(orc32, orc64, x)
    return dict(name=name, geo=geo, R=R, sd=sd, seq=seq, codes=codes, pos=pos, strand=strand, planted=planted, x=x, odd_cols=cols,
                want64=want64, ref32=ref32, orc32=orc32, orc64=orc64)


def rest_of_network(orc, level, tensor, skips=()):
    """What follows encoder tap `enc{level}` in oracle/indel_ref.py::UNet_Small.forward, from `tensor` in its place (`skips`: the taps
    enc0 .. enc{level-1}, which the decoder adds) -> dict(out, gmax, feat: out_conv's output the global maximum is taken over)"""
    assert len(skips) == level
    with torch.no_grad():
        enc, h = list(skips) + [tensor], tensor
        for i in range(level + 1, N_LEVELS):
            h = orc.upblocks[i](orc.uplblocks[i](h))
            enc.append(h)
        for j in range(N_LEVELS - 1):
            h = enc[N_LEVELS - 2 - j] + orc.downblocks[j](orc.downlblocks[j](h))
        feat = orc.out_conv(h)
        gmax = feat.max(dim=2).values
        return dict(out=orc.out_fc(gmax), gmax=gmax, feat=feat)


# ------------------------------------------------------------------------------------------------------------ workspace regions
def forward_regions(ws, layout, lanes, B_per_lane, geo, parts, poison=0xFF):
    """Views of an eval-mode forward's workspace (`ws`: numpy or torch uint8, `layout` of that call) -> one dict per lane.  The carve
    hands out S | E0..E5 | T1 | T2 | H | SP | M | X per lane, each region per_pos * B * 4 bytes with B the lane's first chunk.  `parts`:
    tiles per row of the launch that took the tail; M is read as [B][parts][C0] and whatever lies behind that in the region must still
    hold the `poison` bytes the caller filled the workspace with."""
    assert len(B_per_lane) == lanes
    assert len(layout) == len(REGIONS) * lanes, f"the forward's carve has {len(layout)} regions, expected {len(REGIONS)} x {lanes} lanes"
    per_pos, out = geo.per_pos(), []
    for lane, B in enumerate(B_per_lane):
        reg = {}
        for k, (name, per) in enumerate(zip(REGIONS, per_pos)):
            off, have = layout[lane * len(REGIONS) + k]
            assert have == per * B * 4, f"lane {lane} region {name}: {have} bytes in the carve, expected {per * B * 4}"
            reg[name] = (off, have)
        assert 1 <= parts <= geo.parts_max
        used = B * parts * geo.C0 * 4
        off, have = reg["M"]
        behind = ws[off + used:off + have]
        assert bool((behind == poison).all()), f"lane {lane}: bytes of M behind its {B} x {parts} x {geo.C0} maxima were written"
        views = {f"enc{i}": _f32(ws, reg[f"E{i}"], (B, geo.ch[i], geo.len[i])) for i in range(N_LEVELS)}
        views["sym"] = _f32(ws, reg["S"], (B, 4, geo.L))
        views["dec2"] = _f32(ws, (reg["T2"][0], B * geo.ch[2] * geo.len[2] * 4), (B, geo.ch[2], geo.len[2]))
        views["dec3"] = _f32(ws, (reg["SP"][0], B * geo.ch[1] * geo.len[1] * 4), (B, geo.ch[1], geo.len[1]))
        views["tail_max"] = _f32(ws, (off, used), (B, parts, geo.C0))
        out.append(views)
    return out


def run_maxima(slots, tiles64, tiles32):
    """What the slots of M must hold.  The launch that took the tail writes one slot per (row, tile): the split form the tile's own
    maximum, the persistent decoder (indel_dec0_kernel) 0 for every tile but the last of a workgroup's run of tiles within the row
    (`seg_end = nb != b || tix + 1 == last`), where it stores the maximum carried across the run.  From the slots that are not 0 --
    the run ends -- and the oracle's per-tile maxima: (expected float64, expected float32-oracle) slot values.  The last tile of every
    row must be a run end."""
    slots = np.asarray(slots)
    ends = (slots != 0).any(axis=2)
    assert bool(ends[:, -1].all()), f"tail_max: the last tile of row {int(np.argmin(ends[:, -1]))} holds no maximum"
    want, ref = torch.zeros_like(tiles64), torch.zeros_like(tiles32)
    for b in range(slots.shape[0]):
        start = 0
        for t in np.nonzero(ends[b])[0]:
            want[b, t] = tiles64[b, start:t + 1].max(dim=0).values
            ref[b, t] = tiles32[b, start:t + 1].max(dim=0).values
            start = t + 1
    return want, ref


def check_call(views, out, want64, ref32, what, case, stats, geo):
    """the quantities `what` of one lane's views (forward_regions) and the call's `out` against the references of the same sites"""
    for q in what:
        if q == "out":
            check_tap(out, want64[q], ref32[q], q, case, stats, geo)
        elif q == "tail_max":
            slots = views[q]
            slots = slots.cpu().numpy() if isinstance(slots, torch.Tensor) else np.asarray(slots)
            assert np.isfinite(slots).all() and (slots >= 0).all(), f"tail_max at {case}: a slot holds no Softplus maximum"
            want, ref = run_maxima(slots, want64["tile_max"], ref32["tile_max"])
            check_tap(slots, want, ref, q, case, stats, geo)
            check_tap(slots.max(axis=1), want64["gmax"], ref32["gmax"], "gmax", case, stats, geo)
        else:
            check_tap(views[q], want64[q], ref32[q], q, case, stats, geo)


def check_tap(got, want64, ref32, what, case, stats, geo, other=None):
    """check_stage on one quantity.  [site][channel][column] tensors are compared channel-last, so that a failure names
    (site, column, channel) and the tile -- or window start / end -- the column belongs to."""
    level = level_of(what)
    if level is None:
        return check_stage(got, want64, ref32, what, case, stats, other=other)
    cl = lambda t: None if t is None else torch.as_tensor(np.ascontiguousarray(t) if isinstance(t, np.ndarray) else t).permute(0, 2, 1)      # noqa: E731
    return check_stage(cl(got), cl(want64), cl(ref32), what, case, stats, other=cl(other), column_label=lambda j: tile_of(geo, level, j))
