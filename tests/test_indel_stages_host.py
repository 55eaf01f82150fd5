"""The region reader and the checker of the per-stage INDEL parity tests (tests/_indel_stages_data.py) without a device: a workspace
built from the float32 oracle's taps in the carve's own layout passes; one wrong element of enc0 on a tile border fails the stage check
by name -- and the same wrong element, carried through the rest of the network in float64, moves the scores by less than the end
check's 1e-4 * max(1, |want|max): what the end check cannot see, shown in the suite itself; a carve with other region counts or sizes is
refused."""
import numpy as np
import pytest
import torch

from oracle import encode_ref
from tests import _indel_stages_data as D
from tests._parity import _Stats

SEED = 60
WHAT = D.ENC + ("dec2", "dec3", "tail_max", "out")


def _small():
    return D.cached_case("indel_synth_small.npz", 24, SEED)


def _synthetic_workspace(case, lanes_B, chunk=32, poison=0xFF):
    """(workspace bytes, layout) of a call of sum(lanes_B) sites as indel_forward_impl carves it: per lane S | E0..E5 | T1 | T2 | H | SP |
    M | X at lane * chunk * (floats per position), every region B x its per-position size; the float32 oracle's taps where a call leaves
    them (the module's docstring), the row's maximum in the last slot of M and zeros in the others, poison everywhere else"""
    geo, ref = case["geo"], case["ref32"]
    per_pos = geo.per_pos()
    ws = np.full(len(lanes_B) * chunk * sum(per_pos) * 4 + 4096, poison, np.uint8)
    layout, first = [], 0
    for lane, B in enumerate(lanes_B):
        p = lane * chunk * sum(per_pos) * 4
        sel = slice(first, first + B)
        parts = geo.tail_parts()
        M = np.zeros((B, parts, geo.C0), np.float32)
        M[:, -1] = ref["gmax"][sel].numpy()
        fill = {"S": ref["sym"][sel].numpy(), "T2": ref["dec2"][sel].numpy(), "SP": ref["dec3"][sel].numpy(), "M": M}
        fill.update({f"E{i}": ref[f"enc{i}"][sel].numpy() for i in range(D.N_LEVELS)})
        for name, per in zip(D.REGIONS, per_pos):
            layout.append((p, per * B * 4))
            if name in fill:
                raw = np.ascontiguousarray(fill[name], np.float32).view(np.uint8).ravel()
                ws[p:p + len(raw)] = raw
            p += per * B * 4
        first += B
    return ws, layout


def test_float32_oracle_in_the_carves_layout_passes():
    case = _small()
    geo = case["geo"]
    assert geo.len == [1000, 250, 50, 10, 2, 1] and geo.ch == [8, 16, 24, 32, 40, 48] and geo.use_reverse
    lanes_B = (15, 9)
    ws, layout = _synthetic_workspace(case, lanes_B)
    assert len(layout) == 26
    lanes = D.forward_regions(ws, layout, 2, lanes_B, geo, geo.tail_parts())
    stats = _Stats("host", tag="indel_stages")
    first = 0
    for lane, B in enumerate(lanes_B):
        sel = slice(first, first + B)
        want64 = {k: v[sel] for k, v in case["want64"].items()}
        ref32 = {k: v[sel] for k, v in case["ref32"].items()}
        D.check_call(lanes[lane], ref32["out"], want64, ref32, ("sym",) + WHAT, f"lane {lane}", stats, geo)
        first += B
    stats.show()
    # a slot that no launch wrote is poison, and poison is NaN: it fails
    off, _ = layout[D.REGIONS.index("M")]
    ws[off:off + 4] = 0xFF
    lanes = D.forward_regions(ws, layout, 2, lanes_B, geo, geo.tail_parts())
    with pytest.raises(AssertionError, match="tail_max"):
        D.check_call(lanes[0], None, {k: v[:15] for k, v in case["want64"].items()}, {k: v[:15] for k, v in case["ref32"].items()},
                     ("tail_max",), "poisoned slot", stats, geo)


@pytest.mark.parametrize("name", ["indel_pretrained_human_insertion.npz", "indel_pretrained_human_deletion_start.npz"])
def test_float32_oracle_passes_the_stage_checks_on_the_shipped_windows(name):
    """the inputs of case 1 of the GPU module at a size a CPU affords: the float32 oracle against float64 under the rule, and the
    windows hold what the case is about"""
    n = 16
    case = D.cached_case(name, n, SEED + 1)
    geo, R = case["geo"], case["R"]
    assert geo.len == [8000, 2000, 400, 80, 16, 8] and geo.tail_parts() == 33 and geo.parts_max == 33
    stats = _Stats("host", tag="indel_stages")
    for q in case["want64"]:
        D.check_tap(case["ref32"][q], case["want64"][q], case["ref32"][q], q, name, stats, geo)
        # the bound is never degenerate: the float32 oracle is 1e-7 .. 1e-5 relative from float64
        rel = float((case["ref32"][q].double() - case["want64"][q]).abs().max() / case["want64"][q].abs().max())
        assert 1e-8 < rel < 1e-5, (q, rel)
    stats.show()
    assert case["want64"]["enc0"].dtype == torch.float64 and ("sym" in case["want64"]) == geo.use_reverse
    seq_len = len(case["seq"])
    assert list(case["pos"][:5]) == [0, 3, R - 1, seq_len - 1, seq_len - R] and list(case["strand"][:10]) == [0] * 5 + [1] * 5
    win = encode_ref.gather_windows(case["codes"], case["pos"], R, "indel")
    win = np.where(case["strand"][:, None] == 1, win[:, ::-1], win)      # columns as the strand-oriented window has them
    assert (win[0, :R - 1] == 4).all() and (win[3, R:] == 4).all()       # off-chromosome N at both ends
    for block in D.PLANT_COLUMNS + (tuple(range(2 * R - 8, 2 * R)),):
        sub = win[case["planted"]][:, list(block)]
        assert ((sub == 4).sum(axis=1) >= 3).all() and ((sub > 4).sum(axis=1) >= 2).all(), block
    assert set(case["strand"][case["planted"]]) == {0, 1} and len(case["planted"]) == 6


def test_columns_that_are_no_symbol():
    case = D.cached_case("indel_synth_small.npz", 24, SEED, odd=True)
    x, cols, L = case["x"], case["odd_cols"], case["geo"].L
    assert {0, L - 1, 247, 248, 251, 252, 253} <= set(cols) and len(cols) == 49
    symbol = lambda col: any(np.allclose(col, e, atol=1e-6) for e in encode_ref._OHE)      # noqa: E731
    assert not any(symbol(x[10][:, c]) for c in cols) and not any(symbol(x[11][:, c]) for c in cols)
    assert (x[12][:, cols] == 0).all() and not any(symbol(x[13][:, c]) for c in range(L))
    assert all(symbol(x[9][:, c]) for c in range(L))
    stats = _Stats("host", tag="indel_stages")
    for q in case["want64"]:
        D.check_tap(case["ref32"][q], case["want64"][q], case["ref32"][q], q, "odd columns", stats, case["geo"])


def test_one_wrong_enc0_element_on_a_tile_border_fails_the_stage_check_and_not_the_end_check():
    """the shipped human-insertion weights at L = 8000, a site whose window has N runs and IUPAC codes on the tile borders"""
    case = D.cached_case("indel_pretrained_human_insertion.npz", 16, SEED + 1)
    site, ch = 12, 5
    one = slice(site, site + 1)
    geo, orc, ref32 = case["geo"], case["orc64"], {"enc0": case["ref32"]["enc0"][one]}
    want64 = {k: case["want64"][k][one] for k in ("enc0", "out")}
    clean = D.rest_of_network(orc, 0, want64["enc0"])
    assert float((clean["out"] - want64["out"]).abs().max()) <= 1e-12      # rest_of_network restates the oracle's own second half
    site = 0
    winners = set(int(c) for c in clean["feat"][site].argmax(dim=1))
    col = next(c for c in (247, 248, 251, 252) if all(abs(c - w) > 16 for w in winners))      # no channel's arg-max is near it
    wrong_enc0 = want64["enc0"].clone()
    wrong_enc0[site, ch, col] += 1e-3 * float(want64["enc0"].abs().max())
    wrong = D.rest_of_network(orc, 0, wrong_enc0)
    stats = _Stats("host", tag="indel_stages")
    with pytest.raises(AssertionError) as failure:
        D.check_tap(wrong_enc0.float(), want64["enc0"], ref32["enc0"], "enc0", "one wrong element", stats, geo)
    assert f"enc0[{site}, {col}, {ch}]" in str(failure.value) and f"level 0 column {col}:" in str(failure.value)
    feat_moved = float((wrong["feat"] - clean["feat"]).abs().max())
    gmax_moved = float((wrong["gmax"] - clean["gmax"]).abs().max())
    moved = float((wrong["out"] - want64["out"]).abs().max())
    tol = D.END_TOL * max(1.0, float(want64["out"].abs().max()))
    print(f"[indel_stages] enc0[{site}, {col}, {ch}] off by 1e-3 of the tensor's magnitude: out_conv's output moves by {feat_moved:.3e}, its "
          f"global maximum by {gmax_moved:.3e}, the scores by {moved:.3e} (end check allows {tol:.3e})")
    assert feat_moved > 0 and gmax_moved < feat_moved      # it reaches the row the maximum is taken over, and the maximum hides (most of) it
    assert moved <= tol                                    # the end check passes with the wrong element in
    # ... and so does the float32 result a kernel would hand back
    assert float((wrong["out"].float().double() - want64["out"]).abs().max()) <= tol


def test_run_maxima_follow_the_persistent_decoders_slots():
    """a row cut into runs of tiles: zeros inside a run, the run's maximum at its end; a row whose last tile holds nothing is refused"""
    tiles = torch.tensor([[[1.0, 5.0], [3.0, 2.0], [2.0, 9.0], [4.0, 1.0]]], dtype=torch.float64)      # [1 row][4 tiles][2 channels]
    slots = np.array([[[0, 0], [3.0, 5.0], [0, 0], [4.0, 9.0]]], np.float32)
    want, _ = D.run_maxima(slots, tiles, tiles.float())
    assert torch.equal(want, torch.tensor(slots, dtype=torch.float64))
    per_tile, _ = D.run_maxima(tiles.numpy(), tiles, tiles.float())
    assert torch.equal(per_tile, tiles)
    with pytest.raises(AssertionError, match="last tile"):
        D.run_maxima(np.array([[[1.0, 5.0], [0, 0], [0, 0], [0, 0]]], np.float32), tiles, tiles.float())


def test_geometry_and_tile_labels():
    geo = D.Geometry(4000, n_class=2)
    assert geo.len == [4000, 1000, 200, 40, 8, 4] and geo.parts_max == 17 and geo.tail_parts() == 17 and geo.tail_parts(poly=False) == 16
    assert sum(D.Geometry(8000).per_pos()) == 4 * 8000 * 2 + 64000 + 32000 + 9600 + 2560 + 640 + 384 + 2 * 64000 + 128000 + 64000 + 8 * 33
    with pytest.raises(AssertionError):
        D.Geometry(800)
    geo = D.Geometry(8000)
    assert "column 0 of tile 1 of the 248-column tiles" in D.tile_of(geo, 0, 248) and "column 251 of tile 0 of the 252" in D.tile_of(geo, 0, 251)
    assert "window start" in D.tile_of(geo, 0, 3) and "window end" in D.tile_of(geo, 0, 7995) and "window" not in D.tile_of(geo, 0, 4000)
    assert "level-0 tile 1 emits" in D.tile_of(geo, 1, 62)


def test_region_reader_refuses_a_changed_carve():
    case = _small()
    geo = case["geo"]
    lanes_B = (15, 9)
    ws, layout = _synthetic_workspace(case, lanes_B)
    parts = geo.tail_parts()
    with pytest.raises(AssertionError, match="regions"):
        D.forward_regions(ws, layout[:-1], 2, lanes_B, geo, parts)
    with pytest.raises(AssertionError, match="regions"):
        D.forward_regions(ws, layout, 1, lanes_B[:1], geo, parts)
    swapped = list(layout)
    swapped[1], swapped[2] = swapped[2], swapped[1]
    with pytest.raises(AssertionError, match="region E0"):
        D.forward_regions(ws, swapped, 2, lanes_B, geo, parts)
    with pytest.raises(AssertionError, match="lane 1 region S"):
        D.forward_regions(ws, layout, 2, (15, 8), geo, parts)
    # fewer tiles per row than M is sized for: what lies behind them must be untouched
    with pytest.raises(AssertionError, match="behind"):
        D.forward_regions(ws, layout, 2, lanes_B, geo, parts - 1)
