"""The checker of the per-stage SNV parity tests (tests/_snv_stages_data.py) without a device: the float32 oracle's own taps pass it
for every configuration of tests/test_gpu_snv_stages.py, one wrong element of a pooled row fails it by name -- and the same wrong
element moves the final probabilities by less than the end check's 1e-5: what the end check cannot see, shown in the suite itself."""
import numpy as np
import pytest
import torch

from oracle import encode_ref
from tests import _snv_stages_data as D
from tests._parity import _Stats

# (model_no, local_radius, distal_radius, sites): the windows of the GPU module at sizes a CPU affords
CONFIGS = [(2, 5, 100, 48), (1, 5, 100, 48), (2, 7, 200, 48), (1, 7, 200, 48), (2, 7, 1000, 32), (1, 7, 1000, 32),
           (2, 7, 2000, 12), (2, 7, 3000, 12), (2, 7, 16000, 6)]


def _length(R):
    return 20_000 if R <= 1000 else (40_000 if R <= 4000 else 90_000)


@pytest.mark.parametrize("cfg", CONFIGS)
def test_float32_oracle_passes_the_stage_checks(cfg):
    model_no, r, R, n = cfg
    case = D.cached_case(model_no, r, R, n, 40 + R + model_no, _length(R))
    stats = _Stats("host", tag="snv_stages")
    (L2l, L3l, _), (L2m, L3m, _) = D.tower_lengths(R)
    assert case["want64"]["x0"].shape == (n, L2l + L2m, 32) and case["want64"]["s3_0"].shape == (n, L3l, 32)
    assert case["want64"]["s3_1"].shape == (n, L3m, 32) and case["want64"]["x0"].dtype == torch.float64
    for q in D.QUANTITIES:
        if q == "local_logits" and model_no != 2:
            continue
        D.check_stage(case["ref32"][q].numpy(), case["want64"][q], case["ref32"][q], q, f"{cfg}", stats,
                      column_label=(lambda j: D.segment_of(R, j)) if q == "s3_0" else None)
    stats.show()
    # the windows hold what the cases are about: an ambiguity code, off-chromosome N at both ends, both strands
    win = encode_ref.gather_windows(case["codes"], case["pos"], R, "snv")
    assert (win > 4).any() and (win[0, :R] == 4).all() and (win[2, R + 1:] == 4).all() and set(case["strand"][:8]) == {0, 1}


@pytest.mark.parametrize("cfg", [(7, 300), (10, 1000)])
def test_float32_oracle_passes_the_stage_checks_on_the_reuse_sites(cfg):
    """the reuse path's configurations: dense runs on both strands at both chromosome ends and in the middle, 24 sites each"""
    r, R = cfg
    case = D.reuse_case(r, R, 340 + R, runs=(24, 24, 24))
    stats = _Stats("host", tag="snv_stages")
    assert len(case["pos"]) == 72 and case["pos"].min() == 0 and case["pos"].max() == len(case["seq"]) - 1
    assert set(case["strand"][case["pos"] < 24]) == {0, 1} and set(case["strand"][case["pos"] > 6000]) == {0, 1}
    for q in D.QUANTITIES:
        D.check_stage(case["ref32"][q].numpy(), case["want64"][q], case["ref32"][q], q, f"reuse sites {cfg}", stats)
    stats.show()


def test_one_wrong_pooled_element_fails_the_stage_check_and_not_the_end_check():
    model_no, r, R, n = 2, 7, 1000, 32
    case = D.cached_case(model_no, r, R, n, 40 + R + model_no, _length(R))
    want64, ref32 = case["want64"], case["ref32"]
    orc, clean_s3 = case["orc32"], ref32["s3_0"]
    clean_logits, clean_row = D.rest_of_tower(orc, "_2", clean_s3, with_feature_row=True)
    site, ch = 5, 11
    winner = int(clean_s3[site, :, ch].argmax())
    # the first column -- not the one that holds the channel's maximum -- from which the wrong value provably arrives in the row the
    # global max is taken over (the last conv's output): neither a ReLU nor a max-pool on the way has absorbed it
    for col in range(clean_s3.shape[1]):
        s3 = clean_s3.clone()
        s3[site, col, ch] += 1e-3 * float(clean_s3.abs().max())
        wrong_logits, wrong_row = D.rest_of_tower(orc, "_2", s3, with_feature_row=True)
        if col != winner and not torch.equal(wrong_row, clean_row):
            break
    else:
        raise AssertionError("no column of this channel reaches the last conv's output")
    stats = _Stats("host", tag="snv_stages")
    with pytest.raises(AssertionError) as failure:
        D.check_stage(s3.numpy(), want64["s3_0"], ref32["s3_0"], "s3_0", "one wrong element", stats)
    assert f"s3_0[{site}, {col}, {ch}]" in str(failure.value)
    # ... and through the global max, the fc, the softmax and the head: the probabilities the end check compares
    clean = D.head(model_no, clean_logits, ref32["mid_logits"], ref32["local_logits"])
    wrong = D.head(model_no, wrong_logits, ref32["mid_logits"], ref32["local_logits"])
    assert float((clean.log() - ref32["out"]).abs().max()) <= 1e-5      # rest_of_tower + head restate the oracle's own second half
    row_moved = float((wrong_row - clean_row).abs().max())
    feat_moved = float((wrong_row.max(dim=2).values - clean_row.max(dim=2).values).abs().max())
    moved = float((wrong.double() - clean.double()).abs().max())
    print(f"[snv_stages] s3_0[{site}, {col}, {ch}] off by 1e-3 of the tensor's magnitude: the last conv's output moves by {row_moved:.3e}, "
          f"its global max by {feat_moved:.3e}, the tower's logits by {float((wrong_logits - clean_logits).abs().max()):.3e} "
          f"(of {float(clean_logits[site].abs().max()):.1f}), the probabilities by {moved:.3e}")
    assert row_moved > 0 and feat_moved < row_moved      # it reaches the pooled feature row, and the global max hides (most of) it
    assert moved < D.PROB_TOL
    assert float((wrong.double() - want64["out"].exp()).abs().max()) <= D.PROB_TOL      # the end check passes with the wrong element in


def test_planned_geometries():
    """what the tail and wrap cases of the GPU module are built from"""
    assert D.tower_lengths(100) == ((14, 2, 1), (67, 23, 8)) and D.tower_lengths(1000) == ((134, 20, 7), (67, 23, 8))
    assert D.wave_sites(100) == (9, 2) and D.wave_sites(200) == (5, 2) and D.wave_sites(1000) == (1, 2)
    assert D.short_stage_sites(1000) == ((6, 5), "wave") and D.short_stage_sites(100) == ((32, 10), "tile")
    assert D.longwin_plan(1000) is None
    plan = D.longwin_plan(2000)
    assert D.tower_lengths(2000)[0][:2] == (267, 39) and plan["nA"] == 1 and plan["LpA"] == 21
    assert D.segment_of(2000, 0).startswith("equal segment 0") and D.segment_of(2000, 38).startswith("last segment")
    plan = D.longwin_plan(3000)
    assert D.tower_lengths(3000)[0][:2] == (401, 58) and plan["nA"] == 2 and plan["SB"] == 259
    assert D.segment_of(3000, 19).startswith("equal segment 0") and D.segment_of(3000, 20).startswith("equal segment 1")
    assert D.segment_of(3000, 38).startswith("equal segment 1") and D.segment_of(3000, 39).startswith("last segment")


def test_symbol_windows_are_the_one_hot_windows():
    _, codes = D.sequence(3, 3000)
    pos, strand = D.edge_sites(len(codes), 100, 40, 4)
    sym = D.symbol_windows(codes, pos, strand, 100)
    want = encode_ref.onehot_encode(codes, pos, D.strand_symbols(strand), 100)
    assert np.array_equal(encode_ref._OHE[sym].transpose(0, 2, 1), want) and (strand == 1).any() and (sym > 4).any()


def test_region_reader_refuses_a_changed_carve():
    n, R, ncol = 3, 100, 9
    (L2l, L3l, _), (L2m, L3m, _) = D.tower_lengths(R)
    sizes = [n * 16, n * ncol * 8, 16, n * (L2l + L2m) * 128, n * 64, n * L3l * 128, n * L3m * 128, 64]
    offs = np.cumsum([0] + [(s + 255) & ~255 for s in sizes])
    ws = np.zeros(int(offs[-1]), np.uint8)
    layout = [(int(o), s) for o, s in zip(offs, sizes)]
    reg = D.forward_regions(ws, layout, n, 2, ncol, R, dense=False)
    assert reg["x0"].shape == (n, L2l + L2m, 32) and reg["xlogit"].shape == (n, 4)
    with pytest.raises(AssertionError, match="region s3_0"):
        D.forward_regions(ws, layout[:5] + [layout[6], layout[5]] + layout[7:], n, 2, ncol, R, dense=False)
    with pytest.raises(AssertionError, match="regions"):
        D.forward_regions(ws, layout[:-1], n, 2, ncol, R, dense=False)
