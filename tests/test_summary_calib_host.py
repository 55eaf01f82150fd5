"""The numpy twin of the calibration-metrics summary (predict.summary_calib_host, calib_metrics_from_sums)
and the tool's flag refusals, without a device: parity with the reference's own ECELoss / ClasswiseECELoss / BrierScore / NLL numbers
of tests/golden/analytics.npz (2e-6: the reference evaluates them in float32, tests/test_analytics.py), bit identity of the integer
tables over parts and permutations, the row checks, the bin rule and the class count of the classwise ECE by hand-computed tables."""
import importlib.util
import os

import numpy as np
import pytest

from mural_amd import predict as P
from tests import _calib_data as D
from tests import _util as U

CASES = [("snv", 4), ("indel", 3)]


@pytest.mark.parametrize("tag,nc", CASES)
@pytest.mark.parametrize("dt", ["float32", "float64"])
def test_fixture_parity(tag, nc, dt):
    fx = U.load("analytics.npz")
    prob, label = fx[f"{tag}_metrics_prob_{dt}"], fx[f"{tag}_label"]
    assert prob.dtype == np.dtype(dt)
    table, status = P.summary_calib_host(prob, label, nc)
    got = P.calib_metrics_from_sums(table, 50, nc)
    want = fx[f"{tag}_metrics_{dt}"]
    err = np.abs(np.array([got["nll"], got["ece"], got["c_ece"], got["brier"]]) - want)
    print(tag, dt, "largest difference", err.max())
    assert status == 0 and got["rows"] == len(label) and got["label_counts"] == np.bincount(label, minlength=nc).tolist()
    assert (err <= 2e-6).all(), (got, want)


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_tables_are_bit_identical_over_parts_and_order(dtype):
    prob, label = D.random_rows(5000, 4, 1, dtype)
    prob[7, 1], label[7] = 0.0, 1                      # an infinite NLL term among them
    whole, status = P.summary_calib_host(prob, label, 4, 15)
    assert status == 0 and whole[0] == 5000 and whole[1] == 1
    parts = None
    for a, b in ((0, 1), (1, 1300), (1300, 5000)):
        parts, st = P.summary_calib_host(prob[a:b], label[a:b], 4, 15, into=parts)
        assert st == 0
    perm = np.random.default_rng(2).permutation(5000)
    shuffled, _ = P.summary_calib_host(prob[perm], label[perm], 4, 15)
    assert np.array_equal(parts, whole) and np.array_equal(shuffled, whole)
    lo = P._calib_lo_cells(4, 15)
    assert (whole[lo] < np.uint64(1 << D.LO_BITS)).all() and whole[lo].any()


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_edge_rows_by_hand(dtype):
    """The bin rule -- 0.5 in the bin whose upper bound is 0.5, a confidence of 1.0 in the last bin, a class score of 0 in none --, the
    first maximum as the prediction, an exact 0 at the label (inf_rows, nll == inf, Brier and bins still counted)."""
    nc, nb = D.EDGE_NC, D.EDGE_NB
    assert P.calib_bounds(nb)[5] == np.float32(0.5) and P.calib_bounds(nb).dtype == np.float32
    table, status = P.summary_calib_host(D.EDGE_PROB.astype(dtype), D.EDGE_LABEL, nc, nb)
    assert status == 0
    assert np.array_equal(D.without_nll(table, nc), D.edge_table())
    tol = D.nll_tolerance(dtype)
    assert abs(D.pair_value(table, 2 + nc, D.NLL_BITS) - D.EDGE_NLL) < tol
    m = P.calib_metrics_from_sums(table, nb, nc)
    assert m["rows"] == 4 and m["nll"] == float("inf") and m["brier"] == 2.25 / 4 and m["label_counts"] == [1, 0, 2, 1]
    assert m["ece"] == (0.0 + 0.5 + 0.25) / 4                  # |1 - 1| * 2 + |0.5 - 0| + |0.25 - 0|, over the rows
    # per class: 0: |1 - 1| + .5 + .25; 1: .5 + .25; 2: .25 + 0; 3: |.25 - 1|
    assert m["c_ece"] == (0.75 + 0.75 + 0.25 + 0.75) / 4 / 4
    without = P.calib_metrics_from_sums(P.summary_calib_host(np.delete(D.EDGE_PROB, 1, 0).astype(dtype), np.delete(D.EDGE_LABEL, 1), nc, nb)[0],
                                        nb, nc)
    assert abs(without["nll"] - D.EDGE_NLL / 3) < tol


def test_row_checks_and_status():
    nc, nb = D.EDGE_NC, D.EDGE_NB
    clean, _ = P.summary_calib_host(D.EDGE_PROB, D.EDGE_LABEL, nc, nb)
    for prob, label, bit in D.BAD_ROWS:
        table, status = P.summary_calib_host(np.vstack([D.EDGE_PROB, [prob]]), np.r_[D.EDGE_LABEL, label], nc, nb)
        assert status == bit and np.array_equal(table, clean), (prob, label)
        alone, status = P.summary_calib_host(np.array([prob]), np.array([label]), nc, nb)
        assert status == bit and not alone.any()
    prob = np.vstack([[r[0] for r in D.BAD_ROWS[:3]], D.EDGE_PROB, [r[0] for r in D.BAD_ROWS[3:]]])
    label = np.r_[[r[1] for r in D.BAD_ROWS[:3]], D.EDGE_LABEL, [r[1] for r in D.BAD_ROWS[3:]]]
    table, status = P.summary_calib_host(prob.astype(np.float32), label.astype(np.float32), nc, nb)
    assert status == 10 and np.array_equal(table, P.summary_calib_host(D.EDGE_PROB.astype(np.float32), D.EDGE_LABEL, nc, nb)[0])
    # a label that is no whole number, a row without a positive probability
    assert P.summary_calib_host(D.EDGE_PROB[:1], np.array([0.5]), nc, nb)[1] == 2
    assert P.summary_calib_host(np.zeros((1, 4)), np.array([0]), nc, nb)[1] == 8
    empty = P.calib_metrics_from_sums(np.zeros(P.calib_cells(nc, nb), np.uint64), nb, nc)
    assert empty["rows"] == 0 and all(np.isnan(empty[k]) for k in ("nll", "ece", "c_ece", "brier"))


def test_metrics_from_sums_against_plain_float64():
    """``calib_metrics_from_sums`` against the definitions in float64; the classwise ECE averages over max label + 1 classes when the
    highest class never occurs as a label (the reference's ClasswiseECELoss rule), not over n_class."""
    prob, label = D.random_rows(3000, 4, 5)
    label = np.where(label == 3, 0, label)
    assert label.max() == 2
    table, _ = P.summary_calib_host(prob, label, 4, 15)
    got = P.calib_metrics_from_sums(table, 15, 4)
    want = D.metrics_float64(prob, label, 15, P.calib_bounds(15))
    for key in ("nll", "ece", "c_ece", "brier"):
        assert abs(got[key] - want[key]) < 1e-12, key
    over_four = D.metrics_float64(prob, label, 15, P.calib_bounds(15), n_seen=4)["c_ece"]
    assert abs(got["c_ece"] - over_four) > 1e-4


def test_sink_on_host_shards(tmp_path):
    """SummarySink(calibration=True) over host shards: totals and per-chromosome metrics, the text file, abort() leaves nothing."""
    prob, label = D.random_rows(900, 4, 9, np.float32)
    shards = [("chrB", slice(0, 500)), ("chrA", slice(500, 900)), ("chrB", slice(100, 100))]
    for attempt in ("close", "abort"):
        sink = P.SummarySink(tmp_path / attempt, calibration=True, calibration_bins=15)
        for name, r in shards:
            n = len(label[r])
            sink({"chrom": name, "start": np.arange(n), "end": np.arange(n) + 1, "strand": np.zeros(n, np.uint8), "label": label[r].astype(np.float32),
                  "prob": prob[r], "n_class": 4, "calibrated": False})
        if attempt == "abort":
            sink.abort()
            assert not [f for f in os.listdir(tmp_path) if f.startswith("abort")]
            continue
        sink.close()
        res = sink.result()["calibration"]
        whole = P.calib_metrics_from_sums(P.summary_calib_host(prob, label, 4, 15)[0], 15, 4)
        assert {k: res[k] for k in whole} == whole and list(res["per_chromosome"]) == ["chrA", "chrB"]
        assert res["per_chromosome"]["chrA"] == P.calib_metrics_from_sums(P.summary_calib_host(prob[500:], label[500:], 4, 15)[0], 15, 4)
        assert np.array_equal(sink.calibration_sums()["all"], P.summary_calib_host(prob, label, 4, 15)[0])
        lines = open(str(tmp_path / "close") + ".calibration.txt").read().split("\n")
        assert lines[0].split("\t") == ["chrom", "rows", "nll", "ece", "c_ece", "brier"] and [ln.split("\t")[0] for ln in lines[1:4]] == ["all", "chrA", "chrB"]
        assert lines[1] == "all\t900\t" + "\t".join("%.8f" % whole[k] for k in ("nll", "ece", "c_ece", "brier")) and lines[4] == ""
    with pytest.raises(ValueError, match="calibrated already"):
        P.SummarySink(None, fit_calibrator="FullDiri", poisson=True)
    with pytest.raises(ValueError, match="unknown calibrator"):
        P.SummarySink(None, fit_calibrator="Platt")
    sink = P.SummarySink(None, fit_calibrator="FullDiri", fit_row_terms=lambda *a: None)
    with pytest.raises(ValueError, match="calibrated already"):
        sink({"chrom": "chrA", "start": np.arange(2), "end": np.arange(2) + 1, "strand": np.zeros(2, np.uint8), "label": np.zeros(2, np.float32),
              "prob": prob[:2], "n_class": 4, "calibrated": True})
    with pytest.raises(ValueError, match="too large"):
        big = P.SummarySink(None, calibration=True, calibration_bins=400)
        big({"chrom": "chrA", "start": np.arange(2), "end": np.arange(2) + 1, "strand": np.zeros(2, np.uint8), "label": np.zeros(2, np.float32),
             "prob": prob[:2], "n_class": 4, "calibrated": False})


def _tool():
    spec = importlib.util.spec_from_file_location("predict_files", os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))),
                                                                                  "tools", "predict_files.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def test_tool_flag_refusals():
    """Pure argument handling: nothing is loaded before these are refused."""
    main = _tool().main
    base = ["MODEL", "genome.fa"]
    with pytest.raises(SystemExit, match="--mutations FILE"):          # --regions alone: every label would be 0
        main(base + ["--regions", "chr1", "--summary", "p", "--calibration_metrics", "--no-table"])
    with pytest.raises(SystemExit, match="--scale_factor"):
        main(base + ["sites.bed", "out.tsv", "--summary", "p", "--calibration_metrics", "--fit_calibrator", "FullDiri", "--scale_factor", "2.5"])
    with pytest.raises(SystemExit, match="Poisson"):
        main(base + ["sites.bed", "--summary", "p", "--calibration_metrics", "--fit_calibrator", "FullDiri", "--poisson", "--no-table"])
    with pytest.raises(SystemExit, match="--summary PREFIX"):
        main(base + ["sites.bed", "out.tsv", "--calibration_metrics"])
    with pytest.raises(SystemExit, match="go with --calibration_metrics"):
        main(base + ["sites.bed", "out.tsv", "--summary", "p", "--window_size", "1000", "--n_bins", "15"])
    with pytest.raises(SystemExit, match="one of FullDiri"):
        main(base + ["sites.bed", "out.tsv", "--summary", "p", "--calibration_metrics", "--fit_calibrator", "Platt"])
    with pytest.raises(SystemExit, match="--n_bins must be positive"):
        main(base + ["sites.bed", "out.tsv", "--summary", "p", "--calibration_metrics", "--n_bins", "0"])
