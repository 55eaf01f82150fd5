"""Loss and calibration metrics reduced in flight (csrc/summary_calib.hip: mural_summary_calib_rows; SummarySink(calibration=True,
fit_calibrator=...)): the device entry against the reference's own numbers of tests/golden/analytics.npz
(2e-6, tests/test_analytics.py: the reference evaluates them in float32), bit identity of the integer tables over launches, orders and
contention shapes, the numpy twin, the edge rows, a regions run through the sink, and the calibrator fit from retained shards (weights
1e-5 relative, the bar of tests/test_analytics.py)."""
import os

import numpy as np
import pytest
import torch

from mural_amd import predict as P
from tests import _calib_data as D
from tests import _util as U

pytestmark = pytest.mark.gpu

CASES = [("snv", 4), ("indel", 3)]


def _device_table(prob, label, nc, nb, cuts=None, label_dtype=torch.int64):
    """(table uint64, status) of the rows fed in the launches `cuts` names (one by default)."""
    dev = torch.device("cuda", torch.cuda.current_device())
    table = torch.zeros(P.calib_cells(nc, nb), dtype=torch.int64, device=dev)
    status = torch.zeros(1, dtype=torch.int32, device=dev)
    bounds = torch.from_numpy(P.calib_bounds(nb)).to(dev)
    d_prob = torch.from_numpy(np.ascontiguousarray(prob)).to(dev)
    d_label = torch.from_numpy(np.ascontiguousarray(label)).to(dev, label_dtype)
    cuts = [0, len(label)] if cuts is None else cuts
    for a, b in zip(cuts[:-1], cuts[1:]):
        P.calib_rows_device(d_prob[a:b], d_label[a:b], nc, nb, bounds, table, status)
    return table.cpu().numpy().view(np.uint64), int(status.item())


def _four(m):
    return np.array([m["nll"], m["ece"], m["c_ece"], m["brier"]])


@pytest.mark.parametrize("tag,nc", CASES)
@pytest.mark.parametrize("dt", ["float32", "float64"])
def test_fixture_parity(tag, nc, dt):
    """The test that pins the arithmetic to the reference: its ECELoss / ClasswiseECELoss / BrierScore / NLL numbers."""
    fx = U.load("analytics.npz")
    prob, label = fx[f"{tag}_metrics_prob_{dt}"], fx[f"{tag}_label"]
    table, status = _device_table(prob, label, nc, 50)
    got = P.calib_metrics_from_sums(table, 50, nc)
    want = fx[f"{tag}_metrics_{dt}"]
    err = np.abs(_four(got) - want)
    print(tag, dt, "largest difference", err.max())
    assert status == 0 and got["rows"] == len(label) and got["label_counts"] == np.bincount(label, minlength=nc).tolist()
    assert (err <= 2e-6).all(), (got, want)


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_tables_are_bit_identical(dtype):
    """4 099 rows (no multiple of 64 or 256) as one launch, as launches of 1, 65 and 4 033 rows, permuted; and a constant row
    repeated, whose rows all share one bin per group: its table is the one row's, times the rows."""
    n, nc, nb = 4099, 4, 50
    prob, label = D.random_rows(n, nc, 3, dtype)
    prob[11, 2], label[11] = 0.0, 2
    whole, status = _device_table(prob, label, nc, nb)
    assert status == 0 and whole[0] == n and whole[1] == 1
    perm = np.random.default_rng(4).permutation(n)
    assert np.array_equal(_device_table(prob, label, nc, nb, [0, 1, 66, n])[0], whole)
    assert np.array_equal(_device_table(prob[perm], label[perm], nc, nb)[0], whole)
    assert np.array_equal(_device_table(prob, label, nc, nb, label_dtype=torch.float32)[0], whole)
    lo = P._calib_lo_cells(nc, nb)
    assert (whole[lo] < np.uint64(1 << D.LO_BITS)).all()
    one, _ = _device_table(prob[5:6], label[5:6], nc, nb)
    same, status = _device_table(np.repeat(prob[5:6], n, axis=0), np.repeat(label[5:6], n), nc, nb)
    assert status == 0 and np.array_equal(same, P._calib_fold(one * np.uint64(n), nc, nb))
    assert np.array_equal(_device_table(np.repeat(prob[5:6], n, axis=0), np.repeat(label[5:6], n), nc, nb, [0, 1, 66, n])[0], same)


def test_small_and_extreme_shapes_against_the_twin():
    """n of 0, 1 and 63, n_class of 2, 8 and 16, n_bins of 1, 15 and 50 on float64 rows: counts and status equal the twin's exactly, the
    metrics agree within 2e-6."""
    for nc in (2, 8, 16):
        for nb in (1, 15, 50):
            for n in (0, 1, 63):
                prob, label = D.random_rows(n, nc, 100 * nc + n, sharp=False)
                got, status = _device_table(prob, label, nc, nb)
                want, want_status = P.summary_calib_host(prob, label, nc, nb)
                assert status == want_status == 0 and np.array_equal(got[:2 + nc], want[:2 + nc]), (nc, nb, n)
                if n:
                    a, b = P.calib_metrics_from_sums(got, nb, nc), P.calib_metrics_from_sums(want, nb, nc)
                    assert np.abs(_four(a) - _four(b)).max() <= 2e-6, (nc, nb, n)
                else:
                    assert not got.any()


def test_too_many_bins_are_refused():
    dev = torch.device("cuda", torch.cuda.current_device())
    assert P.calib_cells(16, 50) <= 4096 < P.calib_cells(16, 64)
    prob, label = D.random_rows(63, 16, 1)
    table = torch.zeros(P.calib_cells(16, 64), dtype=torch.int64, device=dev)
    status = torch.zeros(1, dtype=torch.int32, device=dev)
    bounds = torch.from_numpy(P.calib_bounds(64)).to(dev)
    with pytest.raises(ValueError, match=r"n_bins \* \(n_class \+ 1\)"):
        P.calib_rows_device(torch.from_numpy(prob).to(dev), torch.from_numpy(label).to(dev), 16, 64, bounds, table, status)
    torch.cuda.synchronize()
    assert not table.any() and int(status.item()) == 0      # nothing was launched
    from mural_amd import _lib
    assert _lib.lib().mural_summary_calib_cells(16, 64) == 0 and _lib.lib().mural_summary_calib_cells(16, 50) == P.calib_cells(16, 50)


def test_float64_rows_against_the_twin():
    n, nc, nb = 4099, 4, 50
    prob, label = D.random_rows(n, nc, 7)
    clean = (P.calib_metrics_from_sums(_device_table(prob, label, nc, nb)[0], nb, nc), P.calib_metrics_from_sums(P.summary_calib_host(prob, label, nc, nb)[0], nb, nc))
    print("device - twin", _four(clean[0]) - _four(clean[1]))
    assert np.abs(_four(clean[0]) - _four(clean[1])).max() <= 2e-6
    assert np.abs(_four(clean[0]) - _four(D.metrics_float64(prob, label, nb, P.calib_bounds(nb)))).max() <= 2e-6
    # exact zeros at the label and rows that are skipped: counts and status exactly
    prob[[3, 700, 4098], [1, 2, 3]] = 0.0
    label[[3, 700, 4098]] = [1, 2, 3]
    label[[9, 2000]] = [-1, nc]
    prob[[10, 3000], [0, 1]] = [np.nan, -0.5]
    got, status = _device_table(prob, label, nc, nb)
    want, want_status = P.summary_calib_host(prob, label, nc, nb)
    assert status == want_status == 10 and np.array_equal(got[:2 + nc], want[:2 + nc]) and got[0] == n - 4 and got[1] == 3
    a, b = P.calib_metrics_from_sums(got, nb, nc), P.calib_metrics_from_sums(want, nb, nc)
    assert a["nll"] == b["nll"] == float("inf") and np.abs(_four(a)[1:] - _four(b)[1:]).max() <= 2e-6


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_edge_rows(dtype):
    """The edge rows of tests/test_summary_calib_host.py on the device: the hand-computed table, the status bits, the skipped rows."""
    nc, nb = D.EDGE_NC, D.EDGE_NB
    table, status = _device_table(D.EDGE_PROB.astype(dtype), D.EDGE_LABEL, nc, nb)
    assert status == 0 and np.array_equal(D.without_nll(table, nc), D.edge_table())
    assert abs(D.pair_value(table, 2 + nc, D.NLL_BITS) - D.EDGE_NLL) < D.nll_tolerance(dtype)
    m = P.calib_metrics_from_sums(table, nb, nc)
    assert m["nll"] == float("inf") and m["brier"] == 2.25 / 4 and m["ece"] == 0.75 / 4 and m["c_ece"] == 2.5 / 16
    for prob, label, bit in D.BAD_ROWS:
        got, status = _device_table(np.vstack([D.EDGE_PROB, [prob]]).astype(dtype), np.r_[D.EDGE_LABEL, label], nc, nb)
        assert status == bit and np.array_equal(got, table), (prob, label)
    prob = np.vstack([[r[0] for r in D.BAD_ROWS[:3]], D.EDGE_PROB, [r[0] for r in D.BAD_ROWS[3:]]]).astype(dtype)
    label = np.r_[[r[1] for r in D.BAD_ROWS[:3]], D.EDGE_LABEL, [r[1] for r in D.BAD_ROWS[3:]]]
    for label_dtype in (torch.int64, torch.int32, torch.float32):
        got, status = _device_table(prob, label, nc, nb, label_dtype=label_dtype)
        assert status == 10 and np.array_equal(got, table)
    assert _device_table(np.zeros((1, 4), dtype), np.zeros(1, np.int64), nc, nb)[1] == 8      # no positive probability


class _Collect:
    """Keeps every shard's probabilities and labels (device copies)."""
    takes_aligned_blocks = True

    def __init__(self):
        self.prob, self.label = [], []

    def __call__(self, shard):
        k = int(shard.get("n_class", shard["prob"].shape[1]))
        self.prob.append(shard["prob"][:, :k].clone())
        self.label.append(shard["label"].clone())


@pytest.fixture(scope="module")
def region_files(tmp_path_factory):
    """(directory, FASTA, model, its config): the synthetic Network2 and records of tests/test_gpu_region_labels.py."""
    from mural_amd.model import model_choice, weights_init
    from tests.test_gpu_region_labels import RECORDS, R_LOCAL
    from tests.test_gpu_regions import R_DISTAL
    d = tmp_path_factory.mktemp("calib_regions")
    fa = d / "g.fa"
    fa.write_text("".join(f">{k}\n" + "\n".join(s[i:i + 60] for i in range(0, len(s), 60)) + "\n" for k, s in RECORDS.items()))
    ncol = 2 * R_LOCAL + 1 - 2
    config = dict(local_radius=R_LOCAL, local_order=3, local_hidden1_size=150, local_hidden2_size=75, distal_radius=R_DISTAL,
                  emb_dropout=0.1, local_dropout=0.1, CNN_kernel_size=3, CNN_out_channels=32, distal_fc_dropout=0.25, n_class=4,
                  model_no=2, seq_only=True, emb_dims=[(65, 2)] * ncol, segment_center=300000)
    torch.manual_seed(5)
    model = model_choice(2, config, dict(emb_dims=config["emb_dims"], n_cont=0, n_class=4, distal_order=1, in_channels=4), "snv")
    model.apply(weights_init)
    return d, str(fa), model.cuda().eval(), config


def test_regions_run_through_the_sink(region_files, tmp_path, monkeypatch):
    from mural_amd import evaluation as E
    from tests.test_gpu_region_labels import R_LOCAL, Listed
    _, fa, model, _ = region_files
    regions = {"chrA": [(40, 2500)]}
    listed = Listed(regions, "A")
    monkeypatch.setattr(P, "_ALIGNED_PART_ROWS", len(listed.sites["chrA"]) // 2 + 1)      # two parts
    fwd = P.HipShardForward(model, fa, local_radius=R_LOCAL, local_order=3)
    sink, rows, T = P.SummarySink(tmp_path / "s", calibration=True), _Collect(), {}
    n = P.predict_regions_sharded(fwd, regions, "A", sink=P.TeeSink(sink, rows), collect=False, mutations=listed.write(tmp_path / "m.bed"),
                                  timings=T)
    assert len(rows.prob) == 2 and n == len(listed.sites["chrA"])
    prob, label = torch.cat(rows.prob), torch.cat(rows.label)
    res = sink.result()["calibration"]
    direct, status = _device_table(prob.cpu().numpy(), label.cpu().numpy(), 4, 50, label_dtype=label.dtype)
    want = P.calib_metrics_from_sums(direct, 50, 4)
    assert status == 0 and want["rows"] == n and len(set(label.tolist())) == 4
    assert {k: res[k] for k in want} == want and res["per_chromosome"] == {"chrA": want}
    assert np.array_equal(sink.calibration_sums()["all"], direct)
    old = E.calibration_metrics(prob, label)
    assert np.abs(_four(res) - _four(old)).max() <= 2e-6, (res, old)
    lines = open(str(tmp_path / "s") + ".calibration.txt").read().split("\n")
    assert lines[0].split("\t") == ["chrom", "rows", "nll", "ece", "c_ece", "brier"] and len(lines) == 4 and lines[3] == ""
    for line, tag in zip(lines[1:3], ("all", "chrA")):
        cols = line.split("\t")
        assert cols[0] == tag and int(cols[1]) == n and cols[2:] == ["%.8f" % want[k] for k in ("nll", "ece", "c_ece", "brier")]
        assert np.abs(np.array([float(c) for c in cols[2:]]) - _four(want)).max() <= 0.5e-8


@pytest.mark.parametrize("tag,nc", CASES)
def test_fit_on_fixture_shards(tag, nc, tmp_path):
    from mural_amd.calibration import load_dirichlet_weights
    fx = U.load("analytics.npz")
    prob, label = fx[f"{tag}_prob"], fx[f"{tag}_label"]
    n, half = len(label), len(label) // 2 + 7
    dev = torch.device("cuda", torch.cuda.current_device())

    def run(prefix, **kw):
        sink = P.SummarySink(prefix, fit_calibrator="FullDiri", **kw)
        for i, r in enumerate((slice(0, half), slice(half, n))):          # a device shard and a host shard
            p, y = prob[r], label[r].astype(np.float32)
            shard = {"chrom": "chrF", "start": np.arange(len(y)) + r.start, "end": np.arange(len(y)) + r.start + 1, "strand": np.zeros(len(y), np.uint8),
                     "label": torch.from_numpy(y).to(dev) if i == 0 else y, "prob": torch.from_numpy(p).to(dev) if i == 0 else p, "n_class": nc,
                     "calibrated": False, "aligned": True}
            sink(shard)
        sink.close()
        return sink

    res = run(tmp_path / "f").result()["calibration"]
    want = fx[f"{tag}_fit_w"]
    assert np.abs(res["weights"] - want).max() < 1e-5 * np.abs(want).max(), np.abs(res["weights"] - want).max()
    assert abs(res["fit_loss"] - float(fx[f"{tag}_fit_loss"])) < 1e-9
    assert np.array_equal(load_dirichlet_weights(str(tmp_path / "f") + ".fdiri_cal.pkl"), res["weights"])
    print(tag, "nll before", res["nll"], "after", res["after"]["nll"])
    assert res["rows"] == res["after"]["rows"] == n and res["after"]["nll"] <= res["nll"] + 1e-9
    lines = open(str(tmp_path / "f") + ".calibration.txt").read().split("\n")
    assert [ln.split("\t")[0] for ln in lines[:4]] == ["chrom", "all", "all (after FullDiri)", "chrF"]
    with pytest.raises(ValueError, match=f"fit_rows_max={n - 1}"):
        run(tmp_path / "g", fit_rows_max=n - 1)
    assert not [f for f in os.listdir(tmp_path) if f.startswith("g.")]


def test_command_line_writes_the_sink_s_files(region_files, tmp_path, capsys):
    """tools/predict_files.py --summary P --calibration_metrics --n_bins N --fit_calibrator NAME --no-table on a regions run with
    mutations: the files and numbers of the sink driven through the API."""
    import importlib.util
    from mural_amd.calibration import load_dirichlet_weights
    from mural_amd.model import nn_utils
    from tests.test_gpu_region_labels import R_LOCAL, Listed
    d, fa, model, config = region_files
    ckpt = str(tmp_path / "model")
    nn_utils.save_model(model, None, config, ckpt)
    spec = importlib.util.spec_from_file_location("predict_files", os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))),
                                                                                  "tools", "predict_files.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    listed = Listed({"chrA": [(0, 3000)]}, "A")
    mut = listed.write(tmp_path / "cli.bed")
    mod.main([ckpt, fa, "--regions", "chrA:1-3000", "--focal", "A", "--mutations", mut, "--summary", str(tmp_path / "c"), "--calibration_metrics",
              "--n_bins", "15", "--fit_calibrator", "FullDiri", "--no-table"])
    printed = capsys.readouterr().out
    sink = P.SummarySink(tmp_path / "a", calibration_bins=15, fit_calibrator="FullDiri")
    P.predict_regions_sharded(P.HipShardForward(model, fa, local_radius=R_LOCAL, local_order=3), {"chrA": [(0, 3000)]}, "A", sink=sink,
                              collect=False, mutations=mut)
    res = sink.result()["calibration"]
    got, want = open(str(tmp_path / "c") + ".calibration.txt").read().split("\n"), open(str(tmp_path / "a") + ".calibration.txt").read().split("\n")
    assert [ln.split("\t")[0] for ln in got[:4]] == ["chrom", "all", "all (after FullDiri)", "chrA"]
    assert got[0] == want[0] and got[1] == want[1] and got[3] == want[3]                      # the metrics before the fit: bit for bit
    assert np.allclose([float(v) for v in got[2].split("\t")[1:]], [float(v) for v in want[2].split("\t")[1:]], rtol=0, atol=1e-6)
    w = load_dirichlet_weights(str(tmp_path / "c") + ".fdiri_cal.pkl")
    assert np.abs(w - res["weights"]).max() < 1e-5 * np.abs(res["weights"]).max() and res["after"]["nll"] <= res["nll"] + 1e-9
    assert "calibration - rows: %d, NLL: %.8f" % (res["rows"], res["nll"]) in printed and "calibration (after FullDiri) - rows:" in printed
    assert not os.path.exists(str(tmp_path / "c") + ".tsv")
