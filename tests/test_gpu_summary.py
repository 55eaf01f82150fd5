"""Genome summaries in flight (csrc/summary.hip, mural_amd.predict.SummarySink / TeeSink): the window tables of ``evaluate
--window_size`` and the totals of ``calc_scaling_factor`` reduced from the shards on the device, against numpy float64 on the same
values, against the table tools on the written table, and bit for bit against a second run."""
import ctypes as C
import os
import types

import numpy as np
import pytest
import torch

from tests import _summary_data as D

pytestmark = pytest.mark.gpu

RTOL = 1e-12                   # windows hold <= 1e4 non-negative terms: the float64 bound n * 2^-53 of a sum in any order


def _kernel(prob, start, end, label, n_class, windows, regions=None, lo=None, hi=None):
    """One mural_summary_rows call on device copies of the arrays: ({W: (first window, table)}, prob_sum, n_sites, status)."""
    from mural_amd import _lib
    lib = _lib.lib()
    dev = torch.device("cuda", torch.cuda.current_device())
    n, stride = len(start), 1 + 2 * n_class
    up = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)      # noqa: E731
    prob_d, start_d, end_d, label_d = up(prob), up(start), up(end), up(label)
    lo = int(start.min()) if lo is None else lo
    hi = int(start.max()) if hi is None else hi
    s = _lib.MuralSummaryRows()
    s.prob, s.prob_f64, s.prob_stride = prob_d.data_ptr(), int(prob.dtype == np.float64), prob_d.stride(0)
    s.start, s.end, s.label, s.n, s.n_class = start_d.data_ptr(), end_d.data_ptr(), label_d.data_ptr(), n, n_class
    s.label_kind = {np.dtype(np.float32): 0, np.dtype(np.int32): 1, np.dtype(np.int64): 2}[label.dtype]
    s.n_windows = len(windows)
    tabs = []
    for j, W in enumerate(windows):
        bins = hi // W - lo // W + 1
        tabs.append(torch.zeros((bins, stride), dtype=torch.float64, device=dev))
        s.window[j], s.bin0[j], s.n_bins[j], s.table[j] = W, lo // W, bins, tabs[j].data_ptr()
    if regions is not None:
        b0, b1 = up(np.r_[np.sort(regions[0]), 0].astype(np.int64)), up(np.r_[np.sort(regions[1]), 0].astype(np.int64))
        s.reg_b0, s.reg_b1, s.n_reg = b0.data_ptr(), b1.data_ptr(), len(regions[0])
    total = torch.zeros(1, dtype=torch.float64, device=dev)
    n_sites = torch.zeros(1, dtype=torch.int64, device=dev)
    status = torch.zeros(1, dtype=torch.int32, device=dev)
    s.total, s.n_sites, s.status = total.data_ptr(), n_sites.data_ptr(), status.data_ptr()
    ws = torch.empty(int(lib.mural_summary_workspace_bytes(n, n_class, len(windows))) // 8 + 1, dtype=torch.int64, device=dev)
    ws.fill_(-1)                                           # the call initialises what it reads
    _lib.check(lib.mural_summary_rows(C.byref(s), ws.data_ptr(), ws.numel() * 8, _lib.current_stream_ptr(dev)))
    return ({W: (lo // W, tabs[j].cpu().numpy()) for j, W in enumerate(windows)}, float(total.item()), int(n_sites.item()),
            int(status.item()))


def _same_tables(got, want, n_class, rtol=RTOL):
    """Row and label counts equal, probability sums within rtol of `want` ({W: (first window, table)}; trailing / leading empty windows
    of either side are ignored)."""
    assert set(got) == set(want)
    for W in want:
        (g0, g), (w0, w) = got[W], want[W]
        lo, hi = min(g0, w0), max(g0 + len(g), w0 + len(w))
        a, b = np.zeros((hi - lo, g.shape[1])), np.zeros((hi - lo, g.shape[1]))
        a[g0 - lo:g0 - lo + len(g)], b[w0 - lo:w0 - lo + len(w)] = g, w
        assert np.array_equal(a[:, :1 + n_class], b[:, :1 + n_class]), W
        err = np.abs(a[:, 1 + n_class:] - b[:, 1 + n_class:])
        print("W", W, "largest relative error of a probability sum", float((err / np.maximum(b[:, 1 + n_class:], 1e-300)).max()))
        assert (err <= rtol * b[:, 1 + n_class:]).all(), W


CASES = [(n, "mixed") for n in D.SIZES] + [(3 * D.CHUNK + 17, "long")]


# ---- 1. the kernel against numpy float64 ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n_class", [2, 4])
@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_kernel_equals_numpy_float64(dtype, n_class):
    from mural_amd import _lib
    from mural_amd.predict import summary_rows_host
    assert _lib.lib().mural_summary_chunk_rows() == D.CHUNK
    for n, layout in CASES:
        prob, start, end, label = D.rows(n, n_class, dtype, layout)
        assert prob.strides[0] == (n_class + 1) * prob.itemsize and start[0] == 0
        if layout == "mixed" and n > 3 * D.CHUNK:          # the borders the layout promises
            w = start // 64
            assert w[D.CHUNK] != w[D.CHUNK - 1] and w[2 * D.CHUNK - 1] != w[2 * D.CHUNK - 2] and w[2 * D.CHUNK] == w[2 * D.CHUNK - 1]
            assert w[3 * D.CHUNK + 1] != w[3 * D.CHUNK] and w[3 * D.CHUNK] == w[3 * D.CHUNK - 1] and w[4] - w[3] == 51 and w[3] - w[2] == 2
            assert (np.diff(start) == 0).any()
        if layout == "long":
            assert len(set((start // 64)[:3 * D.CHUNK + 2])) == 1
        got = _kernel(prob, start, end, label, n_class, D.WINDOWS)
        want = summary_rows_host(prob, start, end, label, n_class, D.WINDOWS)
        print("n", n, layout)
        _same_tables(got[0], want[0], n_class)
        assert len(got[0][10 ** 9][1]) == 1                # one window for the whole span
        assert got[2] == want[2] == n and got[3] == 0
        assert abs(got[1] - want[1]) <= RTOL * want[1]
        again = _kernel(prob, start, end, label, n_class, D.WINDOWS)
        assert all(np.array_equal(got[0][W][1].view(np.int64), again[0][W][1].view(np.int64)) for W in D.WINDOWS)
        assert np.float64(got[1]).view(np.int64) == np.float64(again[1]).view(np.int64) and got[2] == again[2]


def test_kernel_takes_integer_labels_and_flags_rows_outside_the_table():
    prob, start, end, label = D.rows(D.CHUNK + 1, 4, np.float32)
    want = _kernel(prob, start, end, label, 4, (64,))
    for dt in (np.int32, np.int64):
        got = _kernel(prob, start, end, label.astype(dt), 4, (64,))
        assert np.array_equal(got[0][64][1], want[0][64][1]) and got[1:] == want[1:]
    # a table that ends before the last rows: they are skipped and reported, nothing is written behind the table
    short = _kernel(prob, start, end, label, 4, (64,), hi=int(start[-200]))
    assert short[3] == 4 and short[0][64][1][:, 0].sum() < len(start)
    swapped = start.copy()
    swapped[[100, 1500]] = swapped[[1500, 100]]            # two rows out of order
    assert _kernel(prob, swapped, end, label, 4, (64,))[3] == 4


# ---- 2. totals with and without benchmark regions -------------------------------------------------------------------------------------
def test_totals_with_and_without_benchmark_regions():
    from mural_amd.predict import SummarySink
    n, k = D.CHUNK + 1, 4
    prob, start, end, label = D.rows(n, k, np.float32)
    i = n // 2
    regions = [(0, 500), (200, 900), (250, 300), (3300, 4800), (4000, 10 ** 6), (int(end[i]), int(end[i]) + 40), (int(start[-1]), int(start[-1]) + 1), (10 ** 7, 10 ** 7 + 5)]
    assert not any(lo < end[i] and hi > start[i] for lo, hi in regions[5:6])      # it touches the row's end: no overlap
    for regs in (None, regions):
        _, total, n_sites = D.brute_force(prob, start, end, label, k, (), regs)
        pair = None if regs is None else (np.array([r[0] for r in regs]), np.array([r[1] for r in regs]))
        got = _kernel(prob, start, end, label, k, (), pair)
        print("regions", regs is not None, "n_sites", got[2], "relative error", abs(got[1] - total) / total)
        assert got[2] == n_sites and abs(got[1] - total) <= RTOL * total and got[3] == 0
        assert regs is None or n_sites > n // 8
    # through the sink: the chromosome's regions are picked by name; a chromosome without any counts nothing
    bed = {"chrS": ([r[0] for r in regions], [r[1] for r in regions]), "chrOther": ([0], [10 ** 9])}
    for name, want in (("chrS", D.brute_force(prob, start, end, label, k, (), regions)[1:]), ("chrNone", (0.0, 0))):
        sink = SummarySink(benchmark_regions=bed)
        sink(_shard(name, prob, start, end, label, k))
        sink.close()
        res = sink.result()
        assert res["n_sites"] == want[1] and abs(res["prob_sum"] - want[0]) <= RTOL * want[0]


# ---- 3. parts ---------------------------------------------------------------------------------------------------------------------------
def _shard(name, prob, start, end, label, k, rows=slice(None), aligned=True, device="cuda"):
    up = (lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(device)) if device else (lambda a: a)      # noqa: E731
    shard = {"chrom": name, "start": up(start[rows]), "end": up(end[rows]), "strand": up(np.zeros(len(start[rows]), np.uint8)),
             "label": up(label[rows]), "prob": up(prob)[rows], "n_class": k, "calibrated": False}
    if aligned:
        shard["aligned"] = True
    return shard


def _sink_tables(res, k):
    """{W: (first window, table)} of a SummarySink result, the windows without rows filled in."""
    out = {}
    for W, (keys, table) in res["windows"].items():
        idx = np.array([we // W - 1 for _, we in keys])
        t = np.zeros((idx.max() - idx.min() + 1, 1 + 2 * k))
        t[idx - idx.min()] = table
        out[W] = (int(idx.min()), t)
    return out


def test_parts_accumulate_and_a_gathered_shard_is_sorted_first():
    from mural_amd.predict import SummarySink, summary_rows_host
    n, k = 3 * D.CHUNK + 17, 4
    prob, start, end, label = D.rows(n, k, np.float64)
    want = summary_rows_host(prob, start, end, label, k, D.WINDOWS)
    inside = int(np.nonzero(np.diff(start // 64) == 0)[0][40]) + 1      # a cut between two rows of one 64 bp window
    assert start[inside] // 64 == start[inside - 1] // 64
    cuts7 = sorted({0, 1, inside, D.CHUNK, D.CHUNK + 700, 2 * D.CHUNK + 5, 3 * D.CHUNK + 16, n})      # a one-row part first and last
    assert len(cuts7) == 8
    for cuts in ([0, n], [0, inside, n], cuts7):
        sink = SummarySink(windows=D.WINDOWS)
        for a, b in zip(cuts[:-1], cuts[1:]):
            sink(_shard("chrP", prob, start, end, label, k, slice(a, b)))
        sink.close()
        res = sink.result()
        print("parts", len(cuts) - 1)
        _same_tables(_sink_tables(res, k), want[0], k)
        assert res["n_sites"] == n and abs(res["prob_sum"] - want[1]) <= RTOL * want[1]
        assert [c for c, _ in res["windows"][64][0]] == ["chrP"] * len(res["windows"][64][0])
    perm = np.random.default_rng(3).permutation(n)
    sink = SummarySink(windows=D.WINDOWS)
    sink(_shard("chrP", prob[perm], start[perm], end[perm], label[perm], k, aligned=False))
    sink.close()
    _same_tables(_sink_tables(sink.result(), k), want[0], k)
    assert sink.result()["n_sites"] == n


# ---- 4. status ----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("what", ["label", "start"])
def test_bad_rows_raise_at_close_and_leave_no_file(tmp_path, what):
    from mural_amd.predict import SummarySink, TeeSink, TsvSink
    k = 4
    prob, start, end, label = D.rows(300, k, np.float32)
    if what == "label":
        label[77] = k
    else:
        start = start - 5
        start[3:] = np.maximum(start[3:], 0)
    for tee in (False, True):
        summary = SummarySink(tmp_path / "s", windows=(1000, 64))
        sink = TeeSink(TsvSink(tmp_path / "t.tsv"), summary) if tee else summary
        sink(_shard("chrB", prob, start, end, label, k))
        with pytest.raises(ValueError, match="mut_type outside" if what == "label" else "negative start"):
            sink.close()
        sink.abort()
        assert os.listdir(tmp_path) == []


def test_second_calibration_is_refused():
    from mural_amd.predict import SummarySink
    prob, start, end, label = D.rows(10, 4, np.float64)
    with pytest.raises(ValueError, match="calibrated already"):
        SummarySink(poisson=True)(dict(_shard("c", prob, start, end, label, 4), calibrated=True))


# ---- 5. end to end: the table tools on the written table ----------------------------------------------------------------------------------
R_LOCAL, R_DISTAL = 5, 250
RECORDS = {"chrA": "".join(np.random.default_rng(21).choice(list("ACGT"), size=5003)),
           "chr10": "".join(np.random.default_rng(22).choice(list("ACGT"), size=1203))}      # (file order; chr10 < chrA by name)


@pytest.fixture(scope="module")
def files(tmp_path_factory):
    d = tmp_path_factory.mktemp("summary")
    fa = d / "g.fa"
    fa.write_text("".join(f">{k}\n" + "\n".join(s[i:i + 60] for i in range(0, len(s), 60)) + "\n" for k, s in RECORDS.items()))
    return d, str(fa)


@pytest.fixture(scope="module")
def snv_model():
    from mural_amd.model import model_choice, weights_init
    ncol = 2 * R_LOCAL + 1 - 2
    config = dict(local_radius=R_LOCAL, local_order=3, local_hidden1_size=150, local_hidden2_size=75, distal_radius=R_DISTAL,
                  emb_dropout=0.1, local_dropout=0.1, CNN_kernel_size=3, CNN_out_channels=32, distal_fc_dropout=0.25, n_class=4,
                  model_no=2, seq_only=True, emb_dims=[(65, 2)] * ncol, segment_center=300000)
    common = dict(emb_dims=config["emb_dims"], n_class=4, n_cont=0, distal_order=1, in_channels=4)
    torch.manual_seed(5)
    model = model_choice(2, config, common, "snv")
    model.apply(weights_init)
    return model.cuda().eval(), config


def _forward(snv_model, fa, **kw):
    from mural_amd.predict import HipShardForward
    return HipShardForward(snv_model[0], fa, local_radius=R_LOCAL, local_order=3, **kw)


def _labelled_bed(path):
    """Every A/T site of the records in file order, labels 0 .. 3."""
    rng = np.random.default_rng(4)
    n = 0
    with open(path, "w") as fh:
        for c, s in RECORDS.items():
            for p, b in enumerate(s):
                if b in "AT":
                    fh.write(f"{c}\t{p}\t{p + 1}\t.\t{int(rng.integers(0, 4))}\t{'+' if b == 'A' else '-'}\n")
                    n += 1
    return str(path), n


def _check_against_the_table_tools(res, table, prefix, d):
    from mural_amd import tables
    total, n_sites = tables.prob_sum_file(table, 4)
    assert res["n_sites"] == n_sites
    print("prob_sum", res["prob_sum"], "table tool", total)
    assert abs(res["prob_sum"] - total) <= 5e-4 * res["prob_sum"]
    for W in (1000, 64):
        keys, tab = tables.regional_table(table, W, 4)
        got_keys, got = res["windows"][W]
        assert got_keys == keys and np.array_equal(got[:, :5], tab[:, :5])
        rel = np.abs(got[:, 5:] - tab[:, 5:]) / got[:, 5:]
        print("W", W, "windows", len(keys), "largest relative difference to the table tool", float(rel.max()))
        assert (rel <= 5e-4).all()
    args = types.SimpleNamespace(pred_file=table, window_size=1000, n_class=4, out_prefix=str(d / "tool"), ratio_cutoff=0.2)
    tables.run_regional_corr_calc(args)
    names = tables.regional_output_names(prefix, 1000)
    tool = tables.regional_output_names(str(d / "tool"), 1000)
    assert open(names[0]).readline() == open(tool[0]).readline()
    assert len(open(names[0]).readlines()) == len(open(tool[0]).readlines()) and os.path.exists(names[1])
    assert os.path.exists(tables.regional_output_names(prefix, 64)[0])


def test_tee_equals_the_table_tools_on_the_written_table(files, snv_model, monkeypatch):
    from mural_amd import predict as P
    d, fa = files
    monkeypatch.setattr(P, "_ALIGNED_PART_ROWS", 700)
    alone = str(d / "alone.tsv")
    n = P.predict_regions_sharded(_forward(snv_model, fa), list(RECORDS), "A", sink=P.TsvSink(alone), collect=False)
    summary = P.SummarySink(d / "reg", windows=(1000, 64))
    T = {}
    m = P.predict_regions_sharded(_forward(snv_model, fa), list(RECORDS), "A", sink=P.TeeSink(P.TsvSink(d / "tee.tsv"), summary),
                                  collect=False, timings=T)
    assert n == m > 1400 and T["aligned_shards"] == 2 and summary.rows == n
    assert open(d / "tee.tsv", "rb").read() == open(alone, "rb").read()
    _check_against_the_table_tools(summary.result(), str(d / "tee.tsv"), str(d / "reg"), d)
    # the BED driver, with labels
    bed, rows = _labelled_bed(d / "sites.bed")
    P.predict_bed_sharded(_forward(snv_model, fa), bed, sink=P.TsvSink(d / "bed_alone.tsv"), collect=False)
    summary = P.SummarySink(d / "bed", windows=(1000, 64))
    m = P.predict_bed_sharded(_forward(snv_model, fa), bed, sink=P.TeeSink(P.TsvSink(d / "bed_tee.tsv"), summary), collect=False)
    assert m == rows == n
    assert open(d / "bed_tee.tsv", "rb").read() == open(d / "bed_alone.tsv", "rb").read()
    res = summary.result()
    assert res["windows"][1000][1][:, 2:5].sum() > rows / 2      # the labels arrived
    _check_against_the_table_tools(res, str(d / "bed_tee.tsv"), str(d / "bed"), d)


# ---- 6. scaling round trip -------------------------------------------------------------------------------------------------------------------
def test_scaling_round_trip(files, snv_model, capsys):
    """Pass 1 yields the factor, pass 2 writes the scaled table; the file tool scales the ROUNDED table, so a cell may differ by one unit of
    its fourth digit.  The factor is 0.01 (genomewide_mu is chosen for it): a power of ten moves no digit of prob1.., so the file tool's own
    double rounding shows in prob0 = 1 - sum alone, whose unit (1e-4) is ~100 times the error it inherits from three rounded terms of ~0.003
    (<= 3 * 5e-7): about 1 % of the rows, 0.3 % of the cells."""
    from mural_amd import predict as P
    from mural_amd import tables
    d, fa = files
    summary = P.SummarySink()
    P.predict_regions_sharded(_forward(snv_model, fa), "chrA", "A", sink=P.TeeSink(P.TsvSink(d / "plain.tsv"), summary), collect=False)
    res = summary.result()
    mu = 0.01 * res["prob_sum"] / (res["n_sites"] * 0.3)
    factor = summary.scaling_factor(mu, 0.3)
    printed = capsys.readouterr().out
    assert abs(factor - 0.01) < 1e-15 and "n_sites: %d" % res["n_sites"] in printed and "scaling factor: 1.000e-02" in printed
    P.predict_regions_sharded(_forward(snv_model, fa, scale_factor=factor), "chrA", "A", sink=P.TsvSink(d / "scaled.tsv"), collect=False)
    tables.apply_scaling_file(d / "plain.tsv", factor, 4, d / "by_tool.tsv")
    a, b = (np.loadtxt(d / f, skiprows=1, usecols=(5, 6, 7, 8)) for f in ("scaled.tsv", "by_tool.tsv"))
    assert a.shape == b.shape and a.shape[0] == res["n_sites"]
    unit = 10.0 ** (np.floor(np.log10(np.maximum(np.abs(a), np.abs(b)))) - 3)
    differ = a != b
    print("cells that differ", int(differ.sum()), "of", a.size)
    assert (np.abs(a - b) <= unit * (1 + 1e-9)).all()
    assert differ.sum() < 0.05 * a.size
    assert [ln.split("\t")[:5] for ln in open(d / "scaled.tsv")] == [ln.split("\t")[:5] for ln in open(d / "by_tool.tsv")]
