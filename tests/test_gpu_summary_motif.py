"""Motif rate tables on the device (csrc/summary_kmer.hip: mural_summary_motif_rows; mural_amd.predict.SummarySink(motifs=...);
mural_amd.tables.motif_table): the kernel's integer tables and first-appearance words against the numpy twin cell by cell, bit for bit
across splits into parts, the LDS rule, the status bits, the table route against the reference's recorded output, and end to end the
sink against ``tables.motif_table`` on the table the same run wrote."""
import ctypes as C
import importlib.util
import os

import numpy as np
import pytest
import torch

from tests import _motif_data as D
from tests.test_gpu_summary import RECORDS, _forward, _labelled_bed, files, snv_model  # noqa: F401  (the file fixtures of the summary tests)

pytestmark = pytest.mark.gpu


def _dev():
    return torch.device("cuda", torch.cuda.current_device())


def _kernel(genome, cols, n_class, motifs, indel=False, order_base=0, by_row=False, into=None):
    """One mural_summary_motif_rows call on device copies of the arrays: ({m: (table [4^m][3][n_class], first)}, status)."""
    from mural_amd import _lib
    lib = _lib.lib()
    dev = _dev()
    prob, start, end, label = cols
    up = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)      # noqa: E731
    prob_d, start_d, end_d, label_d = up(prob), up(start), up(end), up(label)
    g = genome.as_struct(dev)
    s = _lib.MuralSummaryMotifRows()
    s.genome = C.pointer(g)
    s.prob, s.prob_f64, s.prob_stride = prob_d.data_ptr(), int(prob.dtype == np.float64), prob_d.stride(0)
    s.start, s.end, s.label, s.label_kind = start_d.data_ptr(), end_d.data_ptr(), label_d.data_ptr(), 2
    s.n, s.n_class, s.n_m, s.indel, s.order_by_row, s.order_base = len(start), n_class, len(motifs), int(indel), int(by_row), order_base
    tabs = into or {m: (torch.zeros(4 ** m * 3 * n_class, dtype=torch.int64, device=dev), torch.full((4 ** m,), -1, dtype=torch.int64, device=dev))
                    for m in motifs}
    status = torch.zeros(1, dtype=torch.int32, device=dev)
    for j, m in enumerate(motifs):
        s.m[j], s.table[j], s.first[j] = m, tabs[m][0].data_ptr(), tabs[m][1].data_ptr()
    s.status = status.data_ptr()
    _lib.check(lib.mural_summary_motif_rows(C.byref(s), _lib.current_stream_ptr(dev)))
    return tabs, int(status.item())


def _host(tabs, n_class):
    return {m: (t.cpu().numpy().view(np.uint64).reshape(4 ** m, 3, n_class), f.cpu().numpy().view(np.uint64)) for m, (t, f) in tabs.items()}


@pytest.fixture(scope="module")
def genomes():
    from mural_amd.data.genome import PackedGenome
    return {name: PackedGenome.from_sequence(seq, _dev()) for name, seq in D.SEQS.items()}


# ---- 1. the kernel against the numpy twin, every cell and every word ------------------------------------------------------------------
def test_the_lds_cut_is_the_160_kib_of_a_workgroup():
    """4^m keys x (3 n_class + 1) cells of 8 bytes in LDS where that fits 160 KiB, global memory otherwise; no table for a refused m."""
    from mural_amd import _lib
    lib = _lib.lib()
    for n_class in range(1, 9):
        for m in range(0, 17):
            want = int(m % 2 == 1 and 3 <= m <= 15 and 4 ** m * (3 * n_class + 1) * 8 <= 160 * 1024)
            assert lib.mural_summary_motif_in_lds(m, n_class) == want, (m, n_class)
    got = {nc: [lib.mural_summary_motif_in_lds(m, nc) for m in (3, 5, 7)] for nc in (4, 8)}
    assert got == {4: [1, 1, 0], 8: [1, 0, 0]}      # m = 7 adds to global memory; m = 5 too at 8 classes


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
@pytest.mark.parametrize("name", list(D.CASES))
def test_kernel_equals_the_numpy_twin_in_every_cell_and_word(genomes, name, dtype):
    """SNV at 4 classes (m = 3, 5 in LDS, 7 in global memory) and INDEL at 8 (m = 3 in LDS, 5 and 7 in global memory), both
    chromosomes into one set of tables, the second with its ordinal above the words."""
    from mural_amd.predict import summary_motif_host
    c = D.case(name)
    nc, indel = c["n_class"], c["model_type"] == "indel"
    got, want = None, {}
    for ordinal, (chrom, (prob, start, end, label)) in enumerate(c["rows"].items()):
        prob = prob.astype(dtype)
        if chrom == "chrM2":
            for j, v in enumerate(D.TINY):
                prob[1000 + j, 1 + j % 3] = v
        got, status = _kernel(genomes[chrom], (prob, start, end, label), nc, D.MOTIFS, indel, order_base=ordinal << 39, into=got)
        assert status == 0
        _, status = summary_motif_host(D.SEQS[chrom], prob, start, end, label, nc, D.MOTIFS, indel, order_base=ordinal << 39, into=want)
        assert status == 0
    got = _host(got, nc)
    for m in D.MOTIFS:
        assert want[m][0][:, 0].sum() > (m - indel) * (1 - D.NO_WINDOW_CAP) * 0.9 * sum(len(v[1]) for v in c["rows"].values())      # (not empty)
        assert np.array_equal(got[m][0], want[m][0]), m
        assert np.array_equal(got[m][1], want[m][1]), m


def test_nine_bases_and_the_order_by_row(genomes):
    """m = 9 (the largest the issue names) beside m = 3, the words counting rows, not starts."""
    from mural_amd.predict import summary_motif_host
    prob, start, end, label = D.case("snv")["rows"]["chrM2"]
    perm = np.random.default_rng(5).permutation(len(start))
    cols = (prob[perm], start[perm], end[perm], label[perm])
    got, status = _kernel(genomes["chrM2"], cols, 4, (9, 3), order_base=12345, by_row=True)
    want, _ = summary_motif_host(D.SEQS["chrM2"], *cols, 4, (9, 3), order_base=12345, order_by_row=True)
    got = _host(got, 4)
    assert status == 0
    for m in (9, 3):
        assert np.array_equal(got[m][0], want[m][0]) and np.array_equal(got[m][1], want[m][1]), m


# ---- 2. parts ---------------------------------------------------------------------------------------------------------------------------
def _shard(name, cols, k, rows=slice(None), aligned=True):
    prob, start, end, label = cols
    up = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(_dev())      # noqa: E731
    shard = {"chrom": name, "start": up(start[rows]), "end": up(end[rows]), "strand": up(np.zeros(len(start), np.uint8)[rows]),
             "label": up(label[rows]), "prob": up(prob)[rows], "n_class": k, "calibrated": False}
    if aligned:
        shard["aligned"] = True
    return shard


def test_one_part_seven_parts_and_shuffled_parts_are_bit_identical(genomes):
    from mural_amd.predict import SummarySink, summary_motif_host
    cols = D.case("snv")["rows"]["chrM2"]
    n = len(cols[1])
    want, _ = summary_motif_host(D.SEQS["chrM2"], *cols, 4, D.MOTIFS)
    cuts7 = [0, 1, 64, 129, 700, 1300, n - 1, n]      # a one-row part first and last
    seven = list(zip(cuts7[:-1], cuts7[1:]))
    shuffled = [seven[i] for i in np.random.default_rng(2).permutation(7)]
    results = []
    for parts in ([(0, n)], seven, shuffled):
        sink = SummarySink(motifs=D.MOTIFS, genome=lambda name: genomes[name])
        for a, b in parts:
            sink(_shard("chrM2", cols, 4, slice(a, b)))
        sink.close()
        sums = sink.motif_sums()
        for m in D.MOTIFS:
            assert np.array_equal(sums[m][0], want[m][0]) and np.array_equal(sums[m][1], want[m][1]), m
        results.append({m: (t.tobytes(), f.tobytes(), sink.result()["motifs"][m][0], sink.result()["motifs"][m][1].tobytes())
                        for m, (t, f) in sums.items()})
    assert results[0] == results[1] == results[2]
    perm = np.random.default_rng(3).permutation(n)      # a gathered shard (not aligned) is sorted first; the rows are the same set
    sink = SummarySink(motifs=D.MOTIFS, kmers=(3,), windows=(1000,), genome=lambda name: genomes[name])
    sink(_shard("chrM2", [c[perm] for c in cols], 4, aligned=False))
    sink.close()
    assert all(sink.motif_sums()[m][0].tobytes() == results[0][m][0] and sink.motif_sums()[m][1].tobytes() == results[0][m][1]
               for m in D.MOTIFS)
    assert set(sink.result()) == {"prob_sum", "n_sites", "windows", "kmers", "motifs"}


# ---- 3. status --------------------------------------------------------------------------------------------------------------------------
BAD = {"label": (2, "mut_type outside"), "start": (1, "negative start"), "nan": (8, "NaN, negative or above 1"),
       "above": (8, "NaN, negative or above 1")}


def _spoil(cols, what, row=40):
    prob, start, end, label = [c.copy() for c in cols]
    if what == "label":
        label[row] = 4
    elif what == "start":
        start[row] = -3
    elif what == "nan":
        prob[row, 2] = np.nan
    else:
        prob[row, 1] = np.nextafter(1.0, 2.0)
    return prob, start, end, label


@pytest.mark.parametrize("what", list(BAD))
def test_bad_rows_set_their_bit_stay_out_and_close_raises(genomes, tmp_path, what):
    from mural_amd.predict import SummarySink, TeeSink, TsvSink
    cols = [c[:300] for c in D.case("snv")["rows"]["chrM2"]]
    keep = np.arange(300) != 40
    clean, status = _kernel(genomes["chrM2"], [c[keep] for c in cols], 4, D.MOTIFS)
    assert status == 0
    got, status = _kernel(genomes["chrM2"], _spoil(cols, what), 4, D.MOTIFS)
    assert status == BAD[what][0]
    clean, got = _host(clean, 4), _host(got, 4)
    for m in D.MOTIFS:                 # left out of every table, the LDS ones and the global one
        assert np.array_equal(got[m][0], clean[m][0]) and np.array_equal(got[m][1], clean[m][1]), m
    for tee in (False, True):
        summary = SummarySink(tmp_path / "s", motifs=(3, 7), genome=lambda name: genomes[name])
        sink = TeeSink(TsvSink(tmp_path / "t.tsv"), summary) if tee else summary
        sink(_shard("chrM2", _spoil(cols, what), 4))
        with pytest.raises(ValueError, match=BAD[what][1]):
            sink.close()
        sink.abort()
        assert os.listdir(tmp_path) == []


# ---- 4. the table route against the reference's recorded output -------------------------------------------------------------------------
@pytest.mark.parametrize("name,m,gz", [("snv", 3, False), ("snv", 5, True), ("snv", 7, False), ("indel", 3, True), ("indel", 5, False),
                                       ("indel", 7, False)])
def test_motif_table_matches_the_reference(tmp_path, name, m, gz):
    """``tables.run_motif_corr_calc`` on the case's table, plain or gzip, in chunks of a few hundred rows: names, order and counts as the
    reference wrote them, rates within 1e-12 relative, the correlation lines as tests/test_gpu_tables.py compares them."""
    import types
    from mural_amd import tables
    nc = D.CASES[name]["n_class"]
    table, fasta = D.write_case(str(tmp_path), name, gz)
    args = types.SimpleNamespace(pred_file=table, ref_genome=fasta, out_prefix=str(tmp_path / "o"), motif_length=m, n_class=nc, strand="-")
    tables.run_motif_corr_calc(args, D.CASES[name]["model_type"], chunk_bytes=20000)
    names, obs, pred, counts, corr_lines = D.golden(name, m)
    rates_path, corr_path = tables.motif_output_names(str(tmp_path / "o"), m)
    rows = [ln.split("\t") for ln in open(rates_path).read().split("\n")[1:] if ln]
    assert [r[0] for r in rows] == names
    assert np.array_equal(np.array([[int(v) for v in r[2 * nc - 1:]] for r in rows]), counts)
    got = np.array([[float(v) for v in r[1:2 * nc - 1]] for r in rows])
    want = np.concatenate([obs, pred], axis=1)
    assert (np.abs(got - want) <= 1e-12 * np.abs(want)).all()
    got_lines = open(corr_path).read().split("\n")[:-1]
    assert len(got_lines) == len(corr_lines)
    for g, w in zip(got_lines, corr_lines):
        g, w = g.split("\t"), w.split("\t")
        assert g[:3] == w[:3]
        assert float(g[3]) == float(w[3]) or abs(float(g[3]) - float(w[3])) <= 1e-9 * abs(float(w[3]))


# ---- 5. end to end: tables.motif_table on the table the same run wrote ----------------------------------------------------------------
def _check_against_motif_table(res, table, fa):
    from mural_amd import tables
    for m in (3, 5):
        names, tab = tables.motif_table(table, fa, m, 4, "snv")
        got_names, got = res["motifs"][m]
        assert got_names == names and np.array_equal(got[:, :5], tab[:, :5]), m
        rel = np.abs(got[:, 5:] - tab[:, 5:]) / got[:, 5:]
        print("m", m, "motifs", len(names), "largest relative difference to the table route", float(rel.max()))
        assert (rel <= 5e-4).all()


def test_tee_equals_motif_table_on_the_written_table_and_no_table_gives_the_same(files, snv_model, monkeypatch):
    from mural_amd import predict as P
    d, fa = files
    monkeypatch.setattr(P, "_ALIGNED_PART_ROWS", 700)      # several parts per chromosome
    forward = _forward(snv_model, fa)
    summary = P.SummarySink(d / "mreg", motifs=(3, 5), genome=forward.genome)
    n = P.predict_regions_sharded(forward, list(RECORDS), "A", sink=P.TeeSink(P.TsvSink(d / "mtee.tsv"), summary), collect=False)
    assert n > 1400 and summary.rows == n and set(summary.result()) == {"prob_sum", "n_sites", "windows", "motifs"}
    _check_against_motif_table(summary.result(), str(d / "mtee.tsv"), fa)
    assert os.path.exists(d / "mreg.3-motif.mut_rates.tsv") and os.path.exists(d / "mreg.5-motif.corr.txt")
    alone = P.SummarySink(motifs=(3, 5), genome=(forward := _forward(snv_model, fa)).genome)      # no table at all
    assert P.predict_regions_sharded(forward, list(RECORDS), "A", sink=alone, collect=False) == n
    for m in (3, 5):
        assert alone.result()["motifs"][m][0] == summary.result()["motifs"][m][0]
        assert all(np.array_equal(a, b) for a, b in zip(alone.motif_sums()[m], summary.motif_sums()[m]))
    # the BED driver, with labels
    bed, rows = _labelled_bed(d / "msites.bed")
    forward = _forward(snv_model, fa)
    summary = P.SummarySink(motifs=(3, 5), genome=forward.genome)
    assert P.predict_bed_sharded(forward, bed, sink=P.TeeSink(P.TsvSink(d / "mbed_tee.tsv"), summary), collect=False) == rows
    assert summary.result()["motifs"][3][1][:, 2:5].sum() > rows / 2      # the labels arrived
    _check_against_motif_table(summary.result(), str(d / "mbed_tee.tsv"), fa)


# ---- 6. command line --------------------------------------------------------------------------------------------------------------------
def test_command_line_writes_the_motif_files_and_no_table(files, snv_model, tmp_path):
    from mural_amd import tables
    from mural_amd.model import nn_utils
    d, fa = files
    ckpt = str(tmp_path / "model")
    nn_utils.save_model(snv_model[0], None, snv_model[1], ckpt)
    before = set(os.listdir(tmp_path))
    spec = importlib.util.spec_from_file_location("predict_files", os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))),
                                                                                  "tools", "predict_files.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    prefix = str(tmp_path / "P")
    mod.main([ckpt, fa, "--regions", "chrA:1-3000", "--regions", "chr10", "--no-table", "--summary", prefix, "--motif_length", "3", "5"])
    want = {os.path.basename(p) for m in (3, 5) for p in tables.motif_output_names(prefix, m)}
    assert set(os.listdir(tmp_path)) - before == want and len(want) == 4
    assert open(tables.motif_output_names(prefix, 3)[1]).readline().startswith("3-moitf\t1\t")
    with pytest.raises(SystemExit, match="--motif_length needs --summary"):
        mod.main([ckpt, fa, "--regions", "chr10", str(tmp_path / "t.tsv"), "--motif_length", "3"])
    with pytest.raises(SystemExit, match="--motif_length"):
        mod.main([ckpt, fa, "--regions", "chr10", "--no-table", "--summary", prefix, "--motif_length", "4"])
