"""k-mer rate tables in flight (csrc/summary_kmer.hip, mural_amd.predict.SummarySink(kmers=...)): the kernel's integer tables against
the numpy twin cell by cell, bit for bit across splits into parts, the status bits, and end to end against ``tables.kmer_table`` on the
table the same run wrote."""
import ctypes as C
import importlib.util
import os
import types

import numpy as np
import pytest
import torch

from tests import _summary_kmer_data as D
from tests.test_gpu_summary import RECORDS, _forward, _labelled_bed, files, snv_model  # noqa: F401  (the file fixtures of the summary tests)

pytestmark = pytest.mark.gpu

MODES = [(False, 0), (True, 1), (True, 2), (True, 3)]      # SNV rows by their own strand; INDEL rows '+', '-', both
NEVER = np.uint64(2 ** 64 - 1)


def _dev():
    return torch.device("cuda", torch.cuda.current_device())


def _kernel(genome, cols, n_class, kmers, indel=False, mode=0, order_base=0, label_dtype=np.float32):
    """One mural_summary_kmer_rows call on device copies of the arrays: ({k: (table [4^k][3][n_class], first)}, status)."""
    from mural_amd import _lib
    lib = _lib.lib()
    dev = _dev()
    prob, start, end, strand, label = cols
    up = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)      # noqa: E731
    prob_d, start_d, end_d, strand_d, label_d = up(prob), up(start), up(end), up(strand), up(label.astype(label_dtype))
    g = genome.as_struct(dev)
    s = _lib.MuralSummaryKmerRows()
    s.genome = C.pointer(g)
    s.prob, s.prob_f64, s.prob_stride = prob_d.data_ptr(), int(prob.dtype == np.float64), prob_d.stride(0)
    s.start, s.end, s.strand, s.label = start_d.data_ptr(), end_d.data_ptr(), strand_d.data_ptr(), label_d.data_ptr()
    s.label_kind = {np.float32: 0, np.int32: 1, np.int64: 2}[label_dtype]
    s.n, s.n_class, s.n_k, s.indel, s.mode, s.order_base = len(start), n_class, len(kmers), int(indel), mode, order_base
    tabs = {k: (torch.zeros(4 ** k * 3 * n_class, dtype=torch.int64, device=dev), torch.full((4 ** k,), -1, dtype=torch.int64, device=dev))
            for k in kmers}
    status = torch.zeros(1, dtype=torch.int32, device=dev)
    for j, k in enumerate(kmers):
        s.k[j], s.table[j], s.first[j] = k, tabs[k][0].data_ptr(), tabs[k][1].data_ptr()
    s.status = status.data_ptr()
    _lib.check(lib.mural_summary_kmer_rows(C.byref(s), _lib.current_stream_ptr(dev)))
    return ({k: (t.cpu().numpy().view(np.uint64).reshape(4 ** k, 3, n_class), f.cpu().numpy().view(np.uint64)) for k, (t, f) in tabs.items()},
            int(status.item()))


@pytest.fixture(scope="module")
def genome():
    from mural_amd.data.genome import PackedGenome
    return PackedGenome.from_sequence(D.SEQ, _dev())


# ---- 1. the kernel against the numpy twin, every cell -----------------------------------------------------------------------------------
def test_the_lds_cut_is_the_160_kib_of_a_workgroup():
    """4^k keys x (3 n_class + 1) cells of 8 bytes in LDS where that fits 160 KiB, global memory otherwise."""
    from mural_amd import _lib
    lib = _lib.lib()
    for n_class in range(1, 9):
        for k in range(1, 11):
            assert lib.mural_summary_kmer_in_lds(k, n_class) == int(4 ** k * (3 * n_class + 1) * 8 <= 160 * 1024), (k, n_class)
    got = {nc: [lib.mural_summary_kmer_in_lds(k, nc) for k in D.KMERS] for nc in (2, 4, 8)}
    assert got == {2: [1, 1, 1, 0], 4: [1, 1, 1, 0], 8: [1, 1, 0, 0]}      # k = 7 always adds to global memory; k = 5 too at 8 classes


@pytest.mark.parametrize("indel,mode", MODES)
@pytest.mark.parametrize("dtype", [np.float32, np.float64])
@pytest.mark.parametrize("n_class", [2, 4, 8])
def test_kernel_equals_the_numpy_twin_in_every_cell(genome, n_class, dtype, indel, mode):
    from mural_amd.predict import summary_kmer_host
    for n, kind in D.CASES:
        cols = D.case(n, kind, n_class, dtype, indel)
        got, status = _kernel(genome, cols, n_class, D.KMERS, indel, mode, order_base=3 << 40)
        want, _ = summary_kmer_host(D.SEQ, *cols, n_class, D.KMERS, indel, mode, order_base=3 << 40)
        assert status == 0
        for k in D.KMERS:
            assert np.array_equal(got[k][0], want[k][0]), (n, kind, k)
            assert np.array_equal(got[k][1], want[k][1]), (n, kind, k)


def test_key_rule_is_the_table_tools(genome):
    """mural_table_kmer_keys (tables.kmer_table's keys) on the same rows: the twin's keys, hence the kernel's."""
    from mural_amd import _lib
    from mural_amd.predict import kmer_keys_host
    dev = _dev()
    for indel, mode in MODES:
        _, start, end, strand, _ = D.rows(2049, 4, np.float32, indel)
        up = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)      # noqa: E731
        start_d, end_d, strand_d = up(start), up(end), up(strand)
        g = genome.as_struct(dev)
        for k in D.KMERS + (10,):
            a, b = torch.full((2049,), -7, dtype=torch.int32, device=dev), torch.full((2049,), -1, dtype=torch.int32, device=dev)
            _lib.check(_lib.lib().mural_table_kmer_keys(C.byref(g), start_d.data_ptr(), end_d.data_ptr(), strand_d.data_ptr(), 2049, k,
                                                       int(indel), mode, a.data_ptr(), b.data_ptr(), _lib.current_stream_ptr(dev)))
            want = kmer_keys_host(D.SEQ, start, end, strand, k, indel, mode)
            assert np.array_equal(a.cpu().numpy(), want[0]) and np.array_equal(b.cpu().numpy(), want[1]), (mode, k)


def test_integer_labels(genome):
    cols = D.rows(65, 4, np.float32)
    want = _kernel(genome, cols, 4, (3,))
    for dt in (np.int32, np.int64):
        got = _kernel(genome, cols, 4, (3,), label_dtype=dt)
        assert got[1] == 0 and np.array_equal(got[0][3][0], want[0][3][0])


# ---- 2. parts ---------------------------------------------------------------------------------------------------------------------------
def _shard(name, cols, k, rows=slice(None), aligned=True):
    prob, start, end, strand, label = cols
    up = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(_dev())      # noqa: E731
    shard = {"chrom": name, "start": up(start[rows]), "end": up(end[rows]), "strand": up(strand[rows]), "label": up(label[rows]),
             "prob": up(prob)[rows], "n_class": k, "calibrated": False}
    if aligned:
        shard["aligned"] = True
    return shard


def test_one_part_seven_parts_and_shuffled_parts_are_bit_identical(genome):
    from mural_amd.predict import SummarySink, summary_kmer_host
    n, k = 2049, 4
    cols = D.rows(n, k, np.float32)
    want, _ = summary_kmer_host(D.SEQ, *cols, k, D.KMERS)
    cuts7 = [0, 1, 64, 129, 700, 1300, 2048, n]      # a one-row part first and last
    seven = list(zip(cuts7[:-1], cuts7[1:]))
    shuffled = [seven[i] for i in np.random.default_rng(2).permutation(7)]
    results = []
    for parts in ([(0, n)], seven, shuffled):
        sink = SummarySink(kmers=D.KMERS, genome=lambda name: genome)
        for a, b in parts:
            sink(_shard("chrK", cols, k, slice(a, b)))
        sink.close()
        sums = sink.kmer_sums()
        for kk in D.KMERS:
            assert np.array_equal(sums[kk][0], want[kk][0]) and np.array_equal(sums[kk][1], want[kk][1]), kk
        results.append({kk: (t.tobytes(), f.tobytes(), sink.result()["kmers"][kk][0], sink.result()["kmers"][kk][1].tobytes())
                        for kk, (t, f) in sums.items()})
    assert results[0] == results[1] == results[2]
    # a gathered shard (not aligned) is sorted first; the rows are the same set
    perm = np.random.default_rng(3).permutation(n)
    sink = SummarySink(kmers=D.KMERS, genome=lambda name: genome)
    sink(_shard("chrK", [c[perm] for c in cols], k, aligned=False))
    sink.close()
    assert all(sink.kmer_sums()[kk][0].tobytes() == results[0][kk][0] and sink.kmer_sums()[kk][1].tobytes() == results[0][kk][1]
               for kk in D.KMERS)


# ---- 3. status --------------------------------------------------------------------------------------------------------------------------
BAD = {"label": (2, "mut_type outside"), "start": (1, "negative start"), "nan": (8, "NaN, negative or above 1"),
       "above": (8, "NaN, negative or above 1")}


def _spoil(cols, what, row=40):
    prob, start, end, strand, label = [c.copy() for c in cols]
    if what == "label":
        label[row] = 4
    elif what == "start":
        start[row] = -3
    elif what == "nan":
        prob[row, 2] = np.nan
    else:
        prob[row, 1] = np.nextafter(np.float32(1), np.float32(2))
    return prob, start, end, strand, label


@pytest.mark.parametrize("what", list(BAD))
def test_bad_rows_set_their_bit_stay_out_and_close_raises(genome, tmp_path, what):
    from mural_amd.predict import SummarySink, TeeSink, TsvSink
    cols = D.rows(300, 4, np.float32)
    keep = np.arange(300) != 40
    clean, status = _kernel(genome, [c[keep] for c in cols], 4, D.KMERS)
    assert status == 0
    got, status = _kernel(genome, _spoil(cols, what), 4, D.KMERS)
    assert status == BAD[what][0]
    for k in D.KMERS:                  # left out of every table, the LDS ones and the global one
        assert np.array_equal(got[k][0], clean[k][0]) and np.array_equal(got[k][1], clean[k][1]), k
    for tee in (False, True):
        summary = SummarySink(tmp_path / "s", kmers=(3, 7), genome=lambda name: genome)
        sink = TeeSink(TsvSink(tmp_path / "t.tsv"), summary) if tee else summary
        sink(_shard("chrB", _spoil(cols, what), 4))
        with pytest.raises(ValueError, match=BAD[what][1]):
            sink.close()
        sink.abort()
        assert os.listdir(tmp_path) == []


# ---- 4. two chromosomes: the part that is reduced after the forward has moved on ------------------------------------------------------
class OneResident:
    """Keeps one packed chromosome, like HipShardForward.genome: asking for another drops the one before."""

    def __init__(self, sequences):
        self.sequences, self.resident, self.packs = sequences, (None, None), 0

    def __call__(self, name):
        from mural_amd.data.genome import PackedGenome
        if self.resident[0] != name:
            self.resident = (None, None)
            self.resident = (name, PackedGenome.from_sequence(self.sequences[name], _dev()))
            self.packs += 1
        return self.resident[1]


def test_two_chromosomes_keep_the_right_genome(tmp_path):
    from mural_amd import tables
    from mural_amd.predict import SummarySink, _kmer_collapse, _kmer_fold, kmer_table_from_sums, summary_kmer_host
    seqs = {"chrK": D.SEQ, "chr2": D.SEQ[::-1]}      # chrK arrives first, chr2 sorts first
    k_cols, two_cols = D.rows(2049, 4, np.float64), D.at_sites(4, np.float64)
    resident = OneResident(seqs)
    sink = SummarySink(tmp_path / "two", windows=(1000,), kmers=(3, 5, 7), genome=resident)
    for a, b in ((0, 900), (900, 2049)):
        sink(_shard("chrK", k_cols, 4, slice(a, b)))
    held = sink._pending["genome"]
    assert held is resident.resident[1] and held.length == D.L
    sink(_shard("chr2", two_cols, 4))                # chrK's last part is reduced (its windows) now, chr2 being the resident one
    assert resident.resident[0] == "chr2" and resident.packs == 2
    sink.close()
    a, _ = summary_kmer_host(seqs["chr2"], *two_cols, 4, (3, 5, 7))
    b, _ = summary_kmer_host(seqs["chrK"], *k_cols, 4, (3, 5, 7))
    for k in (3, 5, 7):
        _, want = _kmer_collapse({k: _kmer_fold(a[k][0] + b[k][0])}, {"chr2": {k: a[k][1]}, "chrK": {k: b[k][1]}})
        got = sink.kmer_sums()[k]
        assert np.array_equal(got[0], want[k][0]) and np.array_equal(got[1], want[k][1])
        names, table = kmer_table_from_sums(*want[k], k, 4)
        assert sink.result()["kmers"][k][0] == names and np.array_equal(sink.result()["kmers"][k][1], table)
        assert [ln.split("\t")[0] for ln in open(tables.kmer_output_names(tmp_path / "two", k)[0])][1:] == names
    assert sink.result()["windows"][1000][1][:, 0].sum() == 2049 + len(two_cols[1])


# ---- 5. end to end: tables.kmer_table on the table the same run wrote --------------------------------------------------------------
def _check_against_kmer_table(res, table, fa, prefix, d):
    from mural_amd import tables
    for k in (3, 5, 7):
        names, tab = tables.kmer_table(table, fa, k, 4, "snv")
        got_names, got = res["kmers"][k]
        assert got_names == names and np.array_equal(got[:, :5], tab[:, :5]), k
        rel = np.abs(got[:, 5:] - tab[:, 5:]) / got[:, 5:]
        print("k", k, "k-mers", len(names), "largest relative difference to the table tool", float(rel.max()))
        assert (rel <= 5e-4).all()
        args = types.SimpleNamespace(pred_file=table, ref_genome=fa, kmer_length=k, n_class=4, out_prefix=str(d / "tool"), strand=None)
        tables.run_kmer_corr_calc(args, "snv")
        mine, tool = (open(tables.kmer_output_names(p, k)[0]).read().split("\n") for p in (prefix, str(d / "tool")))
        assert mine[0] == tool[0] and len(mine) == len(tool)
        cols = [0] + list(range(7, 11))            # the k-mer, number_of_mut1 .. 3, number_of_all
        assert [[ln.split("\t")[c] for c in cols] for ln in mine[1:-1]] == [[ln.split("\t")[c] for c in cols] for ln in tool[1:-1]]
        assert os.path.exists(tables.kmer_output_names(prefix, k)[1])


def test_tee_equals_kmer_table_on_the_written_table(files, snv_model, monkeypatch):
    from mural_amd import predict as P
    d, fa = files
    monkeypatch.setattr(P, "_ALIGNED_PART_ROWS", 700)      # several parts per chromosome
    forward = _forward(snv_model, fa)
    summary = P.SummarySink(d / "kreg", kmers=(3, 5, 7), genome=forward.genome)
    n = P.predict_regions_sharded(forward, list(RECORDS), "A", sink=P.TeeSink(P.TsvSink(d / "ktee.tsv"), summary), collect=False)
    assert n > 1400 and summary.rows == n and set(summary.result()) == {"prob_sum", "n_sites", "windows", "kmers"}
    _check_against_kmer_table(summary.result(), str(d / "ktee.tsv"), fa, str(d / "kreg"), d)
    # the BED driver, with labels, and the window tables beside the k-mer tables
    bed, rows = _labelled_bed(d / "ksites.bed")
    forward = _forward(snv_model, fa)
    summary = P.SummarySink(d / "kbed", windows=(1000,), kmers=(3, 5, 7), genome=forward.genome)
    m = P.predict_bed_sharded(forward, bed, sink=P.TeeSink(P.TsvSink(d / "kbed_tee.tsv"), summary), collect=False)
    assert m == rows == n
    res = summary.result()
    assert res["kmers"][3][1][:, 2:5].sum() > rows / 2      # the labels arrived
    _check_against_kmer_table(res, str(d / "kbed_tee.tsv"), fa, str(d / "kbed"), d)
    plain = P.SummarySink(windows=(1000,))
    P.predict_bed_sharded(_forward(snv_model, fa), bed, sink=plain, collect=False)
    assert np.array_equal(plain.result()["windows"][1000][1], res["windows"][1000][1])      # the window tables do not notice


# ---- 6. command line --------------------------------------------------------------------------------------------------------------------
def test_command_line_writes_the_four_files_and_no_table(files, snv_model, tmp_path):
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
    mod.main([ckpt, fa, "--regions", "chrA:1-3000", "--regions", "chr10", "--no-table", "--summary", prefix, "--kmer_length", "3",
              "--kmer_length", "7"])
    want = {os.path.basename(p) for k in (3, 7) for p in tables.kmer_output_names(prefix, k)}
    assert set(os.listdir(tmp_path)) - before == want and len(want) == 4
    assert len(open(tables.kmer_output_names(prefix, 3)[0]).readlines()) == 1 + 16      # A in the middle, T sites complemented to it
    with pytest.raises(SystemExit, match="--kmer_length needs --summary"):
        mod.main([ckpt, fa, "--regions", "chr10", str(tmp_path / "t.tsv"), "--kmer_length", "3"])
    with pytest.raises(SystemExit, match="--kmer_length"):
        mod.main([ckpt, fa, "--regions", "chr10", "--no-table", "--summary", prefix, "--kmer_length", "11"])
    with pytest.raises(SystemExit, match="strand"):
        mod.main([ckpt, fa, "--regions", "chr10", "--no-table", "--summary", prefix, "--kmer_length", "3", "--strand", "both"])
