"""Structure tables on the device (csrc/summary_txstruct.hip: mural_summary_txstruct_rows; mural_amd.predict.SummarySink(transcripts=...,
transcript_structure=True); mural_amd.tables.structure_table): every case goes through the entry point and is compared for EQUALITY with
the numpy twin ``summary_txstruct_host`` -- the record of tests/_txstruct_data.py in both probability types and the three label kinds,
the three loop bounds of the entry read from its getters, the carry of lo into hi, the status bits, calls that launch nothing,
additivity over calls, every refusal, and the sink's routes: a single-focal regions run, a model-set run, the table route and the command
line."""
import ctypes as C
import importlib.util
import io
import os

import numpy as np
import pytest
import torch

from tests import _conseq_data as D
from tests import _txstruct_data as S
from tests.test_gpu_model_set import files as set_files, models as set_models  # noqa: F401  (fixtures)
from tests.test_gpu_region_labels import REGIONS, _forward, files, snv_model  # noqa: F401  (fixtures)
from tests.test_gpu_summary_conseq import _Keep, _dev, _genome, _lib, _transcripts_over, _up

pytestmark = pytest.mark.gpu

LABEL_DTYPES = {0: np.float32, 1: np.int32, 2: np.int64}


def _acc(n_tx, fill=0):
    dev = _dev()
    return dict(table=torch.full((max(n_tx, 1) * 27,), fill, dtype=torch.int64, device=dev),
                rows=torch.full((max(n_tx, 1) * 2,), fill, dtype=torch.int64, device=dev),
                status=torch.zeros(1, dtype=torch.int32, device=dev), features={}, ws=None, conseq=dict(segments={}))


def _kernel(genome, prob, start, strand, label, segments, features, n_tx, aa=None, alt_order=None, into=None, pad=0):
    """One mural_summary_txstruct_rows call on device copies of the arrays: (accumulators, status)."""
    from mural_amd import tables
    from mural_amd.summaries import txstruct_rows_device
    dev = _dev()
    if pad:
        prob = np.concatenate([prob, np.full((len(prob), pad), 0.25, prob.dtype)], axis=1)
    prob_d, start_d, label_d = _up(prob), _up(start), _up(label)
    strand_d = None if strand is None else _up(strand)
    acc = into or _acc(n_tx)
    n = int(start_d.shape[0])
    txstruct_rows_device(acc, acc["conseq"], "chr", segments, features, n_tx, tables.check_codon_table(aa), tables.check_alt_order(alt_order),
                         genome.as_struct(dev), dev, prob=prob_d.data_ptr(), prob_f64=prob_d.dtype == torch.float64,
                         prob_stride=prob_d.stride(0) if n else 4, start=start_d.data_ptr(),
                         strand=None if strand_d is None else strand_d.data_ptr(), label=label_d.data_ptr(),
                         label_kind={torch.float32: 0, torch.int32: 1, torch.int64: 2}[label_d.dtype], n=n)
    return acc, int(acc["status"].item())


def _host(acc, n_tx):
    return (acc["table"].cpu().numpy().view(np.uint64)[:n_tx * 27].reshape(n_tx, 9, 3), acc["rows"].cpu().numpy().view(np.uint64)[:n_tx * 2].reshape(n_tx, 2))


def _twin(seq, prob, start, strand, label, segments, features, n_tx, **kw):
    from mural_amd.summaries import summary_txstruct_host
    return summary_txstruct_host(seq, prob, start, strand, label, segments, features, n_tx, **kw)


def _same(acc, want, n_tx):
    got = _host(acc, n_tx)
    return got[0].tobytes() == want[0].tobytes() and got[1].tobytes() == want[1].tobytes()


@pytest.fixture(scope="module")
def record():
    from mural_amd import tables
    seq, text, names = S.build()
    tx = tables.read_transcript_structure(io.StringIO(text))
    return dict(seq=seq, text=text, names=names, meta=tx[1], tx=tx, segments=tx[2]["chr1"], features=tx[3]["chr1"], genome=_genome(seq),
                n_tx=len(names))


def _both(record, prob, start, strand, label, **kw):
    pad = kw.pop("pad", 0)
    acc, status = _kernel(record["genome"], prob, start, strand, label, record["segments"], record["features"], record["n_tx"], pad=pad, **kw)
    want = _twin(record["seq"], prob, start, strand, label, record["segments"], record["features"], record["n_tx"], **kw)
    return acc, status, want


# ---- 1. the kernel against the twin ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype,label_kind,pad", [(np.float32, 0, 3), (np.float64, 1, 0), (np.float32, 2, 1)])
def test_kernel_equals_the_twin_on_the_record(record, dtype, label_kind, pad):
    prob, start, strand, label = S.rows(record["seq"], seed=label_kind, dtype=dtype)
    label = label.astype(LABEL_DTYPES[label_kind])
    acc, status, want = _both(record, prob, start, strand, label, pad=pad)
    assert status == 0 and want[2] == 0 and _same(acc, want, record["n_tx"])
    assert len(record["features"]["feat_b0"]) > 600 and record["n_tx"] > 60 and len(start) > 3000
    assert (want[0][:, :, 0].sum(axis=0) > 0).all()                                  # every bin is reached
    assert S.as_integers(*_host(acc, record["n_tx"])) == S.oracle(record["seq"], record["text"], prob, start, strand, label)


def test_no_strand_other_code_other_order(record):
    prob, start, _, label = S.rows(record["seq"], seed=7, dtype=np.float32)
    kw = dict(aa=D.CODE.replace("W", "*").replace("M", "I"), alt_order="TGC,TGA,TCA,GCA")
    acc, status, want = _both(record, prob, start, None, label, **kw)
    plain = _twin(record["seq"], prob, start, None, label, record["segments"], record["features"], record["n_tx"])
    assert status == 0 and _same(acc, want, record["n_tx"]) and want[0].tobytes() != plain[0].tobytes()


def test_calls_accumulate_and_parts_give_the_one_call_tables(record):
    prob, start, strand, label = S.rows(record["seq"], seed=8)
    want = _twin(record["seq"], prob, start, strand, label, record["segments"], record["features"], record["n_tx"])
    for parts in (2, 7):
        acc = None
        for rows in np.array_split(np.arange(len(start)), parts):
            acc, status = _kernel(record["genome"], prob[rows], start[rows], strand[rows], label[rows], record["segments"], record["features"],
                                  record["n_tx"], into=acc)
            assert status == 0
        assert _same(acc, want, record["n_tx"]), parts


# ---- 2. the loop bounds ---------------------------------------------------------------------------------------------------------------------
def test_past_the_chunk_length_the_grid_and_the_scan_threads():
    """Transcripts of two-base exons and three-base introns, enough of them for more chunks than the reduce grid has waves and more
    items than the scan workgroup has threads (a run of several items per thread) -- 8 280 two-base items at the present bounds --; one
    two-exon transcript whose intron's rows are repeated until the item holds more than two chunks and a partial one (2 336 rows at the
    present chunk length).  The bounds are read from the getters."""
    from mural_amd import tables
    lib = _lib().lib()
    chunk, waves, scan = int(lib.mural_summary_txstruct_chunk_rows()), int(lib.mural_summary_txstruct_grid_waves()), int(lib.mural_summary_txstruct_scan_threads())
    n_exons = max(waves, 2 * scan) + 37
    per_tx = 90
    rng = np.random.default_rng(11)
    lines, pos = [], 300
    for t in range(-(-n_exons // per_tx)):
        blocks = [(pos + 5 * j, pos + 5 * j + 2) for j in range(per_tx)]
        lines.append(D.bed12("chr1", f"t{t}", "+-"[t & 1], blocks, None if t % 3 else (blocks[2][0], blocks[-3][1])))
        pos = blocks[-1][1] + 3
    lines.append(D.bed12("chr1", "long", "-", [(1, 3), (295, 297)]))
    seq = "".join(rng.choice(list("ACGT"), size=pos + 10))
    names, meta, segments, features = tables.read_transcript_structure(io.StringIO("\n".join(lines) + "\n"))
    segments, features = segments["chr1"], features["chr1"]
    repeat = -(-(2 * chunk + 77) // 292)
    start = np.sort(np.concatenate([np.arange(len(seq)), np.repeat(np.arange(3, 295), repeat - 1)])).astype(np.int64)
    n = len(start)
    prob = rng.dirichlet(np.ones(4), size=n).astype(np.float32)
    strand, label = rng.integers(0, 2, size=n).astype(np.uint8), rng.integers(0, 4, size=n).astype(np.int32)
    two_base = int((features["feat_b1"] - features["feat_b0"] == 2).sum())
    assert two_base > waves and two_base > scan and 292 * repeat > 2 * chunk
    acc, status = _kernel(_genome(seq), prob, start, strand, label, segments, features, len(names))
    want = _twin(seq, prob, start, strand, label, segments, features, len(names))
    assert status == 0 and _same(acc, want, len(names))
    assert int(want[1][-1, 0]) == 292 * repeat + 4 and int(want[1][:-1, 0].sum()) == (5 * per_tx - 3) * (len(names) - 1)
    assert int(want[0][-1, 3, 0] + want[0][-1, 4, 0] + want[0][-1, 6, 0]) > 0


def test_lo_carries_into_hi():
    """An intron of 6 bases between two one-codon exons, its positions repeated 3000 times each (18 chunks).  Class 1 has p = 1 - 2^-24 (hi
    = 2^31 - 2^7, lo = 0), class 2 p = (2^40 - 1) 2^-71 (hi = 0, lo = 2^40 - 1: two rows carry), class 3 p = 2^-32 + 2^-71 (lo = 2^39 + 1).
    The expected cells in closed form, as Python integers split into limbs."""
    from mural_amd import tables
    seq, reps = "GGATGCCTTAGGATGCC", 3000
    names, meta, segments, features = tables.read_transcript_structure(io.StringIO(D.bed12("chr1", "t", "+", [(2, 5), (11, 14)]) + "\n"))
    start = np.repeat(np.arange(2, 14), reps).astype(np.int64)
    n = len(start)
    q = [(2 ** 31 - 2 ** 7) << 40, 2 ** 40 - 1, 2 ** 39 + 1]
    prob = np.zeros((n, 4), np.float64)
    prob[:, 1:] = [1.0 - 2.0 ** -24, float(2 ** 40 - 1) * 2.0 ** -71, 2.0 ** -32 + 2.0 ** -71]
    label = np.full(n, 2, np.int64)
    acc, status = _kernel(_genome(seq), prob, start, None, label, segments["chr1"], features["chr1"], 1)
    want = _twin(seq, prob, start, None, label, segments["chr1"], features["chr1"], 1)
    assert status == 0 and _same(acc, want, 1)
    table, rows = _host(acc, 1)
    assert rows.tolist() == [[n, 0]] and (table[:, :, 2] < np.uint64(1 << 40)).all()
    value = [(int(h) << 40) + int(l) for _, h, l in table[0].tolist()]
    # donor 2 bases, acceptor 2, intron 2, start lost 3 (ATG), cds 3
    assert value == [0, 0, 0, 2 * reps * sum(q), 2 * reps * sum(q), 0, 2 * reps * sum(q), 3 * reps * sum(q), 3 * reps * sum(q)]
    assert table[0, :, 0].tolist() == [0, 0, 0, 2 * reps, 2 * reps, 0, 2 * reps, 3 * reps, 3 * reps]


# ---- 3. status, and calls that launch nothing -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("what,bit", [("start", 1), ("label", 2), ("nan", 8), ("above", 8)])
def test_bad_rows_are_skipped_and_set_status(record, what, bit):
    prob, start, strand, label = S.rows(record["seq"], seed=3, dtype=np.float32)
    at = 1030
    if what == "start":
        start[0] = -4                                          # (the rows still ascend)
    elif what == "label":
        label[at] = 4
    else:
        prob[at, 2] = dict(nan=np.nan, above=1.5)[what]
    prob[at + 1, 0] = np.nan                                   # class 0's probability is never read
    acc, status, want = _both(record, prob, start, strand, label)
    assert status == bit == want[2] and _same(acc, want, record["n_tx"])


def test_a_descending_pair_sets_status_4(record):
    prob, start, strand, label = S.rows(record["seq"], seed=3, dtype=np.float32, extra=0)
    start[100], start[101] = start[101], start[100]
    _, status = _kernel(record["genome"], prob, start, strand, label, record["segments"], record["features"], record["n_tx"])
    assert status == 4


def test_calls_that_launch_nothing_leave_the_tables_untouched(record):
    n_tx = record["n_tx"]
    prob, start, strand, label = S.rows(record["seq"], seed=2, dtype=np.float32)
    acc, status = _kernel(record["genome"], prob[:0], start[:0], strand[:0], label[:0], record["segments"], record["features"], n_tx,
                          into=_acc(n_tx, 7))
    assert status == 0 and (acc["table"] == 7).all() and (acc["rows"] == 7).all()
    none = {key: v[:0] if key.startswith("feat_") else v for key, v in record["features"].items()}
    acc, status = _kernel(record["genome"], prob, start, strand, label, record["segments"], none, n_tx, into=_acc(n_tx, 7))
    assert status == 0 and (acc["table"] == 7).all() and (acc["rows"] == 7).all()
    # a chromosome the file does not name: the reducer launches nothing
    from mural_amd.predict import SummarySink
    sink = SummarySink(None, transcripts=record["tx"], genome=lambda name: record["genome"], transcript_structure=True)
    sink({"chrom": "chrZ", "start": _up(start), "end": _up(start + 1), "strand": _up(strand), "label": _up(label.astype(np.float32)),
          "prob": _up(prob), "n_class": 4, "calibrated": False, "aligned": True})
    assert not sink._reducers["transcript_structure"].dev
    sink.close()
    assert not sink.structure_sums()[0].any() and not sink.structure_sums()[1].any()


def test_a_chromosome_without_cds_on_the_device():
    """Items and no segments: the entry takes n_segments == 0, and the sink uploads the strands on its own."""
    from mural_amd import tables
    from mural_amd.predict import SummarySink
    text = D.bed12("chr2", "nc", "-", [(5, 12), (20, 30)], (5, 5)) + "\n" + D.bed12("chr1", "c", "+", [(0, 9)]) + "\n"
    tx = tables.read_transcript_structure(io.StringIO(text))
    seq = "ACGT" * 10
    genome = _genome(seq)
    start = np.arange(40)
    prob, label, strand = np.full((40, 4), 0.25, np.float32), np.ones(40, np.float32), np.zeros(40, np.uint8)
    sink = SummarySink(None, transcripts=tx, genome=lambda name: genome, transcript_structure=True)
    sink({"chrom": "chr2", "start": _up(start), "end": _up(start + 1), "strand": _up(strand), "label": _up(label), "prob": _up(prob),
          "n_class": 4, "calibrated": False, "aligned": True})
    sink.close()
    want = _twin(seq, prob, start, strand, label, None, tx[3]["chr2"], 2)
    got = sink.structure_sums()
    assert got[0].tobytes() == want[0].tobytes() and got[1].tobytes() == want[1].tobytes() and got[1].tolist() == [[25, 0], [0, 0]]


def test_refusals(record):
    L = _lib()
    lib = L.lib()
    prob, start, strand, label = S.rows(record["seq"], seed=2, dtype=np.float32)
    n_tx = record["n_tx"]

    def call(alt_order=None, ws_short=False, **fields):
        """The return code of one call with `fields` overridden; the arrays are the record's."""
        from mural_amd import tables
        dev = _dev()
        acc = _acc(n_tx)
        keep = [_up(prob), _up(start), _up(label)] + [_up(record["features"][k]) for k in ("feat_b0", "feat_b1", "feat_tx", "feat_kind", "feat_seg")]
        keep += [_up(record["segments"][k]) for k in ("seg_b0", "seg_b1", "seg_cds0", "seg_tx", "seg_prev", "seg_next", "tx_strand", "tx_cds_len")]
        g = record["genome"].as_struct(dev)
        s = L.MuralSummaryTxstructRows()
        s.genome = C.pointer(g)
        s.prob, s.prob_f64, s.prob_stride, s.start, s.label, s.label_kind = keep[0].data_ptr(), 0, 4, keep[1].data_ptr(), keep[2].data_ptr(), 2
        s.n, s.n_class, s.n_transcripts = len(start), 4, n_tx
        s.feat_b0, s.feat_b1, s.feat_tx, s.feat_kind, s.feat_seg = (x.data_ptr() for x in keep[3:8])
        s.n_features = len(record["features"]["feat_b0"])
        s.seg_b0, s.seg_b1, s.seg_cds0, s.seg_tx, s.seg_prev, s.seg_next, s.tx_strand, s.tx_cds_len = (x.data_ptr() for x in keep[8:16])
        s.n_segments = len(record["segments"]["seg_b0"])
        C.memmove(s.aa, record["meta"]["aa"].ctypes.data, 64)
        C.memmove(s.alt_order, np.ascontiguousarray(tables.check_alt_order(None) if alt_order is None else alt_order, np.uint8).ctypes.data, 12)
        s.table, s.rows, s.status = acc["table"].data_ptr(), acc["rows"].data_ptr(), acc["status"].data_ptr()
        for key, v in fields.items():
            setattr(s, key, v)
        need = int(lib.mural_summary_txstruct_workspace_bytes(s.n_features))
        ws = torch.empty(need // 8 + 1, dtype=torch.int64, device=dev)
        rc = lib.mural_summary_txstruct_rows(C.byref(s), ws.data_ptr(), need - 8 if ws_short else need, L.current_stream_ptr(dev))
        torch.cuda.synchronize()
        return rc, acc

    rc, acc = call()
    want = _twin(record["seq"], prob, start, None, label, record["segments"], record["features"], n_tx)
    assert rc == 0 and _same(acc, want, n_tx)
    invalid = 1
    for fields in (dict(n_class=2), dict(n=(1 << 31) + 1), dict(n=-1), dict(n_features=(1 << 22) + 1), dict(label_kind=3), dict(prob_stride=3),
                   dict(feat_kind=None), dict(seg_next=None), dict(table=None)):
        rc, acc = call(**fields)
        assert rc == invalid and not acc["table"].any(), fields
    rc, acc = call(alt_order=np.zeros((4, 3), np.uint8))
    assert rc == invalid and not acc["table"].any()
    rc, acc = call(ws_short=True)
    assert rc != 0 and rc != invalid and not acc["table"].any()          # MURAL_E_WORKSPACE
    with pytest.raises(ValueError, match="alt_order"):
        L.check(call(alt_order=np.zeros((4, 3), np.uint8))[0])


# ---- 4. the sink's routes -------------------------------------------------------------------------------------------------------------------
def _run_equals_the_twin(fwd, records, regions, focal, d, tag):
    from mural_amd import predict as P
    from mural_amd import tables
    text = _transcripts_over(records, regions)
    tx = tables.read_transcript_structure(io.StringIO(text))
    keep, sink = _Keep(), P.SummarySink(str(d / tag), transcripts=tx, genome=fwd.genome, transcript_labels=False, transcript_structure=True)
    n = P.predict_regions_sharded(fwd, regions, focal, sink=P.TeeSink(keep, sink), collect=False)
    want = None
    for chrom, parts in keep.rows.items():
        prob, start, label, strand = (np.concatenate([p[i] for p in parts]) for i in range(4))
        if chrom in tx[3]:
            t, r, status = _twin(records[chrom], prob, start, strand, label, tx[2].get(chrom), tx[3][chrom], len(tx[0]), into=want)
            want = (t, r)
            assert status == 0
    got = sink.structure_sums()
    assert n > 0 and got[0].tobytes() == want[0].tobytes() and got[1].tobytes() == want[1].tobytes() and int(want[1][:, 0].sum()) > 100
    assert (want[0][:, [3, 4, 6, 7, 8], 1].sum(axis=0) > 0).all()
    lines = (d / f"{tag}.consequence.structure.tsv").read_text().splitlines()
    assert [ln.split("\t")[0] for ln in lines[1:]] == tx[0] and lines[1].split("\t")[6] == "NA"
    assert (d / f"{tag}.consequence.mut_rates.tsv").exists()


def test_sink_behind_a_single_focal_regions_run_equals_the_twin(files, snv_model):
    from tests.test_gpu_region_labels import RECORDS
    d, fa = files
    _run_equals_the_twin(_forward(snv_model, fa), RECORDS, REGIONS, "A", d, "txstruct_a")


def test_sink_behind_a_model_set_run_equals_the_twin(set_files, set_models):
    """Rows at every base of the regions, each on its base's own strand."""
    from tests import test_gpu_model_set as M
    d, fa = set_files
    fwd, _ = M._set(set_models, fa)
    _run_equals_the_twin(fwd, M.RECORDS, M.REGIONS, "SET", d, "txstruct_set")


def test_table_route_and_command_line(files, snv_model, tmp_path):
    """The written table through ``tables.structure_table``: the counts of the in-flight sink, the sums within the table's four digits;
    ``run_structure_calc`` and the command line write the same file; the flag is refused without --transcripts and with --indel."""
    from mural_amd import predict as P
    from mural_amd import tables
    from mural_amd.model import nn_utils
    from tests.test_gpu_region_labels import RECORDS
    d, fa = files
    regions = {"chrA": REGIONS["chrA"][:1]}
    text = _transcripts_over(RECORDS, regions, seed=3)
    bed = tmp_path / "tx.bed"
    bed.write_text(text)
    tx = tables.read_transcript_structure(str(bed))
    fwd = _forward(snv_model, fa)
    out = str(tmp_path / "t.tsv")
    sink = P.SummarySink(str(tmp_path / "s"), transcripts=tx, genome=fwd.genome, transcript_structure=True)
    P.predict_regions_sharded(fwd, regions, "A", sink=P.TeeSink(P.TsvSink(out), sink), collect=False)
    names, meta, table, rows, stop_gained = tables.structure_table(out, tx, fa, chunk_bytes=16 << 10)      # several chunks
    want_table, want_rows = sink.structure_sums()
    assert names == tx[0] and np.array_equal(table[:, :, 0], want_table[:, :, 0]) and np.array_equal(rows, want_rows) and rows[:, 0].sum() > 100
    assert np.array_equal(stop_gained[:, 0], sink.consequence_sums()[0][:, 2, 0])
    value = lambda t: np.array([[((int(h) << 40) + int(l)) / 2 ** 71 for _, h, l in cells] for cells in t.tolist()])      # noqa: E731
    # a printed probability is within 5e-5 relative (four digits) of the one that was reduced in flight, or below the smallest printed value
    assert (np.abs(value(table) - value(want_table)) <= 5e-4 * value(want_table) + 1e-30).all()

    class Args:
        pred_file, transcripts, ref_genome, out_prefix = out, str(bed), fa, str(tmp_path / "calc")
    path = tables.run_structure_calc(Args)
    calc = open(path).read().splitlines()
    assert path == str(tmp_path / "calc.consequence.structure.tsv") and [ln.split("\t")[0] for ln in calc[1:]] == names
    ckpt = str(tmp_path / "model")
    nn_utils.save_model(snv_model[0], None, snv_model[1], ckpt)
    spec = importlib.util.spec_from_file_location("predict_files", os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))),
                                                                                  "tools", "predict_files.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    region_args = [a for lo, hi in regions["chrA"] for a in ("--regions", f"chrA:{lo + 1}-{hi}")]
    mod.main([ckpt, fa, str(tmp_path / "cli.tsv"), *region_args, "--focal", "A", "--summary", str(tmp_path / "cli"), "--transcripts", str(bed),
              "--transcript_structure"])
    cli = (tmp_path / "cli.consequence.structure.tsv").read_text().splitlines()
    api = (tmp_path / "s.consequence.structure.tsv").read_text().splitlines()
    counts = lambda lines: [ln.split("\t")[:5] + ln.split("\t")[5::2] for ln in lines[1:]]      # noqa: E731  (--regions alone: observed is NA)
    assert cli[0] == api[0] == calc[0] and counts(cli) == counts(api)
    assert [ln.split("\t")[:5] + ln.split("\t")[6::2] for ln in calc[1:]] == [ln.split("\t")[:5] + ln.split("\t")[6::2] for ln in api[1:]]
    with pytest.raises(SystemExit, match="--transcripts"):
        mod.main([ckpt, fa, str(tmp_path / "cli2.tsv"), *region_args, "--focal", "A", "--summary", str(tmp_path / "cli2"), "--window_size", "100",
                  "--transcript_structure"])
    with pytest.raises(SystemExit, match="--indel"):
        mod.main([ckpt, fa, str(tmp_path / "cli3.tsv"), *region_args, "--summary", str(tmp_path / "cli3"), "--transcripts", str(bed),
                  "--transcript_structure", "--indel"])
    assert not (tmp_path / "cli2.tsv").exists() and not (tmp_path / "cli3.tsv").exists()
