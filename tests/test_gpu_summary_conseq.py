"""Consequence tables on the device (csrc/summary_conseq.hip: mural_summary_conseq_rows; mural_amd.predict.SummarySink(transcripts=...);
mural_amd.tables.consequence_table): every case goes through the entry point and is compared for EQUALITY with the numpy twin
``summary_conseq_host`` -- the record of tests/_conseq_data.py (both strands, codons over one and two junctions, incomplete and masked
codons, nesting) in both probability types and the three label kinds, the three loop bounds of the entry read from its getters, the
carry of lo into hi, the status bits, calls that launch nothing, additivity over calls, and the sink's routes: a single-focal regions run,
a model-set run, the table route and the command line."""
import ctypes as C
import importlib.util
import os

import numpy as np
import pytest
import torch

from tests import _conseq_data as D
from tests.test_gpu_model_set import files as set_files, models as set_models  # noqa: F401  (fixtures)
from tests.test_gpu_region_labels import REGIONS, _forward, files, snv_model  # noqa: F401  (fixtures)

pytestmark = pytest.mark.gpu

LABEL_DTYPES = {0: np.float32, 1: np.int32, 2: np.int64}


def _dev():
    return torch.device("cuda", torch.cuda.current_device())


def _lib():
    from mural_amd import _lib
    return _lib


def _up(a):
    return a if isinstance(a, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(a)).to(_dev())


def _genome(seq):
    from mural_amd.data import PackedGenome
    return PackedGenome.from_sequence(seq, _dev())


def _kernel(genome, prob, start, strand, label, segments, n_tx, aa=None, alt_order=None, into=None, pad=0):
    """One mural_summary_conseq_rows call on device copies of the arrays: ((table, rows) tensors, status)."""
    from mural_amd import tables
    from mural_amd.summaries import conseq_rows_device
    dev = _dev()
    if pad:
        prob = np.concatenate([prob, np.full((len(prob), pad), 0.25, prob.dtype)], axis=1)
    prob_d, start_d, label_d = _up(prob), _up(start), _up(label)
    strand_d = None if strand is None else _up(strand)
    acc = into or dict(table=torch.zeros(max(n_tx, 1) * 15, dtype=torch.int64, device=dev), rows=torch.zeros(max(n_tx, 1) * 2, dtype=torch.int64, device=dev),
                       status=torch.zeros(1, dtype=torch.int32, device=dev), segments={}, ws=None)
    n = int(start_d.shape[0])
    conseq_rows_device(acc, "chr", segments, n_tx, tables.check_codon_table(aa), tables.check_alt_order(alt_order), genome.as_struct(dev), dev,
                       prob=prob_d.data_ptr(), prob_f64=prob_d.dtype == torch.float64, prob_stride=prob_d.stride(0) if n else 4,
                       start=start_d.data_ptr(), strand=None if strand_d is None else strand_d.data_ptr(), label=label_d.data_ptr(),
                       label_kind={torch.float32: 0, torch.int32: 1, torch.int64: 2}[label_d.dtype], n=n)
    return acc, int(acc["status"].item())


def _host(acc, n_tx):
    return (acc["table"].cpu().numpy().view(np.uint64)[:n_tx * 15].reshape(n_tx, 5, 3), acc["rows"].cpu().numpy().view(np.uint64)[:n_tx * 2].reshape(n_tx, 2))


def _twin(seq, prob, start, strand, label, segments, n_tx, **kw):
    from mural_amd.summaries import summary_conseq_host
    return summary_conseq_host(seq, prob, start, strand, label, segments, n_tx, **kw)


def _same(acc, want, n_tx):
    got = _host(acc, n_tx)
    return got[0].tobytes() == want[0].tobytes() and got[1].tobytes() == want[1].tobytes()


@pytest.fixture(scope="module")
def record():
    from mural_amd import tables
    import io
    seq, text, names = D.build()
    _, meta, segments = tables.read_transcripts(io.StringIO(text))
    return dict(seq=seq, text=text, names=names, meta=meta, segments=segments["chr1"], genome=_genome(seq), n_tx=len(names))


# ---- 1. the kernel against the twin ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype,label_kind,pad", [(np.float32, 0, 3), (np.float64, 1, 0), (np.float32, 2, 1)])
def test_kernel_equals_the_twin_on_the_record(record, dtype, label_kind, pad):
    prob, start, strand, label = D.rows(record["seq"], seed=label_kind, dtype=dtype)
    label = label.astype(LABEL_DTYPES[label_kind])
    acc, status = _kernel(record["genome"], prob, start, strand, label, record["segments"], record["n_tx"], pad=pad)
    want = _twin(record["seq"], prob, start, strand, label, record["segments"], record["n_tx"])
    assert status == 0 and want[2] == 0 and _same(acc, want, record["n_tx"])
    assert len(record["segments"]["seg_b0"]) > 300 and record["n_tx"] > 40 and len(start) > 3000
    assert (want[0][:, :, 0].sum(axis=0) > 0).all()                                  # every bin is reached
    assert D.as_integers(*_host(acc, record["n_tx"])) == D.oracle(record["seq"], record["text"], prob, start, strand, label)


def test_no_strand_other_code_other_order(record):
    prob, start, _, label = D.rows(record["seq"], seed=7, dtype=np.float32)
    kw = dict(aa=D.CODE.replace("W", "*").replace("M", "I"), alt_order="TGC,TGA,TCA,GCA")
    acc, status = _kernel(record["genome"], prob, start, None, label, record["segments"], record["n_tx"], **kw)
    want = _twin(record["seq"], prob, start, None, label, record["segments"], record["n_tx"], **kw)
    plain = _twin(record["seq"], prob, start, None, label, record["segments"], record["n_tx"])
    assert status == 0 and _same(acc, want, record["n_tx"]) and want[0].tobytes() != plain[0].tobytes()


def test_calls_accumulate_and_parts_give_the_one_call_tables(record):
    prob, start, strand, label = D.rows(record["seq"], seed=8)
    want = _twin(record["seq"], prob, start, strand, label, record["segments"], record["n_tx"])
    for parts in (2, 7):
        acc = None
        for rows in np.array_split(np.arange(len(start)), parts):
            acc, status = _kernel(record["genome"], prob[rows], start[rows], strand[rows], label[rows], record["segments"], record["n_tx"], into=acc)
            assert status == 0
        assert _same(acc, want, record["n_tx"]), parts


# ---- 2. the loop bounds ---------------------------------------------------------------------------------------------------------------------
def test_past_the_chunk_length_the_grid_and_the_scan_threads():
    """Transcripts of two-base exons, enough of them for more chunks than the reduce grid has waves and more segments than the scan
    workgroup has threads (a run of several segments per thread); one one-exon transcript over a stretch whose rows are repeated until
    the segment holds more than two chunks and a partial one.  The bounds are read from the getters."""
    import io
    from mural_amd import tables
    lib = _lib().lib()
    chunk, waves, scan = int(lib.mural_summary_conseq_chunk_rows()), int(lib.mural_summary_conseq_grid_waves()), int(lib.mural_summary_conseq_scan_threads())
    n_seg = max(waves, 2 * scan) + 37
    per_tx = 90
    rng = np.random.default_rng(11)
    lines, pos = [], 300
    for t in range(-(-n_seg // per_tx)):
        blocks = [(pos + 5 * j, pos + 5 * j + 2) for j in range(per_tx)]
        lines.append(D.bed12("chr1", f"t{t}", "+-"[t & 1], blocks))
        pos = blocks[-1][1] + 3
    lines.append(D.bed12("chr1", "long", "-", [(3, 295)]))
    seq = "".join(rng.choice(list("ACGT"), size=pos + 10))
    names, meta, segments = tables.read_transcripts(io.StringIO("\n".join(lines) + "\n"))
    segments = segments["chr1"]
    repeat = -(-(2 * chunk + 77) // 292)
    start = np.sort(np.concatenate([np.arange(len(seq)), np.repeat(np.arange(3, 295), repeat - 1)])).astype(np.int64)
    n = len(start)
    prob = rng.dirichlet(np.ones(4), size=n).astype(np.float32)
    strand, label = rng.integers(0, 2, size=n).astype(np.uint8), rng.integers(0, 4, size=n).astype(np.int32)
    assert len(segments["seg_b0"]) > waves and len(segments["seg_b0"]) > scan and 292 * repeat > 2 * chunk
    acc, status = _kernel(_genome(seq), prob, start, strand, label, segments, len(names))
    want = _twin(seq, prob, start, strand, label, segments, len(names))
    assert status == 0 and _same(acc, want, len(names))
    assert int(want[1][-1, 0]) == 292 * repeat and int(want[1][:-1, 0].sum()) == 2 * (len(segments["seg_b0"]) - 1)


def test_lo_carries_into_hi():
    """One codon, its three positions repeated 3000 times each (nine chunks).  Class 1 has p = 1 - 2^-24 (hi = 2^31 - 2^7, lo = 0), class 2
    p = (2^40 - 1) 2^-71 (hi = 0, lo = 2^40 - 1: two rows carry), class 3 p = 2^-32 + 2^-71 (lo = 2^39 + 1).  The expected cells in closed
    form, as Python integers split into limbs."""
    import io
    from mural_amd import tables
    seq, reps = "GGATGCC", 3000
    names, meta, segments = tables.read_transcripts(io.StringIO(D.bed12("chr1", "t", "+", [(2, 5)]) + "\n"))
    start = np.repeat(np.arange(2, 5), reps).astype(np.int64)
    n = len(start)
    q = [(2 ** 31 - 2 ** 7) << 40, 2 ** 40 - 1, 2 ** 39 + 1]
    prob = np.zeros((n, 4), np.float64)
    prob[:, 1:] = [1.0 - 2.0 ** -24, float(2 ** 40 - 1) * 2.0 ** -71, 2.0 ** -32 + 2.0 ** -71]
    label = np.full(n, 2, np.int64)
    acc, status = _kernel(_genome(seq), prob, start, None, label, segments["chr1"], 1)
    want = _twin(seq, prob, start, None, label, segments["chr1"], 1)
    assert status == 0 and _same(acc, want, 1)
    table, rows = _host(acc, 1)
    assert rows.tolist() == [[n, 0]]
    assert (table[:, :, 2] < np.uint64(1 << 40)).all()
    total = sum((int(h) << 40) + int(l) for _, h, l in table[0].tolist())
    assert total == n * sum(q) and int(table[0, 1, 0]) == n       # ATG: all nine substitutions are missense; the label is class 2
    assert (int(table[0, 1, 1]) << 40) + int(table[0, 1, 2]) == n * sum(q)


# ---- 3. status, and calls that launch nothing -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("what,bit", [("start", 1), ("label", 2), ("nan", 8), ("above", 8)])
def test_bad_rows_are_skipped_and_set_status(record, what, bit):
    prob, start, strand, label = D.rows(record["seq"], seed=3, dtype=np.float32)
    at = 70
    if what == "start":
        start[0] = -4                                          # (the rows still ascend)
    elif what == "label":
        label[at] = 4
    else:
        prob[at, 2] = dict(nan=np.nan, above=1.5)[what]
    prob[at + 1, 0] = np.nan                                   # class 0's probability is never read
    acc, status = _kernel(record["genome"], prob, start, strand, label, record["segments"], record["n_tx"])
    want = _twin(record["seq"], prob, start, strand, label, record["segments"], record["n_tx"])
    assert status == bit == want[2] and _same(acc, want, record["n_tx"])


def test_a_descending_pair_sets_status_4(record):
    prob, start, strand, label = D.rows(record["seq"], seed=3, dtype=np.float32, extra=0)
    start[100], start[101] = start[101], start[100]
    _, status = _kernel(record["genome"], prob, start, strand, label, record["segments"], record["n_tx"])
    assert status == 4


def test_calls_that_launch_nothing_leave_the_tables_untouched(record):
    dev, n_tx = _dev(), record["n_tx"]
    prob, start, strand, label = D.rows(record["seq"], seed=2, dtype=np.float32)

    def fresh():
        return dict(table=torch.full((n_tx * 15,), 7, dtype=torch.int64, device=dev), rows=torch.full((n_tx * 2,), 7, dtype=torch.int64, device=dev),
                    status=torch.zeros(1, dtype=torch.int32, device=dev), segments={}, ws=None)

    acc, status = _kernel(record["genome"], prob[:0], start[:0], strand[:0], label[:0], record["segments"], n_tx, into=fresh())
    assert status == 0 and (acc["table"] == 7).all() and (acc["rows"] == 7).all()
    none = {key: v[:0] if key.startswith("seg_") else v for key, v in record["segments"].items()}
    acc, status = _kernel(record["genome"], prob, start, strand, label, none, n_tx, into=fresh())
    assert status == 0 and (acc["table"] == 7).all() and (acc["rows"] == 7).all()
    # a chromosome the file does not name: the reducer launches nothing
    from mural_amd.predict import SummarySink
    sink = SummarySink(None, transcripts=(record["names"], record["meta"], {"chr1": record["segments"]}), genome=lambda name: record["genome"])
    sink({"chrom": "chrZ", "start": _up(start), "end": _up(start + 1), "strand": _up(strand), "label": _up(label.astype(np.float32)),
          "prob": _up(prob), "n_class": 4, "calibrated": False, "aligned": True})
    assert not sink._reducers["consequences"].dev
    sink.close()
    assert not sink.consequence_sums()[0].any() and not sink.consequence_sums()[1].any()


def test_refusals(record):
    L = _lib()
    s = L.MuralSummaryConseqRows()
    s.n_class = 2
    assert L.lib().mural_summary_conseq_rows(C.byref(s), None, 0, None) == 1
    prob, start, strand, label = D.rows(record["seq"], seed=2, dtype=np.float32)
    with pytest.raises(ValueError, match="alt_order"):
        from mural_amd.summaries import conseq_rows_device
        dev = _dev()
        acc = dict(table=torch.zeros(record["n_tx"] * 15, dtype=torch.int64, device=dev), rows=torch.zeros(record["n_tx"] * 2, dtype=torch.int64, device=dev),
                   status=torch.zeros(1, dtype=torch.int32, device=dev), segments={}, ws=None)
        p, st, lb = _up(prob), _up(start), _up(label)
        conseq_rows_device(acc, "chr", record["segments"], record["n_tx"], record["meta"]["aa"], np.zeros((4, 3), np.uint8),
                           record["genome"].as_struct(dev), dev, prob=p.data_ptr(), prob_f64=0, prob_stride=4, start=st.data_ptr(), strand=None,
                           label=lb.data_ptr(), label_kind=2, n=len(start))


# ---- 4. the sink's routes -------------------------------------------------------------------------------------------------------------------
class _Keep:
    """Keeps every shard's rows on the host, per chromosome."""
    takes_aligned_blocks = True

    def __init__(self):
        self.rows = {}

    def __call__(self, shard):
        from mural_amd.sinks import shard_name, strand_u8
        cols = [np.asarray(v.cpu() if isinstance(v, torch.Tensor) else v) for v in (shard["prob"], shard["start"], shard["label"])]
        strand = shard["strand"]
        cols.append(strand_u8(strand.cpu().numpy() if isinstance(strand, torch.Tensor) else strand))
        self.rows.setdefault(shard_name(shard), []).append(cols)

    def close(self):
        pass


def _transcripts_over(records, regions, seed=0):
    """BED12 text: per region a few multi-exon transcripts on both strands."""
    rng = np.random.default_rng(seed)
    lines = []
    for chrom, ivs in regions.items():
        for j, (lo, hi) in enumerate(ivs):
            hi = min(hi, len(records[chrom]))
            if hi - lo < 40:
                continue
            for t in range(4):
                n_blocks = int(rng.integers(1, 8))
                cuts = np.sort(rng.choice(np.arange(lo + 1, hi), size=2 * n_blocks, replace=False))
                blocks = [(int(a), int(b)) for a, b in zip(cuts[::2], cuts[1::2])]
                lines.append(D.bed12(chrom, f"{chrom}_{j}_{t}", "+-"[t & 1], blocks))
    return "\n".join(lines) + "\n"


def _run_equals_the_twin(fwd, records, regions, focal, d, tag):
    import io
    from mural_amd import predict as P
    from mural_amd import tables
    text = _transcripts_over(records, regions)
    tx = tables.read_transcripts(io.StringIO(text))
    keep, sink = _Keep(), P.SummarySink(str(d / tag), transcripts=tx, genome=fwd.genome, transcript_labels=False)
    n = P.predict_regions_sharded(fwd, regions, focal, sink=P.TeeSink(keep, sink), collect=False)
    want = None
    for chrom, parts in keep.rows.items():
        prob, start, label, strand = (np.concatenate([p[i] for p in parts]) for i in range(4))
        if chrom in tx[2]:
            t, r, status = _twin(records[chrom], prob, start, strand, label, tx[2][chrom], len(tx[0]), into=want)
            want = (t, r)
            assert status == 0
    got = sink.consequence_sums()
    assert n > 0 and got[0].tobytes() == want[0].tobytes() and got[1].tobytes() == want[1].tobytes() and int(want[1][:, 0].sum()) > 100
    lines = (d / f"{tag}.consequence.mut_rates.tsv").read_text().splitlines()
    assert [ln.split("\t")[0] for ln in lines[1:]] == tx[0] and lines[1].split("\t")[8] == "NA"
    return text


def test_sink_behind_a_single_focal_regions_run_equals_the_twin(files, snv_model):
    from tests.test_gpu_region_labels import RECORDS
    d, fa = files
    _run_equals_the_twin(_forward(snv_model, fa), RECORDS, REGIONS, "A", d, "conseq_a")


def test_sink_behind_a_model_set_run_equals_the_twin(set_files, set_models):
    """Rows at every base of the regions, each on its base's own strand."""
    from tests import test_gpu_model_set as M
    d, fa = set_files
    fwd, _ = M._set(set_models, fa)
    _run_equals_the_twin(fwd, M.RECORDS, M.REGIONS, "SET", d, "conseq_set")


def test_table_route_and_command_line(files, snv_model, tmp_path):
    """The written table through ``tables.consequence_table``: the counts of the in-flight sink, the sums within the table's four digits;
    the command line writes the sink's file and refuses --transcripts without --summary."""
    import io
    from mural_amd import predict as P
    from mural_amd import tables
    from mural_amd.model import nn_utils
    from tests.test_gpu_region_labels import RECORDS
    d, fa = files
    regions = {"chrA": REGIONS["chrA"][:1]}
    text = _transcripts_over(RECORDS, regions, seed=3)
    bed = tmp_path / "tx.bed"
    bed.write_text(text)
    tx = tables.read_transcripts(str(bed))
    fwd = _forward(snv_model, fa)
    out = str(tmp_path / "t.tsv")
    sink = P.SummarySink(str(tmp_path / "s"), transcripts=tx, genome=fwd.genome)
    P.predict_regions_sharded(fwd, regions, "A", sink=P.TeeSink(P.TsvSink(out), sink), collect=False)
    names, meta, table = tables.consequence_table(out, tx, fa, chunk_bytes=16 << 10)      # several chunks
    want = sink.result()["consequences"][2]
    counts = [0, 1, 2, 4, 6, 8, 10]
    assert names == tx[0] and np.array_equal(table[:, counts], want[:, counts]) and want[:, 0].sum() > 100
    sums = [3, 5, 7, 9, 11]
    # a printed probability is within 5e-5 relative (four digits) of the one that was reduced in flight, or below the smallest printed value
    assert (np.abs(table[:, sums] - want[:, sums]) <= 5e-4 * want[:, sums] + 1e-30).all()

    class Args:
        pred_file, transcripts, ref_genome, out_prefix = out, str(bed), fa, str(tmp_path / "calc")
    tables.run_consequence_calc(Args)
    assert [ln.split("\t")[0] for ln in (tmp_path / "calc.consequence.mut_rates.tsv").read_text().splitlines()[1:]] == names
    ckpt = str(tmp_path / "model")
    nn_utils.save_model(snv_model[0], None, snv_model[1], ckpt)
    spec = importlib.util.spec_from_file_location("predict_files", os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))),
                                                                                  "tools", "predict_files.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    region_args = [a for lo, hi in regions["chrA"] for a in ("--regions", f"chrA:{lo + 1}-{hi}")]
    mod.main([ckpt, fa, str(tmp_path / "cli.tsv"), *region_args, "--focal", "A", "--summary", str(tmp_path / "cli"), "--transcripts", str(bed)])
    cli = (tmp_path / "cli.consequence.mut_rates.tsv").read_text().splitlines()
    api = (tmp_path / "s.consequence.mut_rates.tsv").read_text().splitlines()
    assert cli[0] == api[0] and [ln.split("\t")[:7] + ln.split("\t")[7::2] for ln in cli[1:]] == [ln.split("\t")[:7] + ln.split("\t")[7::2] for ln in api[1:]]
    with pytest.raises(SystemExit, match="--summary"):
        mod.main([ckpt, fa, str(tmp_path / "cli2.tsv"), *region_args, "--focal", "A", "--transcripts", str(bed)])
    assert not (tmp_path / "cli2.tsv").exists()
