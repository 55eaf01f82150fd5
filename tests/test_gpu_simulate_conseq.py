"""The simulated null of the consequence table on the device (csrc/simulate_conseq.hip: mural_simulate_conseq_rows;
mural_amd.predict.SummarySink(simulate_transcripts=True); mural_amd.tables.simulate_consequence_table): every case goes through the entry
point and is compared for EQUALITY with the numpy twin ``simulate_conseq_host`` -- the record of tests/_conseq_data.py in both
probability types, with and without strands, at replicate counts around a Philox call, a block of 64 and two blocks, the three loop bounds
read from the simulation's getters, the identity with the two existing entries on the device, calls that accumulate or launch nothing, the
refusals, and the sink's routes: a single-focal regions run, the table route and the command line."""
import ctypes as C
import importlib.util
import io
import os

import numpy as np
import pytest
import torch

from tests import _conseq_data as D
from tests.test_gpu_region_labels import REGIONS, _forward, files, snv_model  # noqa: F401  (fixtures)
from tests.test_gpu_summary_conseq import _Keep, _dev, _genome, _lib, _transcripts_over, _up

pytestmark = pytest.mark.gpu

KEY, SEED = 0xC0FFEE11, (3 << 33) + 5
POISON = 0x07070707


def _acc(n_tx, dev):
    return dict(table=torch.zeros(max(n_tx, 1) * 15, dtype=torch.int64, device=dev), rows=torch.zeros(max(n_tx, 1) * 2, dtype=torch.int64, device=dev),
                status=torch.zeros(1, dtype=torch.int32, device=dev), segments={}, ws=None)


def _struct(genome, prob_d, start_d, strand_d, seg_d, tx_d, n_tx, n_rep, table, status, aa=None, alt_order=None):
    from mural_amd import tables
    L, dev = _lib(), _dev()
    s = L.MuralSimulateConseqRows()
    g = genome.as_struct(dev)
    s.genome = C.pointer(g)
    s.prob, s.prob_f64, s.prob_stride, s.n_class = prob_d.data_ptr(), int(prob_d.dtype == torch.float64), prob_d.stride(0) if prob_d.shape[0] else 4, 4
    s.start, s.strand, s.n = start_d.data_ptr(), None if strand_d is None else strand_d.data_ptr(), int(start_d.shape[0])
    s.chrom_key, s.n_rep, s.seed = KEY, n_rep, SEED
    s.seg_b0, s.seg_b1, s.seg_cds0, s.seg_tx, s.seg_prev, s.seg_next = (x.data_ptr() for x in seg_d)
    s.n_segments, s.n_transcripts = int(seg_d[0].shape[0]), n_tx
    s.tx_strand, s.tx_cds_len = tx_d[0].data_ptr(), tx_d[1].data_ptr()
    C.memmove(s.aa, np.ascontiguousarray(tables.check_codon_table(aa), np.uint8).ctypes.data, 64)
    C.memmove(s.alt_order, np.ascontiguousarray(tables.check_alt_order(alt_order), np.uint8).ctypes.data, 12)
    s.table, s.status = table.data_ptr(), status.data_ptr()
    return s, g


def _kernel(genome, prob, start, strand, segments, n_tx, n_rep, aa=None, alt_order=None, into=None, pad=0, fill=0, rc=0, edit=None, short_ws=False):
    """One mural_simulate_conseq_rows call on device copies of the arrays: (table uint32 [n_tx][5][n_rep] on the host, status)."""
    L, dev = _lib(), _dev()
    lib = L.lib()
    if pad:
        prob = np.concatenate([prob, np.full((len(prob), pad), 0.25, prob.dtype)], axis=1)
    prob_d, start_d = _up(prob), _up(start)
    strand_d = None if strand is None else _up(strand)
    seg_d = tuple(_up(np.ascontiguousarray(segments[key])) for key in ("seg_b0", "seg_b1", "seg_cds0", "seg_tx", "seg_prev", "seg_next"))
    tx_d = (_up(np.ascontiguousarray(segments["tx_strand"])), _up(np.ascontiguousarray(segments["tx_cds_len"])))
    table = torch.full((max(n_tx * 5 * n_rep, 1),), fill, dtype=torch.int32, device=dev) if into is None else into
    status = torch.zeros(1, dtype=torch.int32, device=dev)
    s, g = _struct(genome, prob_d, start_d, strand_d, seg_d, tx_d, n_tx, n_rep, table, status, aa, alt_order)
    if edit:
        edit(s)
    need = int(lib.mural_simulate_conseq_workspace_bytes(int(seg_d[0].shape[0])))
    assert need >= 24 * int(seg_d[0].shape[0])      # (the arena aligns each array)
    ws = torch.empty(need // 8 + 1, dtype=torch.int64, device=dev)
    got = lib.mural_simulate_conseq_rows(C.byref(s), ws.data_ptr(), need - 8 if short_ws else ws.numel() * 8, L.current_stream_ptr(dev))
    assert got == rc
    torch.cuda.synchronize()
    return table, int(status.item())


def _host(table, n_tx, n_rep):
    return table.cpu().numpy().view(np.uint32)[:n_tx * 5 * n_rep].reshape(n_tx, 5, n_rep)


def _twin(seq, prob, start, strand, segments, n_tx, n_rep, **kw):
    from mural_amd.summaries import simulate_conseq_host
    return simulate_conseq_host(seq, prob, start, strand, segments, n_tx, KEY, SEED, n_rep, **kw)


@pytest.fixture(scope="module")
def record():
    from mural_amd import tables
    seq, text, names = D.build()
    _, meta, segments = tables.read_transcripts(io.StringIO(text))
    return dict(seq=seq, text=text, names=names, meta=meta, segments=segments["chr1"], genome=_genome(seq), n_tx=len(names))


@pytest.fixture(scope="module")
def record_twin(record):
    """The twin's table of the record's float32 rows at 129 replicates, computed once: the cases at fewer replicates read its columns
    (replicate r does not depend on the replicate count)."""
    prob, start, strand, _ = D.rows(record["seq"], seed=1, dtype=np.float32)
    table, status = _twin(record["seq"], prob, start, strand, record["segments"], record["n_tx"], 129)
    assert status == 0
    table.setflags(write=False)
    return prob, start, strand, table


# ---- 1. the kernel against the twin ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n_rep", [1, 3, 4, 5, 63, 64, 65, 129])
def test_kernel_equals_the_twin_on_the_record(record, record_twin, n_rep):
    prob, start, strand, want = record_twin
    table, status = _kernel(record["genome"], prob, start, strand, record["segments"], record["n_tx"], n_rep, pad=n_rep % 3)
    got = _host(table, record["n_tx"], n_rep)
    assert status == 0 and got.tobytes() == np.ascontiguousarray(want[:, :, :n_rep]).tobytes()
    assert (want[:, :, :n_rep].sum(axis=(0, 2)) > 0).all() or n_rep < 3                # every bin is reached


def test_float64_no_strand_other_code_other_order(record):
    prob, start, _, _ = D.rows(record["seq"], seed=7, dtype=np.float64)
    kw = dict(aa=D.CODE.replace("W", "*").replace("M", "I"), alt_order="TGC,TGA,TCA,GCA")
    table, status = _kernel(record["genome"], prob, start, None, record["segments"], record["n_tx"], 6, **kw)
    want, _ = _twin(record["seq"], prob, start, None, record["segments"], record["n_tx"], 6, **kw)
    plain, _ = _twin(record["seq"], prob, start, None, record["segments"], record["n_tx"], 6)
    assert status == 0 and _host(table, record["n_tx"], 6).tobytes() == want.tobytes() != plain.tobytes()
    table, status = _kernel(record["genome"], prob, start, None, record["segments"], record["n_tx"], 6)
    assert status == 0 and _host(table, record["n_tx"], 6).tobytes() == plain.tobytes()


# ---- 2. the loop bounds ---------------------------------------------------------------------------------------------------------------------
def test_past_the_chunk_length_the_grid_and_the_scan_threads():
    """Transcripts of two-base exons, enough of them for more units than the draw grid has waves (at 64 replicates or fewer a chunk is one
    unit) and more segments than the scan workgroup has threads; one one-exon transcript over a stretch with 2 rows per base (equal
    starts on both strands) repeated until the segment holds more than two chunks and a partial one.  The bounds are read from the
    getters."""
    from mural_amd import tables
    lib = _lib().lib()
    chunk, waves, scan = int(lib.mural_simulate_chunk_rows()), int(lib.mural_simulate_grid_waves()), int(lib.mural_simulate_scan_threads())
    n_seg = max(waves, 2 * scan) + 88
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
    strand = (np.arange(n) & 1).astype(np.uint8)
    assert len(segments["seg_b0"]) > waves and len(segments["seg_b0"]) > scan and 292 * repeat > 2 * chunk
    table, status = _kernel(_genome(seq), prob, start, strand, segments, len(names), 5)
    want, _ = _twin(seq, prob, start, strand, segments, len(names), 5)
    assert status == 0 and _host(table, len(names), 5).tobytes() == want.tobytes() and want[-1].sum() > chunk


@pytest.mark.parametrize("n", [1, 63, 64, 65, 1023, 1024, 1025])
def test_row_counts_around_a_tile_and_a_chunk_inside_one_segment(n):
    from mural_amd import tables
    rng = np.random.default_rng(n)
    seq = "".join(rng.choice(list("ACGT"), size=400))
    names, meta, segments = tables.read_transcripts(io.StringIO(D.bed12("chr1", "t", "+", [(10, 130), (140, 391)]) + "\n"))
    start = np.sort(rng.integers(140, 391, size=n)).astype(np.int64)
    prob = rng.dirichlet(np.ones(4), size=n).astype(np.float32)
    strand = rng.integers(0, 2, size=n).astype(np.uint8)
    table, status = _kernel(_genome(seq), prob, start, strand, segments["chr1"], 1, 66)
    want, _ = _twin(seq, prob, start, strand, segments["chr1"], 1, 66)
    assert status == 0 and _host(table, 1, 66).tobytes() == want.tobytes()


def test_more_replicate_blocks_than_one_unit_holds():
    """1030 replicates are 17 blocks of 64: a unit holds 16 of them, so a chunk becomes two units, the second with a partial block."""
    from mural_amd import tables
    rng = np.random.default_rng(5)
    seq = "".join(rng.choice(list("ACGT"), size=200))
    names, meta, segments = tables.read_transcripts(io.StringIO(D.bed12("chr1", "t", "-", [(10, 70), (80, 191)]) + "\n"))
    start = np.arange(5, 195, dtype=np.int64)
    prob = rng.dirichlet(np.ones(4), size=len(start)).astype(np.float32)
    table, status = _kernel(_genome(seq), prob, start, None, segments["chr1"], 1, 1030)
    want, _ = _twin(seq, prob, start, None, segments["chr1"], 1, 1030)
    assert status == 0 and _host(table, 1, 1030).tobytes() == want.tobytes() and want[:, :, 1024:].any()


# ---- 3. the identity on the device ------------------------------------------------------------------------------------------------------------
def test_device_identity_with_the_two_existing_entries(record):
    """For three replicates: the table's column equals the label counts of mural_summary_conseq_rows run with `label` set to that
    replicate's mural_simulate_rows labels, scattered back to the rows."""
    from mural_amd import tables
    from mural_amd.summaries import conseq_rows_device
    L, dev = _lib(), _dev()
    lib = L.lib()
    prob, start, strand, _ = D.rows(record["seq"], seed=9, dtype=np.float32, extra=0)      # distinct starts: a list entry names its row
    n, n_tx, R = len(start), record["n_tx"], 70
    table, status = _kernel(record["genome"], prob, start, strand, record["segments"], n_tx, R)
    got = _host(table, n_tx, R)
    prob_d, start_d, strand_d = _up(prob), _up(start), _up(strand)
    for rep in (0, 6, 69):
        out = (torch.empty(n, dtype=torch.int64, device=dev), torch.empty(n, dtype=torch.uint8, device=dev), torch.empty(n, dtype=torch.uint8, device=dev))
        count, st = torch.zeros(1, dtype=torch.int64, device=dev), torch.zeros(1, dtype=torch.int32, device=dev)
        s = L.MuralSimulateRows()
        s.prob, s.prob_f64, s.prob_stride, s.n_class = prob_d.data_ptr(), 0, 4, 4
        s.start, s.strand, s.n = start_d.data_ptr(), strand_d.data_ptr(), n
        s.chrom_key, s.replicate, s.seed = KEY, rep, SEED
        s.out_start, s.out_strand, s.out_label, s.count, s.status = out[0].data_ptr(), out[1].data_ptr(), out[2].data_ptr(), count.data_ptr(), st.data_ptr()
        need = int(lib.mural_simulate_rows_workspace_bytes(n))
        ws = torch.empty(need // 8 + 1, dtype=torch.int64, device=dev)
        L.check(lib.mural_simulate_rows(C.byref(s), ws.data_ptr(), ws.numel() * 8, L.current_stream_ptr(dev)))
        m = int(count.item())
        label = torch.zeros(n, dtype=torch.int64, device=dev)
        label[torch.searchsorted(start_d, out[0][:m])] = out[2][:m].to(torch.int64)
        acc = _acc(n_tx, dev)
        conseq_rows_device(acc, "chr", record["segments"], n_tx, tables.check_codon_table(None), tables.check_alt_order(None),
                           record["genome"].as_struct(dev), dev, prob=prob_d.data_ptr(), prob_f64=0, prob_stride=4, start=start_d.data_ptr(),
                           strand=strand_d.data_ptr(), label=label.data_ptr(), label_kind=2, n=n)
        observed = acc["table"].cpu().numpy().view(np.uint64).reshape(n_tx, 5, 3)[:, :, 0]
        assert int(acc["status"].item()) == 0 and m > 0 and (got[:, :, rep] == observed).all(), rep


# ---- 4. calls ---------------------------------------------------------------------------------------------------------------------------------
def test_calls_accumulate_and_parts_give_the_one_call_table(record, record_twin):
    prob, start, strand, want = record_twin
    for parts in (2, 7):
        table = None
        for rows in np.array_split(np.arange(len(start)), parts):
            table, status = _kernel(record["genome"], prob[rows], start[rows], strand[rows], record["segments"], record["n_tx"], 65, into=table)
            assert status == 0
        assert _host(table, record["n_tx"], 65).tobytes() == np.ascontiguousarray(want[:, :, :65]).tobytes(), parts


def test_status_bits_and_calls_that_launch_nothing(record):
    prob, start, strand, _ = D.rows(record["seq"], seed=3, dtype=np.float32)
    n_tx = record["n_tx"]
    table, status = _kernel(record["genome"], prob[:0], start[:0], strand[:0], record["segments"], n_tx, 4, fill=POISON)
    assert status == 0 and (table == POISON).all()
    none = {key: v[:0] if key.startswith("seg_") else v for key, v in record["segments"].items()}
    bad = prob.copy()
    bad[70, 2], bad[71, 0], bad[72, 1] = np.nan, np.nan, 1.5       # class 0 is never read; 1.5 is clamped
    table, status = _kernel(record["genome"], bad, start, strand, none, n_tx, 4, fill=POISON)      # no segments: only the rows are checked
    assert status == 8 and (table == POISON).all()
    first = start.copy()
    first[0] = -4
    table, status = _kernel(record["genome"], bad, first, strand, record["segments"], n_tx, 4)
    want, want_status = _twin(record["seq"], bad, first, strand, record["segments"], n_tx, 4)
    assert status == want_status == 9 and _host(table, n_tx, 4).tobytes() == want.tobytes()
    swapped = start.copy()
    swapped[100], swapped[101] = start[101] + 1, start[100]
    assert swapped[100] > swapped[101]
    assert _kernel(record["genome"], prob, swapped, strand, record["segments"], n_tx, 4)[1] == 4


def test_a_segment_of_a_transcript_out_of_range_is_skipped(record):
    prob, start, strand, _ = D.rows(record["seq"], seed=3, dtype=np.float32)
    n_tx = record["n_tx"]
    atg = record["names"].index("atg")                           # a one-segment transcript
    s = int(np.nonzero(np.asarray(record["segments"]["seg_tx"]) == atg)[0][0])
    seg_tx = np.asarray(record["segments"]["seg_tx"]).copy()
    seg_tx[s] = n_tx
    table, status = _kernel(record["genome"], prob, start, strand, dict(record["segments"], seg_tx=seg_tx), n_tx, 4)
    want, _ = _twin(record["seq"], prob, start, strand, record["segments"], n_tx, 4)
    assert want[atg].any()
    want[atg] = 0
    assert status == 0 and _host(table, n_tx, 4).tobytes() == want.tobytes()


# ---- 5. refusals ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("what", ["n_class", "n_rep_0", "n_rep_above", "n", "n_segments", "alt_order", "workspace"])
def test_refusals_leave_the_table_untouched(record, what):
    prob, start, strand, _ = D.rows(record["seq"], seed=3, dtype=np.float32)

    def edit(s):
        if what == "n_class":
            s.n_class = 5
        elif what == "n_rep_0":
            s.n_rep = 0
        elif what == "n_rep_above":
            s.n_rep = (1 << 20) + 1
        elif what == "n":
            s.n = (1 << 31) + 1
        elif what == "n_segments":
            s.n_segments = (1 << 22) + 1
        elif what == "alt_order":
            s.alt_order[2][1] = 2

    table, status = _kernel(record["genome"], prob, start, strand, record["segments"], record["n_tx"], 4, fill=POISON, edit=edit,
                            rc=3 if what == "workspace" else 1, short_ws=what == "workspace")
    assert status == 0 and (table == POISON).all()


# ---- 6. the sink's routes ---------------------------------------------------------------------------------------------------------------------
def test_sink_behind_a_single_focal_regions_run_equals_the_twin(files, snv_model, monkeypatch):  # noqa: F811
    from mural_amd import predict as P
    from mural_amd import tables
    from mural_amd.summaries import simulate_chrom_key, simulate_conseq_host
    from tests.test_gpu_region_labels import RECORDS
    d, fa = files
    tx = tables.read_transcripts(io.StringIO(_transcripts_over(RECORDS, REGIONS)))
    fwd = _forward(snv_model, fa)
    counts = []
    for tag, part_rows in (("cs_a", 1 << 20), ("cs_b", 700)):      # one and several parts per chromosome
        monkeypatch.setattr(P, "_ALIGNED_PART_ROWS", part_rows)
        keep = _Keep()
        sink = P.SummarySink(str(d / tag), transcripts=tx, genome=fwd.genome, transcript_labels=False, simulate=7, simulate_seed=21,
                             simulate_transcripts=True)
        assert P.predict_regions_sharded(fwd, REGIONS, "A", sink=P.TeeSink(keep, sink), collect=False) > 0
        counts.append(sink.consequence_simulation_counts())
    want = None
    for chrom, parts in keep.rows.items():
        prob, start, label, strand = (np.concatenate([p[i] for p in parts]) for i in range(4))
        if chrom in tx[2]:
            want, status = simulate_conseq_host(RECORDS[chrom], prob, start, strand, tx[2][chrom], len(tx[0]), simulate_chrom_key(chrom), 21, 7,
                                                into=want)
            assert status == 0
    assert counts[0].tobytes() == counts[1].tobytes() == want.tobytes() and want.sum() > 100
    assert (d / "cs_a.consequence.sim.tsv").read_bytes() == (d / "cs_b.consequence.sim.tsv").read_bytes()
    assert (d / "cs_a.consequence.sim.tsv").read_text().splitlines()[1].split("\t")[2] == "NA"


def test_table_route_and_command_line(files, snv_model, tmp_path):  # noqa: F811
    """The written table through ``tables.simulate_consequence_table``: the twin on the table's four-digit probabilities; the command
    line writes the sink's file."""
    from mural_amd import predict as P
    from mural_amd import tables
    from mural_amd.model import nn_utils
    from mural_amd.summaries import simulate_chrom_key, simulate_conseq_host
    from tests.test_gpu_region_labels import RECORDS
    d, fa = files
    regions = {"chrA": REGIONS["chrA"][:1]}
    bed = tmp_path / "tx.bed"
    bed.write_text(_transcripts_over(RECORDS, regions, seed=3))
    tx = tables.read_transcripts(str(bed))
    fwd = _forward(snv_model, fa)
    out = str(tmp_path / "t.tsv")
    sink = P.SummarySink(str(tmp_path / "s"), transcripts=tx, genome=fwd.genome, simulate=6, simulate_seed=4, simulate_transcripts=True)
    P.predict_regions_sharded(fwd, regions, "A", sink=P.TeeSink(P.TsvSink(out), sink), collect=False)
    names, counts, observed, expected = tables.simulate_consequence_table(out, tx, fa, 6, 4, chunk_bytes=16 << 10)      # several chunks
    rows = [ln.split("\t") for ln in open(out).read().splitlines()[1:]]
    start = np.array([int(r[1]) for r in rows], np.int64)
    strand = np.array([r[3] == "-" for r in rows], np.uint8)
    prob = np.array([[float(v) for v in r[-4:]] for r in rows], np.float64)
    want, status = simulate_conseq_host(RECORDS["chrA"], prob, start, strand, tx[2]["chrA"], len(tx[0]), simulate_chrom_key("chrA"), 4, 6)
    assert status == 0 and names == tx[0] and counts.tobytes() == want.tobytes() and want.sum() > 50
    assert np.array_equal(observed, sink.result()["consequence_simulation"][2])

    class Args:
        pred_file, transcripts, ref_genome, out_prefix, simulate, seed = out, str(bed), fa, str(tmp_path / "calc"), 6, 4
    tables.run_simulate_consequence_calc(Args)
    assert len((tmp_path / "calc.consequence.sim.tsv").read_text().splitlines()) == 1 + 4 * len(names)
    ckpt = str(tmp_path / "model")
    nn_utils.save_model(snv_model[0], None, snv_model[1], ckpt)
    spec = importlib.util.spec_from_file_location("predict_files", os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))),
                                                                                  "tools", "predict_files.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    region_args = [a for lo, hi in regions["chrA"] for a in ("--regions", f"chrA:{lo + 1}-{hi}")]
    mod.main([ckpt, fa, "--no-table", *region_args, "--focal", "A", "--summary", str(tmp_path / "cli"), "--transcripts", str(bed), "--simulate", "6",
              "--seed", "4", "--simulate_consequences"])
    cli = [ln.split("\t") for ln in (tmp_path / "cli.consequence.sim.tsv").read_text().splitlines()]
    api = [ln.split("\t") for ln in (tmp_path / "s.consequence.sim.tsv").read_text().splitlines()]
    # the command line's rows carry no labels (--regions without --mutations): the simulated columns are the sink's
    assert cli[0] == api[0] and [r[:2] + r[3:7] for r in cli[1:]] == [r[:2] + r[3:7] for r in api[1:]] and cli[1][2] == "NA"
