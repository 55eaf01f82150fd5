"""The simulated null of the structure table on the device (csrc/simulate_txstruct.hip: mural_simulate_txstruct_rows;
mural_amd.predict.SummarySink(simulate_structure=True); mural_amd.tables.simulate_structure_table): every case goes through the entry
point and is compared for EQUALITY with the numpy twin ``simulate_txstruct_host`` -- the record of tests/_txstruct_data.py at replicate
counts around a Philox call, a block of 64 and two blocks, the three loop bounds read from the simulation's getters, row counts around a
tile and a chunk inside an intron item and a CDS item that holds codon 0, short gaps, a first codon over a junction on '-', the two
identities with the existing entries on the device, calls that accumulate or launch nothing, every refusal, the skipped items, and the
sink's routes: a single-focal regions run, the table route and the command line."""
import ctypes as C
import importlib.util
import io
import os

import numpy as np
import pytest
import torch

from tests import _conseq_data as D
from tests import _txstruct_data as S
from tests.test_gpu_region_labels import REGIONS, _forward, files, snv_model  # noqa: F401  (fixtures)
from tests.test_gpu_summary_conseq import _Keep, _dev, _genome, _lib, _transcripts_over, _up

pytestmark = pytest.mark.gpu

KEY, SEED = 0xC0FFEE11, (3 << 33) + 5
POISON = 0x07070707
SEG_KEYS = ("seg_b0", "seg_b1", "seg_cds0", "seg_tx", "seg_prev", "seg_next")
FEAT_KEYS = ("feat_b0", "feat_b1", "feat_tx", "feat_kind", "feat_seg")


def _kernel(genome, prob, start, strand, segments, features, n_tx, n_rep, aa=None, alt_order=None, into=None, pad=0, fill=0, rc=0, edit=None,
            short_ws=False):
    """One mural_simulate_txstruct_rows call on device copies of the arrays: (table int32 [n_tx * 9 * n_rep] on the device, status)."""
    from mural_amd import tables
    L, dev = _lib(), _dev()
    lib = L.lib()
    if pad:
        prob = np.concatenate([prob, np.full((len(prob), pad), 0.25, prob.dtype)], axis=1)
    prob_d, start_d = _up(prob), _up(start)
    strand_d = None if strand is None else _up(strand)
    feat_d = tuple(_up(np.ascontiguousarray(features[key])) for key in FEAT_KEYS)
    seg_d = None if segments is None else tuple(_up(np.ascontiguousarray(segments[key])) for key in SEG_KEYS)
    tx_d = (_up(np.ascontiguousarray(features["tx_strand"])), _up(np.ascontiguousarray(features["tx_cds_len"])))
    table = torch.full((max(n_tx * 9 * n_rep, 1),), fill, dtype=torch.int32, device=dev) if into is None else into
    status = torch.zeros(1, dtype=torch.int32, device=dev)
    s = L.MuralSimulateTxstructRows()
    g = genome.as_struct(dev)
    s.genome = C.pointer(g)
    s.prob, s.prob_f64, s.prob_stride, s.n_class = prob_d.data_ptr(), int(prob_d.dtype == torch.float64), prob_d.stride(0) if prob_d.shape[0] else 4, 4
    s.start, s.strand, s.n = start_d.data_ptr(), None if strand_d is None else strand_d.data_ptr(), int(start_d.shape[0])
    s.chrom_key, s.n_rep, s.seed = KEY, n_rep, SEED
    if seg_d is not None and seg_d[0].shape[0]:
        s.seg_b0, s.seg_b1, s.seg_cds0, s.seg_tx, s.seg_prev, s.seg_next = (x.data_ptr() for x in seg_d)
        s.n_segments = int(seg_d[0].shape[0])
    s.feat_b0, s.feat_b1, s.feat_tx, s.feat_kind, s.feat_seg = (x.data_ptr() for x in feat_d)
    s.n_features, s.n_transcripts = int(feat_d[0].shape[0]), n_tx
    s.tx_strand, s.tx_cds_len = tx_d[0].data_ptr(), tx_d[1].data_ptr()
    C.memmove(s.aa, np.ascontiguousarray(tables.check_codon_table(aa), np.uint8).ctypes.data, 64)
    C.memmove(s.alt_order, np.ascontiguousarray(tables.check_alt_order(alt_order), np.uint8).ctypes.data, 12)
    s.table, s.status = table.data_ptr(), status.data_ptr()
    if edit:
        edit(s)
    need = int(lib.mural_simulate_txstruct_workspace_bytes(int(feat_d[0].shape[0])))
    assert need >= 24 * int(feat_d[0].shape[0])      # (the arena aligns each array)
    ws = torch.empty(need // 8 + 1, dtype=torch.int64, device=dev)
    got = lib.mural_simulate_txstruct_rows(C.byref(s), ws.data_ptr(), need - 8 if short_ws else ws.numel() * 8, L.current_stream_ptr(dev))
    assert got == rc
    torch.cuda.synchronize()
    return table, int(status.item())


def _host(table, n_tx, n_rep):
    return table.cpu().numpy().view(np.uint32)[:n_tx * 9 * n_rep].reshape(n_tx, 9, n_rep)


def _twin(seq, prob, start, strand, segments, features, n_tx, n_rep, **kw):
    from mural_amd.summaries import simulate_txstruct_host
    return simulate_txstruct_host(seq, prob, start, strand, segments, features, n_tx, KEY, SEED, n_rep, **kw)


def _read(text):
    from mural_amd import tables
    names, meta, segments, features = tables.read_transcript_structure(io.StringIO(text))
    return names, segments.get("chr1"), features["chr1"]


@pytest.fixture(scope="module")
def record():
    from mural_amd import tables
    seq, text, names = S.build()
    tx = tables.read_transcript_structure(io.StringIO(text))
    return dict(seq=seq, text=text, names=names, meta=tx[1], tx=tx, segments=tx[2]["chr1"], features=tx[3]["chr1"], genome=_genome(seq),
                n_tx=len(names))


@pytest.fixture(scope="module")
def record_twin(record):
    """The twin's table of the record's float32 rows at 129 replicates, computed once: the cases at fewer replicates read its columns
    (replicate r does not depend on the replicate count)."""
    prob, start, strand, _ = S.rows(record["seq"], seed=1, dtype=np.float32)
    table, status = _twin(record["seq"], prob, start, strand, record["segments"], record["features"], record["n_tx"], 129)
    assert status == 0
    table.setflags(write=False)
    return prob, start, strand, table


def _both(record, prob, start, strand, n_rep, segments=None, features=None, **kw):
    segments, features = segments or record["segments"], features or record["features"]
    table, status = _kernel(record["genome"], prob, start, strand, segments, features, record["n_tx"], n_rep, **kw)
    return _host(table, record["n_tx"], n_rep), status


# ---- 1. the kernel against the twin ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n_rep", [1, 3, 4, 5, 63, 64, 65, 129])
def test_kernel_equals_the_twin_on_the_record(record, record_twin, n_rep):
    prob, start, strand, want = record_twin
    got, status = _both(record, prob, start, strand, n_rep, pad=n_rep % 3)
    assert status == 0 and got.tobytes() == np.ascontiguousarray(want[:, :, :n_rep]).tobytes()
    assert len(record["features"]["feat_b0"]) > 600 and record["n_tx"] > 60 and len(start) > 3000
    assert (want[:, :, :n_rep].sum(axis=(0, 2)) > 0).all() or n_rep < 63                # every bin is reached


def test_float64_no_strand_other_code_other_order(record):
    prob, start, _, _ = S.rows(record["seq"], seed=7, dtype=np.float64)
    kw = dict(aa=D.CODE.replace("W", "*").replace("M", "I"), alt_order="TGC,TGA,TCA,GCA")
    args = (record["seq"], prob, start, None, record["segments"], record["features"], record["n_tx"], 6)
    got, status = _both(record, prob, start, None, 6, **kw)
    want, plain = _twin(*args, **kw)[0], _twin(*args)[0]
    assert status == 0 and got.tobytes() == want.tobytes() != plain.tobytes()
    got, status = _both(record, prob, start, None, 6)
    assert status == 0 and got.tobytes() == plain.tobytes()


# ---- 2. the loop bounds ---------------------------------------------------------------------------------------------------------------------
def test_past_the_chunk_length_the_grid_and_the_scan_threads():
    """Transcripts of two-base exons and three-base introns, enough of them for more units than the draw grid has waves (at 64
    replicates or fewer a chunk is one unit) and more items than the scan workgroup has threads; one two-exon transcript whose intron's
    rows are repeated until the item holds more than two chunks and a partial one.  The bounds are read from the getters."""
    lib = _lib().lib()
    chunk, waves, scan = int(lib.mural_simulate_chunk_rows()), int(lib.mural_simulate_grid_waves()), int(lib.mural_simulate_scan_threads())
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
    names, segments, features = _read("\n".join(lines) + "\n")
    repeat = -(-(2 * chunk + 77) // 292)
    start = np.sort(np.concatenate([np.arange(len(seq)), np.repeat(np.arange(3, 295), repeat - 1)])).astype(np.int64)
    n = len(start)
    prob = rng.dirichlet(np.ones(4), size=n).astype(np.float32)
    strand = (np.arange(n) & 1).astype(np.uint8)
    two_base = int((features["feat_b1"] - features["feat_b0"] == 2).sum())
    assert two_base > waves and two_base > scan and 292 * repeat > 2 * chunk and (292 * repeat) % chunk
    table, status = _kernel(_genome(seq), prob, start, strand, segments, features, len(names), 5)
    want, _ = _twin(seq, prob, start, strand, segments, features, len(names), 5)
    assert status == 0 and _host(table, len(names), 5).tobytes() == want.tobytes() and want[-1].sum() > chunk
    assert want[-1, 3].any() and want[-1, 4].any() and want[-1, 6].any()


@pytest.mark.parametrize("where", ["intron", "cds"])
@pytest.mark.parametrize("n", [1, 63, 64, 65, 1023, 1024, 1025])
def test_row_counts_around_a_tile_and_a_chunk_inside_one_item(n, where):
    """The rows fall in one item: the intron [130, 140) -- donor, acceptor and the bases between -- or the first CDS part [10, 130),
    which holds codon 0."""
    rng = np.random.default_rng(n)
    seq = "".join(rng.choice(list("ACGT"), size=400))
    names, segments, features = _read(D.bed12("chr1", "t", "+", [(10, 130), (140, 391)]) + "\n")
    lo, hi = (130, 140) if where == "intron" else (10, 130)
    start = np.sort(np.concatenate([rng.integers(lo, hi, size=max(n - 3, 0)), np.arange(lo, lo + 3)[:n]])).astype(np.int64)[:n]
    prob = rng.dirichlet(np.ones(4), size=n).astype(np.float32)
    strand = rng.integers(0, 2, size=n).astype(np.uint8)
    table, status = _kernel(_genome(seq), prob, start, strand, segments, features, 1, 66)
    want, _ = _twin(seq, prob, start, strand, segments, features, 1, 66)
    assert status == 0 and _host(table, 1, 66).tobytes() == want.tobytes() and want.any()
    assert not want[0, [0, 1, 2, 5] + ([7, 8] if where == "intron" else [3, 4, 6])].any()


def test_more_replicate_blocks_than_one_unit_holds():
    """1030 replicates are 17 blocks of 64: a unit holds 16 of them, so a chunk becomes two units, the second with a partial block."""
    rng = np.random.default_rng(5)
    seq = "".join(rng.choice(list("ACGT"), size=200))
    names, segments, features = _read(D.bed12("chr1", "t", "-", [(10, 70), (80, 191)], (20, 150)) + "\n")
    start = np.arange(5, 195, dtype=np.int64)
    prob = rng.dirichlet(np.ones(4), size=len(start)).astype(np.float32)
    table, status = _kernel(_genome(seq), prob, start, None, segments, features, 1, 1030)
    want, _ = _twin(seq, prob, start, None, segments, features, 1, 1030)
    assert status == 0 and _host(table, 1, 1030).tobytes() == want.tobytes() and want[:, :, 1024:].any()


def test_gaps_of_three_and_four_bases_and_a_first_codon_over_a_junction():
    text = (D.bed12("chr1", "gaps", "+", [(10, 16), (19, 25), (29, 35)]) + "\n" +
            D.bed12("chr1", "junction", "-", [(50, 60), (70, 72), (80, 81)], (52, 81)) + "\n")      # codon 0: 80, 71, 70 on '-'
    seq = "ACGTTGCATG" * 5 + "ACGTACGTAC" + "GCAACGTACG" + "CACGTACGTA" + "TTCGA"                 # 80, 71, 70 read T, A, C: ATG on '-'
    assert seq[80] == "T" and seq[70:72] == "CA"
    names, segments, features = _read(text)
    start = np.repeat(np.arange(0, len(seq)), 2).astype(np.int64)
    strand = (np.arange(len(start)) & 1).astype(np.uint8)
    rng = np.random.default_rng(2)
    prob = rng.dirichlet(np.ones(4), size=len(start)).astype(np.float32)
    prob[:, 0] = 0                                                   # (class 0 is never read: nearly every draw is a mutation)
    table, status = _kernel(_genome(seq), prob, start, strand, segments, features, 2, 70)
    want, _ = _twin(seq, prob, start, strand, segments, features, 2, 70)
    assert status == 0 and _host(table, 2, 70).tobytes() == want.tobytes()
    assert want[0, 6].any() and want[0, 3].any() and want[0, 4].any() and want[1, 7].any() and want[1, 8].any()
    certain = np.zeros((len(start), 4), np.float32)
    certain[:, 1] = 1
    table, status = _kernel(_genome(seq), certain, start, strand, segments, features, 2, 2)
    got = _host(table, 2, 2)
    assert got[0, :, 0].tolist() == [0, 0, 0, 4, 4, 0, 6, got[0, 7, 0], 36 - got[0, 7, 0]]      # the gap of 3 is all intron, the gap of 4 all sites
    assert got[1, 7, 0] == 6                                                                   # ATG over two junctions: 3 bases x 2 rows


# ---- 3. the identities on the device ----------------------------------------------------------------------------------------------------------
def test_device_identity_with_simulate_rows_and_summary_txstruct_rows(record):
    """(a) For three replicates: the table's column equals the label counts of mural_summary_txstruct_rows run with `label` set to that
    replicate's mural_simulate_rows labels, scattered back to the rows."""
    from mural_amd import tables
    from mural_amd.summaries import txstruct_rows_device
    L, dev = _lib(), _dev()
    lib = L.lib()
    prob, start, strand, _ = S.rows(record["seq"], seed=9, dtype=np.float32, extra=0)      # distinct starts: a list entry names its row
    n, n_tx, R = len(start), record["n_tx"], 70
    got, status = _both(record, prob, start, strand, R)
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
        acc = dict(table=torch.zeros(n_tx * 27, dtype=torch.int64, device=dev), rows=torch.zeros(n_tx * 2, dtype=torch.int64, device=dev),
                   status=torch.zeros(1, dtype=torch.int32, device=dev), features={}, ws=None, conseq=dict(segments={}))
        txstruct_rows_device(acc, acc["conseq"], "chr", record["segments"], record["features"], n_tx, tables.check_codon_table(None),
                             tables.check_alt_order(None), record["genome"].as_struct(dev), dev, prob=prob_d.data_ptr(), prob_f64=0, prob_stride=4,
                             start=start_d.data_ptr(), strand=strand_d.data_ptr(), label=label.data_ptr(), label_kind=2, n=n)
        observed = acc["table"].cpu().numpy().view(np.uint64).reshape(n_tx, 9, 3)[:, :, 0]
        assert int(acc["status"].item()) == 0 and m > 0 and (got[:, :, rep] == observed).all(), rep


def test_device_identity_with_simulate_conseq_rows(record, record_twin):
    """(b) Bins 7 + 8 add up to the five bins of mural_simulate_conseq_rows at the same key, seed and replicate."""
    from tests import test_gpu_simulate_conseq as Q
    assert (Q.KEY, Q.SEED) == (KEY, SEED)
    prob, start, strand, _ = record_twin
    got, status = _both(record, prob, start, strand, 65)
    table, conseq_status = Q._kernel(record["genome"], prob, start, strand, record["segments"], record["n_tx"], 65)
    conseq = Q._host(table, record["n_tx"], 65).astype(np.int64)
    assert status == conseq_status == 0 and conseq.any()
    assert (got[:, 7].astype(np.int64) + got[:, 8] == conseq.sum(axis=1)).all()


# ---- 4. calls ---------------------------------------------------------------------------------------------------------------------------------
def test_calls_accumulate_and_parts_give_the_one_call_table(record, record_twin):
    prob, start, strand, want = record_twin
    for parts in (2, 7):
        table = None
        for rows in np.array_split(np.arange(len(start)), parts):
            table, status = _kernel(record["genome"], prob[rows], start[rows], strand[rows], record["segments"], record["features"], record["n_tx"],
                                    65, into=table)
            assert status == 0
        assert _host(table, record["n_tx"], 65).tobytes() == np.ascontiguousarray(want[:, :, :65]).tobytes(), parts


def test_status_bits_and_calls_that_launch_nothing(record):
    prob, start, strand, _ = S.rows(record["seq"], seed=3, dtype=np.float32)
    n_tx = record["n_tx"]
    args = (record["segments"], record["features"], n_tx, 4)
    table, status = _kernel(record["genome"], prob[:0], start[:0], strand[:0], *args, fill=POISON)
    assert status == 0 and (table == POISON).all()
    none = {key: v[:0] if key.startswith("feat_") else v for key, v in record["features"].items()}
    bad = prob.copy()
    bad[70, 2], bad[71, 0], bad[72, 1] = np.nan, np.nan, 1.5       # class 0 is never read; 1.5 is clamped
    table, status = _kernel(record["genome"], bad, start, strand, record["segments"], none, n_tx, 4, fill=POISON)      # no items: only the rows are checked
    assert status == 8 and (table == POISON).all()
    first = start.copy()
    first[0] = -4
    table, status = _kernel(record["genome"], bad, first, strand, *args)
    want, want_status = _twin(record["seq"], bad, first, strand, *args)
    assert status == want_status == 9 and _host(table, n_tx, 4).tobytes() == want.tobytes()
    swapped = start.copy()
    swapped[100], swapped[101] = start[101] + 1, start[100]
    assert swapped[100] > swapped[101]
    assert _kernel(record["genome"], prob, swapped, strand, *args)[1] == 4


def test_a_chromosome_without_cds(record):
    """Items and no segments: n_segments == 0 is legal."""
    names, segments, features = _read(D.bed12("chr1", "nc", "-", [(5, 12), (20, 30)], (5, 5)) + "\n")
    assert segments is None
    seq = "ACGT" * 10
    start = np.arange(40, dtype=np.int64)
    prob = np.full((40, 4), 0.25, np.float32)
    table, status = _kernel(_genome(seq), prob, start, None, None, features, 1, 8)
    want, _ = _twin(seq, prob, start, None, None, features, 1, 8)
    assert status == 0 and _host(table, 1, 8).tobytes() == want.tobytes() and want[0, 2].any() and want[0, 5].any() and want[0, 6].any()


def test_skipped_items(record):
    """A CDS item whose feat_seg is out of range or names another segment, an item of an unknown kind and an item whose transcript is out
    of range add nothing; the twin of the record without those items' rows is the answer."""
    prob, start, strand, _ = S.rows(record["seq"], seed=3, dtype=np.float32)
    n_tx, feats = record["n_tx"], record["features"]
    want, _ = _twin(record["seq"], prob, start, strand, record["segments"], feats, n_tx, 4)
    t = record["names"].index("one_exon_p")                              # items [1000,1020) utr5, [1020,1081) cds, [1081,1100) utr3
    mine = np.nonzero(np.asarray(feats["feat_tx"]) == t)[0]
    kinds = np.asarray(feats["feat_kind"])[mine].tolist()
    assert sorted(kinds) == [0, 1, 5] and want[t, 0].any() and want[t, 1].any() and want[t, 8].any()
    cds, utr5, utr3 = (int(mine[kinds.index(k)]) for k in (5, 0, 1))
    other_seg = int((np.asarray(feats["feat_seg"])[cds] + 1) % len(record["segments"]["seg_b0"]))
    for key, at, value, gone in (("feat_seg", cds, len(record["segments"]["seg_b0"]), (7, 8)), ("feat_seg", cds, -1, (7, 8)),
                                 ("feat_seg", cds, other_seg, (7, 8)), ("feat_kind", utr5, 6, (0,)), ("feat_kind", utr3, 255, (1,)),
                                 ("feat_tx", utr5, n_tx, (0,)), ("feat_tx", utr3, -1, (1,))):
        arr = np.asarray(feats[key]).copy()
        arr[at] = value
        got, status = _both(record, prob, start, strand, 4, features=dict(feats, **{key: arr}))
        expect = want.copy()
        expect[t, list(gone)] = 0
        assert status == 0 and got.tobytes() == expect.tobytes(), (key, value)


# ---- 5. refusals ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("what", ["n_class", "n_rep_0", "n_rep_above", "n", "n_features", "n_segments", "alt_order", "workspace"])
def test_refusals_leave_the_table_untouched(record, what):
    prob, start, strand, _ = S.rows(record["seq"], seed=3, dtype=np.float32)

    def edit(s):
        if what == "n_class":
            s.n_class = 5
        elif what == "n_rep_0":
            s.n_rep = 0
        elif what == "n_rep_above":
            s.n_rep = (1 << 20) + 1
        elif what == "n":
            s.n = (1 << 31) + 1
        elif what == "n_features":
            s.n_features = (1 << 22) + 1
        elif what == "n_segments":
            s.n_segments = (1 << 22) + 1
        elif what == "alt_order":
            s.alt_order[2][1] = 2

    table, status = _kernel(record["genome"], prob, start, strand, record["segments"], record["features"], record["n_tx"], 4, fill=POISON,
                            edit=edit, rc=3 if what == "workspace" else 1, short_ws=what == "workspace")
    assert status == 0 and (table == POISON).all()


# ---- 6. the sink's routes ---------------------------------------------------------------------------------------------------------------------
def _sink_kw(tx, fwd, R, seed, **kw):
    return dict(transcripts=tx, genome=fwd.genome, simulate=R, simulate_seed=seed, simulate_transcripts=True, transcript_structure=True,
                simulate_structure=True, **kw)


def test_sink_behind_a_single_focal_regions_run_equals_the_twin(files, snv_model, monkeypatch):  # noqa: F811
    from mural_amd import predict as P
    from mural_amd import tables
    from mural_amd.summaries import simulate_chrom_key, simulate_conseq_host, simulate_lof_counts, simulate_txstruct_host
    from tests.test_gpu_region_labels import RECORDS
    d, fa = files
    tx = tables.read_transcript_structure(io.StringIO(_transcripts_over(RECORDS, REGIONS)))
    fwd = _forward(snv_model, fa)
    counts = []
    for tag, part_rows in (("ts_a", 1 << 20), ("ts_b", 700)):      # one and several parts per chromosome
        monkeypatch.setattr(P, "_ALIGNED_PART_ROWS", part_rows)
        keep = _Keep()
        sink = P.SummarySink(str(d / tag), **_sink_kw(tx, fwd, 7, 21, transcript_labels=False))
        assert P.predict_regions_sharded(fwd, REGIONS, "A", sink=P.TeeSink(keep, sink), collect=False) > 0
        counts.append(sink.structure_simulation_counts())
    want = conseq = None
    for chrom, parts in keep.rows.items():
        prob, start, label, strand = (np.concatenate([p[i] for p in parts]) for i in range(4))
        if chrom in tx[3]:
            want, status = simulate_txstruct_host(RECORDS[chrom], prob, start, strand, tx[2].get(chrom), tx[3][chrom], len(tx[0]),
                                                  simulate_chrom_key(chrom), 21, 7, into=want)
            assert status == 0
        if chrom in tx[2]:
            conseq, _ = simulate_conseq_host(RECORDS[chrom], prob, start, strand, tx[2][chrom], len(tx[0]), simulate_chrom_key(chrom), 21, 7,
                                             into=conseq)
    assert counts[0].tobytes() == counts[1].tobytes() == want.tobytes() and want.sum() > 100
    assert np.array_equal(sink.result()["structure_simulation"][2], simulate_lof_counts(conseq, want))
    for tail in ("consequence.structure.sim.tsv", "consequence.structure.tsv", "consequence.sim.tsv"):
        assert (d / f"ts_a.{tail}").read_bytes() == (d / f"ts_b.{tail}").read_bytes()
    lines = (d / "ts_a.consequence.structure.sim.tsv").read_text().splitlines()
    assert len(lines) == 1 + 10 * len(tx[0]) and lines[10].split("\t")[1:3] == ["lof", "NA"]


def test_table_route_and_command_line(files, snv_model, tmp_path):  # noqa: F811
    """The written table through ``tables.simulate_structure_table``: the twin on the table's four-digit probabilities; the command
    line writes the sink's file."""
    from mural_amd import predict as P
    from mural_amd import tables
    from mural_amd.model import nn_utils
    from mural_amd.summaries import simulate_chrom_key, simulate_conseq_host, simulate_lof_counts, simulate_txstruct_host
    from tests.test_gpu_region_labels import RECORDS
    d, fa = files
    regions = {"chrA": REGIONS["chrA"][:1]}
    bed = tmp_path / "tx.bed"
    bed.write_text(_transcripts_over(RECORDS, regions, seed=3))
    tx = tables.read_transcript_structure(str(bed))
    fwd = _forward(snv_model, fa)
    out = str(tmp_path / "t.tsv")
    sink = P.SummarySink(str(tmp_path / "s"), **_sink_kw(tx, fwd, 6, 4))
    P.predict_regions_sharded(fwd, regions, "A", sink=P.TeeSink(P.TsvSink(out), sink), collect=False)
    names, counts, lof, observed, expected = tables.simulate_structure_table(out, tx, fa, 6, 4, chunk_bytes=16 << 10)      # several chunks
    rows = [ln.split("\t") for ln in open(out).read().splitlines()[1:]]
    start = np.array([int(r[1]) for r in rows], np.int64)
    strand = np.array([r[3] == "-" for r in rows], np.uint8)
    prob = np.array([[float(v) for v in r[-4:]] for r in rows], np.float64)
    key = simulate_chrom_key("chrA")
    want, status = simulate_txstruct_host(RECORDS["chrA"], prob, start, strand, tx[2]["chrA"], tx[3]["chrA"], len(tx[0]), key, 4, 6)
    conseq, _ = simulate_conseq_host(RECORDS["chrA"], prob, start, strand, tx[2]["chrA"], len(tx[0]), key, 4, 6)
    assert status == 0 and names == tx[0] and counts.tobytes() == want.tobytes() and want.sum() > 50
    assert np.array_equal(lof, simulate_lof_counts(conseq, want)) and np.array_equal(observed, sink.result()["structure_simulation"][3])

    class Args:
        pred_file, transcripts, ref_genome, out_prefix, simulate, seed = out, str(bed), fa, str(tmp_path / "calc"), 6, 4
    tables.run_simulate_structure_calc(Args)
    assert len((tmp_path / "calc.consequence.structure.sim.tsv").read_text().splitlines()) == 1 + 10 * len(names)
    ckpt = str(tmp_path / "model")
    nn_utils.save_model(snv_model[0], None, snv_model[1], ckpt)
    spec = importlib.util.spec_from_file_location("predict_files", os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))),
                                                                                  "tools", "predict_files.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    region_args = [a for lo, hi in regions["chrA"] for a in ("--regions", f"chrA:{lo + 1}-{hi}")]
    mod.main([ckpt, fa, "--no-table", *region_args, "--focal", "A", "--summary", str(tmp_path / "cli"), "--transcripts", str(bed),
              "--transcript_structure", "--simulate", "6", "--seed", "4", "--simulate_consequences", "--simulate_structure"])
    cli = [ln.split("\t") for ln in (tmp_path / "cli.consequence.structure.sim.tsv").read_text().splitlines()]
    api = [ln.split("\t") for ln in (tmp_path / "s.consequence.structure.sim.tsv").read_text().splitlines()]
    # the command line's rows carry no labels (--regions without --mutations): the simulated columns are the sink's
    assert cli[0] == api[0] and [r[:2] + r[3:7] for r in cli[1:]] == [r[:2] + r[3:7] for r in api[1:]] and cli[1][2] == "NA"
