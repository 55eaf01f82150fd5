"""The simulated null of the INDEL structure table on the device (csrc/simulate_txindel.hip: mural_simulate_txindel_rows;
SummarySink(simulate_indel_structure=True)): every case goes through the entry point and is compared for EQUALITY, byte for byte, with
the numpy twin ``simulate_txindel_host`` -- both probability types, the strand given and NULL, the three kinds, both offsets, 2 / 5 / 8
classes, replicate counts around a block of 64 and past one unit's 16 blocks, the three loop bounds read from the simulation's getters,
long deletions over exons of three bases, the span's end and the chromosome's, broken links and skipped items, parts and permuted
equal starts, guard words around the table, the status bits, every refusal, the totals of the counted rows' draws, and in flight a
small UNet_Small over regions."""
import ctypes as C
import io

import numpy as np
import pytest
import torch

from tests import _conseq_data as D
from tests import _txindel_sim_data as X
from tests.test_gpu_regions import MAIN, R_LOCAL, files  # noqa: F401  (fixture)
from tests.test_gpu_summary_conseq import _Keep, _dev, _lib, _up

pytestmark = pytest.mark.gpu

POISON = 0x07070707
FEAT_KEYS = ("feat_b0", "feat_b1", "feat_tx", "feat_kind", "feat_seg")
SEG_KEYS = ("seg_b0", "seg_b1", "seg_cds0", "seg_tx")


def _kernel(prob, start, strand, k, segments, features, n_tx, kind, n_rep, off=1, spec=None, chrom_length=None, links=None, into=None, pad=0,
            fill=0, rc=0, edit=None, short_ws=False, guard=0):
    """One mural_simulate_txindel_rows call on device copies of the arrays: (table int32 [n_tx * 10 * n_rep] on the device, status); with
    `guard` the table sits between that many POISON words, returned as well."""
    from mural_amd import tables
    L, dev = _lib(), _dev()
    lib = L.lib()
    if pad:
        prob = np.concatenate([prob, np.full((len(prob), pad), 0.25, prob.dtype)], axis=1)
    prob_d, start_d = _up(prob), _up(start)
    strand_d = None if strand is None else _up(strand)
    links = tables.structure_links(features) if links is None else links
    feat_d = tuple(_up(np.ascontiguousarray(features[key])) for key in FEAT_KEYS) + tuple(_up(np.asarray(x, np.int32)) for x in links)
    seg_d = None if segments is None else tuple(_up(np.ascontiguousarray(segments[key])) for key in SEG_KEYS)
    tx_d = (_up(np.ascontiguousarray(features["tx_strand"])), _up(np.ascontiguousarray(features["tx_cds_len"])))
    cells = max(n_tx * 10 * n_rep, 1)
    whole = None
    if into is None:
        whole = torch.full((cells + 2 * guard,), POISON if guard else fill, dtype=torch.int32, device=dev)
        table = whole[guard:guard + cells]
        if guard:
            table.fill_(fill)
    else:
        table = into
    status = torch.zeros(1, dtype=torch.int32, device=dev)
    s = L.MuralSimulateTxindelRows()
    s.prob, s.prob_f64, s.prob_stride, s.n_class = prob_d.data_ptr(), int(prob_d.dtype == torch.float64), prob_d.stride(0) if prob_d.shape[0] else k, k
    s.start, s.strand, s.n = start_d.data_ptr(), None if strand_d is None else strand_d.data_ptr(), int(start_d.shape[0])
    s.chrom_key, s.n_rep, s.seed = X.KEY, n_rep, X.SEED
    s.kind, s.breakpoint_offset, s.chrom_length = kind, off, -1 if chrom_length is None else chrom_length
    for c, (lo, hi) in enumerate(tables.check_indel_lengths(spec, k).tolist()):
        s.class_len[c][0], s.class_len[c][1] = lo, hi
    if seg_d is not None and seg_d[0].shape[0]:
        s.seg_b0, s.seg_b1, s.seg_cds0, s.seg_tx = (x.data_ptr() for x in seg_d)
        s.n_segments = int(seg_d[0].shape[0])
    s.feat_b0, s.feat_b1, s.feat_tx, s.feat_kind, s.feat_seg, s.feat_prev, s.feat_next = (x.data_ptr() for x in feat_d)
    s.n_features, s.n_transcripts = int(feat_d[0].shape[0]), n_tx
    s.tx_strand, s.tx_cds_len = tx_d[0].data_ptr(), tx_d[1].data_ptr()
    s.table, s.status = table.data_ptr(), status.data_ptr()
    if edit:
        edit(s)
    need = int(lib.mural_simulate_txindel_workspace_bytes(int(feat_d[0].shape[0])))
    assert need >= 24 * int(feat_d[0].shape[0])      # (the arena aligns each array)
    ws = torch.empty(need // 8 + 1, dtype=torch.int64, device=dev)
    got = lib.mural_simulate_txindel_rows(C.byref(s), ws.data_ptr(), need - 8 if short_ws else ws.numel() * 8, L.current_stream_ptr(dev))
    assert got == rc
    torch.cuda.synchronize()
    if guard:
        return table, int(status.item()), whole
    return table, int(status.item())


def _host(table, n_tx, n_rep):
    return table.cpu().numpy().view(np.uint32)[:n_tx * 10 * n_rep].reshape(n_tx, 10, n_rep)


def _twin(prob, start, strand, k, segments, features, n_tx, kind, n_rep, off=1, spec=None, chrom_length=None, **kw):
    from mural_amd.summaries import simulate_txindel_host
    return simulate_txindel_host(prob, start, strand, k, segments, features, n_tx, kind, X.KEY, X.SEED, n_rep, off, spec, chrom_length, **kw)


@pytest.fixture(scope="module")
def record():
    text = X.toy_text() + X.random_text(seed=1, n_tx=24)
    names, segments, features = X.read(text)
    length = int(np.asarray(features["feat_b1"]).max()) + 25
    return dict(text=text, names=names, segments=segments, features=features, n_tx=len(names), length=length)


@pytest.fixture(scope="module")
def record_twin(record):
    """The twin's table of the record's float32 rows of 8 classes, deletion starts, at 1025 replicates, computed once: the cases at fewer
    replicates read its columns (replicate r does not depend on the replicate count)."""
    prob, start, strand, _ = X.rows(record["length"], 8, seed=1, dtype=np.float32, extra=60)
    table, status = _twin(prob, start, strand, 8, record["segments"], record["features"], record["n_tx"], 1, 1025)
    assert status == 0
    table.setflags(write=False)
    return prob, start, strand, table


def _args(record, k, kind):
    return (k, record["segments"], record["features"], record["n_tx"], kind)


# ---- 1. the kernel against the twin ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n_rep", [1, 63, 64, 65, 100, 1025])
def test_replicate_counts_around_a_block_and_past_one_unit(record, record_twin, n_rep):
    """1025 replicates are 17 blocks of 64: a unit holds 16, so a chunk becomes two units, the second with one partial block."""
    prob, start, strand, want = record_twin
    table, status, whole = _kernel(prob, start, strand, *_args(record, 8, 1), n_rep, pad=n_rep % 3, guard=256)
    assert status == 0 and _host(table, record["n_tx"], n_rep).tobytes() == np.ascontiguousarray(want[:, :, :n_rep]).tobytes()
    assert (whole[:256] == POISON).all() and (whole[-256:] == POISON).all()      # the guard words around the table
    assert want[:, :, :n_rep].any() and (n_rep < 1025 or want[:, :, 1024].any())


@pytest.mark.parametrize("kind,off,k,dtype,with_strand", [(0, 1, 8, np.float32, True), (0, 0, 5, np.float64, False), (1, 1, 5, np.float64, True),
                                                          (1, 0, 2, np.float32, False), (2, 1, 2, np.float64, True), (2, 0, 8, np.float32, False),
                                                          (0, 1, 2, np.float64, False), (2, 1, 5, np.float32, True)])
def test_kinds_offsets_classes_types_and_strand(record, kind, off, k, dtype, with_strand):
    prob, start, strand, _ = X.rows(record["length"], k, seed=10 + kind + 3 * off + k, dtype=dtype)
    strand = strand if with_strand else None
    kw = dict(off=off, spec=X.LENGTHS[k], chrom_length=record["length"] - 40)
    table, status = _kernel(prob, start, strand, *_args(record, k, kind), 66, pad=k % 2, **kw)
    want, want_status = _twin(prob, start, strand, *_args(record, k, kind), 66, **kw)
    assert status == want_status == 0 and _host(table, record["n_tx"], 66).tobytes() == want.tobytes() and want.any()
    if k == 8:
        assert int((want.sum(axis=(0, 2)) > 0).sum()) >= 8
    if with_strand:      # the strand bit is part of the counter
        assert want.tobytes() != _twin(prob, start, None, *_args(record, k, kind), 66, **kw)[0].tobytes()


def test_totals_equal_the_counted_rows_nonzero_draws(record):
    """Bins 0 .. 9 of one run, summed over the bins, are the non-zero draws of the rows each transcript counts: formed on the host from
    ``simulate_rows_host`` over the rows whose home base lies in the transcript's span (a deletion start counts whenever it does)."""
    from mural_amd import tables
    from mural_amd.summaries import simulate_rows_host
    prob, start, strand, _ = X.rows(record["length"], 8, seed=4, dtype=np.float32)
    table, status = _kernel(prob, start, strand, *_args(record, 8, 1), 70)
    got = _host(table, record["n_tx"], 70).astype(np.int64).sum(axis=1)
    drawn = simulate_rows_host(prob, start, strand, 8, X.KEY, X.SEED, np.arange(70)) > 0
    spans = [(s, e) for chrom, _, s, e, *_ in X._fields(record["text"])]
    want = np.stack([drawn[(start + 1 >= s) & (start + 1 < e)].sum(axis=0) for s, e in spans])
    assert status == 0 and np.array_equal(got, want) and want.any() and tables.INDEL_STRUCTURE_BINS[7] == "frameshift"


# ---- 2. the loop bounds ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind,n_rep", [(0, 5), (1, 1025), (2, 5)])
def test_past_the_chunk_length_the_grid_and_the_scan_threads(kind, n_rep):
    """Transcripts of two-base exons and three-base introns: more items than the scan workgroup has threads, and more units than the draw
    grid has waves -- at 1025 replicates every one-row chunk is two units --; one two-exon transcript whose intron holds 1100 rows, more
    than a chunk.  The bounds are read from the getters."""
    lib = _lib().lib()
    chunk, waves, scan = int(lib.mural_simulate_chunk_rows()), int(lib.mural_simulate_grid_waves()), int(lib.mural_simulate_scan_threads())
    n_rg = -(-(-(-n_rep // 64)) // 16)
    n_exons = max(-(-waves // n_rg), 2 * scan) // 2 + 37      # (an exon and its intron: two items)
    per_tx = 90
    rng = np.random.default_rng(11)
    lines, pos = [], 300
    for t in range(-(-n_exons // per_tx)):
        blocks = [(pos + 5 * j, pos + 5 * j + 2) for j in range(per_tx)]
        lines.append(D.bed12("chr1", f"t{t}", "+-"[t & 1], blocks, None if t % 3 else (blocks[2][0], blocks[-3][1])))
        pos = blocks[-1][1] + 3
    lines.append(D.bed12("chr1", "long", "-", [(1, 3), (295, 297)]))
    names, segments, features = X.read("\n".join(lines) + "\n")
    extra = chunk + 76 - 292      # the intron [3, 295) holds chunk + 76 rows
    start = np.sort(np.concatenate([np.arange(pos + 10), rng.integers(10, 280, size=extra)])).astype(np.int64)
    n = len(start)
    prob = rng.dirichlet(np.ones(8), size=n).astype(np.float32)
    strand = (np.arange(n) & 1).astype(np.uint8)
    n_items = len(features["feat_b0"])
    assert n_items > scan and n_items * n_rg > waves and chunk == 1024
    table, status = _kernel(prob, start, strand, 8, segments, features, len(names), kind, n_rep)
    want, _ = _twin(prob, start, strand, 8, segments, features, len(names), kind, n_rep)
    assert status == 0 and _host(table, len(names), n_rep).tobytes() == want.tobytes() and int(want[-1, :, 0].sum()) > 100


@pytest.mark.parametrize("n", [1, 63, 64, 65, 1023, 1024, 1025])
def test_row_counts_around_a_tile_and_a_chunk_inside_one_item(n):
    rng = np.random.default_rng(n)
    names, segments, features = X.read(D.bed12("chr1", "t", "+", [(10, 130), (140, 391)]) + "\n")
    start = np.sort(rng.integers(11, 127, size=n)).astype(np.int64)
    prob = rng.dirichlet(np.ones(8), size=n).astype(np.float32)
    table, status = _kernel(prob, start, None, 8, segments, features, 1, 1, 66)
    want, _ = _twin(prob, start, None, 8, segments, features, 1, 1, 66)
    assert status == 0 and _host(table, 1, 66).tobytes() == want.tobytes() and want.any()


# ---- 3. walks ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", [1, 2])
def test_long_deletions_walk_over_short_exons_to_the_spans_end_and_the_chromosomes(kind):
    """Exons of three bases and introns of four: a deletion of the 7-20 class (located by 7 bases) crosses two or three items, one of 64
    bases some twenty; the last transcript runs past the chromosome's end."""
    blocks = [(20 + 7 * j, 23 + 7 * j) for j in range(30)]
    text = (D.bed12("chr1", "p", "+", blocks, (27, 200)) + "\n" + D.bed12("chr1", "m", "-", blocks, (30, 226)) + "\n" +
            D.bed12("chr1", "nc", "+", [(b0 + 300, b1 + 300) for b0, b1 in blocks], (320, 320)) + "\n")
    names, segments, features = X.read(text)
    rng = np.random.default_rng(kind)
    start = np.repeat(np.arange(0, 540, dtype=np.int64), 2)
    prob = rng.dirichlet(np.ones(8), size=len(start)).astype(np.float32)
    prob[:, 0] = 0
    for spec, chrom_length in ((None, 520), ("1,2,3,7,20,33,64", None), ("1,2,3,7,20,33,64", 505)):
        kw = dict(spec=spec, chrom_length=chrom_length)
        table, status = _kernel(prob, start, None, 8, segments, features, 3, kind, 9, **kw)
        want, _ = _twin(prob, start, None, 8, segments, features, 3, kind, 9, **kw)
        assert status == 0 and _host(table, 3, 9).tobytes() == want.tobytes()
        assert want[0, 3].any() and want[0, 6].any() and want[1, 6].any() and want[2, 4].any() and want[2, 2].any()


@pytest.mark.parametrize("kind", [0, 1, 2])
def test_broken_links_and_skipped_items(record, kind):
    """Links out of range or into another transcript end a walk; a CDS item without its segment, an item of an unknown kind and an empty
    item are skipped as home items and end a walk that reaches them."""
    from mural_amd import tables
    prob, start, strand, _ = X.rows(record["length"], 8, seed=6, dtype=np.float32)
    feats = record["features"]
    prev, nxt = tables.structure_links(feats)
    bad_next, bad_prev = nxt.copy(), prev.copy()
    other = int(np.nonzero(feats["feat_tx"] != feats["feat_tx"][21])[0][0])
    bad_next[5], bad_next[20], bad_next[21], bad_prev[30], bad_prev[31] = len(nxt) + 3, -7, other, 1 << 30, other
    args = _args(record, 8, kind)
    table, status = _kernel(prob, start, strand, *args, 6, links=(bad_prev, bad_next))
    want, _ = _twin(prob, start, strand, *args, 6, links=(bad_prev, bad_next))
    assert status == 0 and _host(table, record["n_tx"], 6).tobytes() == want.tobytes()
    assert want.tobytes() != _twin(prob, start, strand, *args, 6)[0].tobytes() or kind == 0
    cds = np.nonzero(np.asarray(feats["feat_kind"]) == 5)[0]
    edits = (("feat_seg", int(cds[0]), len(record["segments"]["seg_b0"])), ("feat_seg", int(cds[1]), -1), ("feat_kind", 7, 9),
             ("feat_b1", 9, int(feats["feat_b0"][9])))
    changed = dict(feats)
    for key, at, value in edits:
        arr = np.asarray(changed[key]).copy()
        arr[at] = value
        changed[key] = arr
    args = (8, record["segments"], changed, record["n_tx"], kind)
    table, status = _kernel(prob, start, strand, *args, 6, links=(prev, nxt))
    want2, _ = _twin(prob, start, strand, *args, 6, links=(prev, nxt))
    assert status == 0 and _host(table, record["n_tx"], 6).tobytes() == want2.tobytes() != _twin(prob, start, strand, *_args(record, 8, kind), 6)[0].tobytes()


# ---- 4. calls ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", [0, 1, 2])
def test_parts_and_permuted_equal_starts_give_equal_bytes(record, kind):
    prob, start, strand, _ = X.rows(record["length"], 8, seed=8, dtype=np.float32, extra=700)
    strand[:] = 0      # (rows of one start and strand draw one value whatever their order; mixed strands at one start are distinct rows)
    want, _ = _twin(prob, start, strand, *_args(record, 8, kind), 65)
    rng = np.random.default_rng(kind)
    perm = np.lexsort((rng.random(len(start)), start))
    assert not np.array_equal(perm, np.arange(len(start)))
    cuts = np.sort(rng.choice(np.arange(1, len(start)), size=5, replace=False))
    table = None
    for rows in np.split(perm, cuts):
        table, status = _kernel(prob[rows], start[rows], strand[rows], *_args(record, 8, kind), 65, into=table)
        assert status == 0
    assert _host(table, record["n_tx"], 65).tobytes() == want.tobytes()


def test_status_bits_and_calls_that_launch_nothing(record):
    prob, start, strand, _ = X.rows(record["length"], 8, seed=3, dtype=np.float32)
    n_tx = record["n_tx"]
    args = _args(record, 8, 1)
    table, status = _kernel(prob[:0], start[:0], strand[:0], *args, 4, fill=POISON)
    assert status == 0 and (table == POISON).all()
    none = {key: v[:0] if key.startswith("feat_") else v for key, v in record["features"].items()}
    bad = prob.copy()
    at = int(np.nonzero(start >= 50)[0][0])
    bad[at, 2], bad[at + 1, 0], bad[at + 2, 1] = np.nan, np.nan, 1.5       # class 0 is never read; 1.5 is clamped
    empty_links = (np.zeros(0, np.int32), np.zeros(0, np.int32))
    table, status = _kernel(bad, start, strand, 8, record["segments"], none, n_tx, 1, 4, fill=POISON, links=empty_links)      # only the rows are checked
    assert status == 8 and (table == POISON).all()
    first = start.copy()
    first[0] = -4
    table, status = _kernel(bad, first, strand, *args, 4)
    want, want_status = _twin(bad, first, strand, *args, 4)
    assert status == want_status == 9 and _host(table, n_tx, 4).tobytes() == want.tobytes()
    swapped = start.copy()
    swapped[100], swapped[101] = start[101] + 1, start[100]
    assert swapped[100] > swapped[101]
    table, status, whole = _kernel(prob, swapped, strand, *args, 4, guard=128)
    assert status == 4 and (whole[:128] == POISON).all() and (whole[-128:] == POISON).all()


# ---- 5. refusals ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("what", ["n_class_1", "n_class_9", "n_class_16", "n_rep_0", "n_rep_above", "n", "n_features", "n_segments", "kind_3",
                                  "kind_neg", "offset_2", "offset_neg", "len_lo_0", "len_hi_below", "len_hi_65", "workspace"])
def test_refusals_leave_the_table_untouched(record, what):
    prob, start, strand, _ = X.rows(record["length"], 8, seed=3, dtype=np.float32)

    def edit(s):
        if what.startswith("n_class"):
            s.n_class = int(what.rsplit("_", 1)[1])
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
        elif what.startswith("kind"):
            s.kind = 3 if what == "kind_3" else -1
        elif what.startswith("offset"):
            s.breakpoint_offset = 2 if what == "offset_2" else -1
        elif what == "len_lo_0":
            s.class_len[3][0] = 0
        elif what == "len_hi_below":
            s.class_len[7][0], s.class_len[7][1] = 5, 4
        elif what == "len_hi_65":
            s.class_len[1][1] = 65

    invalid, workspace = 1, 3      # MURAL_E_INVALID, MURAL_E_WORKSPACE
    table, status = _kernel(prob, start, strand, *_args(record, 8, 1), 4, fill=POISON, edit=edit, rc=workspace if what == "workspace" else invalid,
                            short_ws=what == "workspace")
    assert status == 0 and (table == POISON).all()


def test_the_message_of_nine_classes_names_the_bound(record):
    L = _lib()
    prob, start, strand, _ = X.rows(record["length"], 8, seed=3, dtype=np.float32)

    def edit(s):
        s.n_class = 9

    _kernel(prob, start, strand, *_args(record, 8, 1), 4, edit=edit, rc=1)
    with pytest.raises(ValueError, match="n_class <= 8"):
        L.check(1)


# ---- 6. in flight ---------------------------------------------------------------------------------------------------------------------------
def test_sink_behind_an_indel_regions_run_equals_the_twin(files, tmp_path, monkeypatch):  # noqa: F811
    """A small UNet_Small over regions through SummarySink(simulate_indel_structure=True), in one part and in several: the table equals
    the twin over the rows of the same run, the LoF counts are ``simulate_indel_lof_counts`` of it, and the file has a line per
    transcript and bin."""
    from mural_amd import predict as P
    from mural_amd import tables
    from mural_amd.summaries import simulate_chrom_key, simulate_indel_lof_counts, simulate_txindel_host
    from tests import _util as U
    from tests.test_gpu_indel import product_from
    d, fa = files
    fx = U.load("indel_synth_small.npz")
    model = product_from(fx)
    model.load_state_dict(U.indel_state_for(fx, U.indel_oracle_from_hp(fx["hp"], fx["down"])))
    model = model.cuda().eval()
    fwd = P.HipShardForward(model, fa, local_radius=R_LOCAL, local_order=3, distal_radius=int(fx["hp"][0]), model_type="indel", poisson=False)
    rng = np.random.default_rng(5)
    lines = []
    for t in range(6):
        cuts = np.sort(rng.choice(np.arange(70, 410), size=2 * int(rng.integers(1, 6)), replace=False))
        blocks = [(int(a), int(b)) for a, b in zip(cuts[::2], cuts[1::2])]
        lines.append(D.bed12("chrA", f"tx{t}", "+-"[t & 1], blocks, None if t % 3 else (blocks[0][0], blocks[0][0])))
    tx = tables.read_transcript_structure(io.StringIO("\n".join(lines) + "\n"))
    counts = []
    for tag, part_rows in (("a", 1 << 20), ("b", 100)):
        monkeypatch.setattr(P, "_ALIGNED_PART_ROWS", part_rows)
        keep = _Keep()
        sink = P.SummarySink(str(tmp_path / tag), indel_transcripts=tx, indel_kind="deletion_start", genome=fwd.genome, transcript_labels=False,
                             simulate=70, simulate_seed=21, simulate_indel_structure=True)
        n = P.predict_regions_sharded(fwd, "chrA:61-420", "ANY", model_type="indel", sink=P.TeeSink(keep, sink), collect=False)
        counts.append(sink.indel_structure_simulation_counts())
    k = sink._n_class
    prob, start, label, strand = (np.concatenate([p[i] for p in keep.rows["chrA"]]) for i in range(4))
    want, status = simulate_txindel_host(prob, start, strand, k, tx[2].get("chrA"), tx[3]["chrA"], len(tx[0]), 1, simulate_chrom_key("chrA"),
                                         21, 70, chrom_length=len(MAIN))
    assert n == len(start) > 200 and k == 8 and status == 0
    assert counts[0].tobytes() == counts[1].tobytes() == want.tobytes()
    res = sink.result()["indel_structure_simulation"]
    lof, upper = simulate_indel_lof_counts(want)
    assert res[0] == tx[0] and np.array_equal(res[2], lof) and np.array_equal(res[3], upper) and res[4] is None and len(res[5]) == len(tx[0])
    text, other = ((tmp_path / f"{tag}.indel_structure.sim.tsv").read_text().splitlines() for tag in "ab")
    # (the simulated columns are the counts'; the expected column follows the forward's own rounding, which may move with the part size)
    assert [ln.split("\t")[:3] + ln.split("\t")[4:] for ln in text] == [ln.split("\t")[:3] + ln.split("\t")[4:] for ln in other]
    assert len(text) == 1 + 12 * len(tx[0]) and text[11].split("\t")[1:3] == ["lof", "NA"] and text[12].split("\t")[1] == "lof_upper"
