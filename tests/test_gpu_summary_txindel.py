"""INDEL structure tables on the device (csrc/summary_txindel.hip: mural_summary_txindel_rows; SummarySink(indel_transcripts=...);
tables.indel_structure_table): every case goes through the entry point and is compared for EQUALITY, word for word, with the numpy twin
``summary_txindel_host`` -- the record of the host suite in both probability types, the three label kinds, the three event kinds and
both offsets, the three loop bounds of the entry read from its getters, parts and permuted equal starts, the status bits, calls that
launch nothing, the refusals, and in flight a small UNet_Small over regions."""
import ctypes as C
import io

import numpy as np
import pytest
import torch

from tests import _conseq_data as D
from tests import _txindel_data as I
from tests.test_gpu_regions import MAIN, R_LOCAL, RECORDS, files  # noqa: F401  (fixture)
from tests.test_gpu_summary_conseq import _Keep, _dev, _lib, _up

pytestmark = pytest.mark.gpu

LABEL_DTYPES = {0: np.float32, 1: np.int32, 2: np.int64}


def _acc(n_tx, fill=0):
    dev = _dev()
    return dict(table=torch.full((max(n_tx, 1) * 30,), fill, dtype=torch.int64, device=dev),
                rows=torch.full((max(n_tx, 1) * 2,), fill, dtype=torch.int64, device=dev),
                status=torch.zeros(1, dtype=torch.int32, device=dev), features={}, segments={}, ws=None)


def _kernel(prob, start, label, k, segments, features, n_tx, kind, off=1, spec=None, chrom_length=None, links=None, into=None, pad=0):
    """One mural_summary_txindel_rows call on device copies of the arrays: (accumulators, status)."""
    from mural_amd import tables
    from mural_amd.summaries import txindel_rows_device
    dev = _dev()
    if pad:
        prob = np.concatenate([prob, np.full((len(prob), pad), 0.25, prob.dtype)], axis=1)
    prob_d, start_d, label_d = _up(prob), _up(start), _up(label)
    acc = into or _acc(n_tx)
    n = int(start_d.shape[0])
    txindel_rows_device(acc, "chr", segments, features, tables.structure_links(features) if links is None else links, n_tx, kind, off,
                        tables.check_indel_lengths(spec, k), chrom_length, dev, prob=prob_d.data_ptr(), prob_f64=prob_d.dtype == torch.float64,
                        prob_stride=prob_d.stride(0) if n else k, start=start_d.data_ptr(), label=label_d.data_ptr(),
                        label_kind={torch.float32: 0, torch.int32: 1, torch.int64: 2}[label_d.dtype], n=n, n_class=k)
    return acc, int(acc["status"].item())


def _host(acc, n_tx):
    return (acc["table"].cpu().numpy().view(np.uint64)[:n_tx * 30].reshape(n_tx, 10, 3), acc["rows"].cpu().numpy().view(np.uint64)[:n_tx * 2].reshape(n_tx, 2))


def _twin(prob, start, label, k, segments, features, n_tx, kind, off=1, spec=None, chrom_length=None, **kw):
    from mural_amd.summaries import summary_txindel_host
    return summary_txindel_host(prob, start, label, k, segments, features, n_tx, kind, off, spec, chrom_length, **kw)


def _same(acc, want, n_tx):
    got = _host(acc, n_tx)
    return got[0].tobytes() == want[0].tobytes() and got[1].tobytes() == want[1].tobytes()


@pytest.fixture(scope="module")
def record():
    from mural_amd import tables
    seq, text, names = I.build()
    tx = tables.read_transcript_structure(io.StringIO(text))
    return dict(seq=seq, text=text, names=names, tx=tx, segments=tx[2]["chr1"], features=tx[3]["chr1"], n_tx=len(names))


def _both(record, prob, start, label, k, kind, off=1, spec=None, chrom_length=None, pad=0):
    args = (k, record["segments"], record["features"], record["n_tx"], kind, off, spec, chrom_length)
    acc, status = _kernel(prob, start, label, *args, pad=pad)
    return acc, status, _twin(prob, start, label, *args)


# ---- 1. the kernel against the twin ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind,off,k,dtype,label_kind,pad", [(0, 1, 8, np.float32, 0, 3), (1, 1, 16, np.float64, 1, 0), (2, 0, 5, np.float32, 2, 1),
                                                             (0, 0, 16, np.float64, 2, 0), (1, 0, 2, np.float32, 1, 2), (2, 1, 8, np.float64, 0, 0)])
def test_kernel_equals_the_twin_on_the_record(record, kind, off, k, dtype, label_kind, pad):
    prob, start, label = I.rows(record["seq"], k, seed=kind + 3 * off, dtype=dtype)
    label = label.astype(LABEL_DTYPES[label_kind])
    acc, status, want = _both(record, prob, start, label, k, kind, off, I.LENGTHS[k], len(record["seq"]), pad=pad)
    assert status == 0 and want[2] == 0 and _same(acc, want, record["n_tx"])
    assert len(record["features"]["feat_b0"]) > 600 and record["n_tx"] > 60 and len(start) > 3000 and int(want[1][:, 0].sum()) > 3000
    if k == 16:
        assert (want[0][:, :, 0].sum(axis=0) > 0).all()                                  # every bin is reached
    if (kind, off) == (1, 1):      # against the oracle as well, and without the chromosome's length
        got = _host(acc, record["n_tx"])
        assert I.as_integers(*got) == I.oracle(record["text"], prob, start, label, k, kind, off, I.pairs(I.LENGTHS[k], k), len(record["seq"]))
        acc, status, free = _both(record, prob, start, label, k, kind, off, I.LENGTHS[k])
        assert status == 0 and _same(acc, free, record["n_tx"]) and free[0].tobytes() != want[0].tobytes()


@pytest.mark.parametrize("kind", [0, 1, 2])
def test_parts_and_permuted_equal_starts_are_bit_identical(record, kind):
    prob, start, label = I.rows(record["seq"], 8, seed=8, dtype=np.float32, extra=900)
    want = _twin(prob, start, label, 8, record["segments"], record["features"], record["n_tx"], kind)
    rng = np.random.default_rng(kind)
    perm = np.lexsort((rng.random(len(start)), start))      # ascending, the rows of equal starts in another order
    assert not np.array_equal(perm, np.arange(len(start)))
    cuts = np.sort(rng.choice(np.arange(1, len(start)), size=6, replace=False))
    acc = None
    for rows in np.split(perm, cuts):
        acc, status = _kernel(prob[rows], start[rows], label[rows], 8, record["segments"], record["features"], record["n_tx"], kind, into=acc)
        assert status == 0
    assert _same(acc, want, record["n_tx"])


# ---- 2. the loop bounds ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", [0, 1, 2])
def test_past_the_chunk_length_the_grid_and_the_scan_threads(kind):
    """Transcripts of two-base exons and three-base introns, enough of them for more chunks than the reduce grid has waves and more items
    than the scan workgroup has threads; one two-exon transcript whose intron's rows are repeated until the item holds more than two chunks
    and a partial one.  The bounds are read from the getters.  A deletion of 7 bases crosses three items here."""
    from mural_amd import tables
    lib = _lib().lib()
    chunk, waves, scan = int(lib.mural_summary_txindel_chunk_rows()), int(lib.mural_summary_txindel_grid_waves()), int(lib.mural_summary_txindel_scan_threads())
    n_exons = max(waves, 2 * scan) + 37
    per_tx = 90
    rng = np.random.default_rng(11)
    lines, pos = [], 300
    for t in range(-(-n_exons // per_tx)):
        blocks = [(pos + 5 * j, pos + 5 * j + 2) for j in range(per_tx)]
        lines.append(D.bed12("chr1", f"t{t}", "+-"[t & 1], blocks, None if t % 3 else (blocks[2][0], blocks[-3][1])))
        pos = blocks[-1][1] + 3
    lines.append(D.bed12("chr1", "long", "-", [(1, 3), (295, 297)]))
    names, meta, segments, features = tables.read_transcript_structure(io.StringIO("\n".join(lines) + "\n"))
    segments, features = segments["chr1"], features["chr1"]
    repeat = -(-(2 * chunk + 77) // 292)
    start = np.sort(np.concatenate([np.arange(pos + 10), np.repeat(np.arange(3, 295), repeat - 1)])).astype(np.int64)
    n = len(start)
    prob = rng.dirichlet(np.ones(8), size=n).astype(np.float32)
    label = rng.integers(0, 8, size=n).astype(np.int32)
    two_base = int((features["feat_b1"] - features["feat_b0"] == 2).sum())
    assert two_base > waves and two_base > scan and 292 * repeat > 2 * chunk
    acc, status = _kernel(prob, start, label, 8, segments, features, len(names), kind)
    want = _twin(prob, start, label, 8, segments, features, len(names), kind)
    assert status == 0 and _same(acc, want, len(names))
    assert int(want[1][-1, 0]) > 2 * chunk and int(want[1][:-1, 0].sum()) > (5 * per_tx - 4) * (len(names) - 2)


@pytest.mark.parametrize("off", [0, 1])
@pytest.mark.parametrize("kind", [0, 1, 2])
def test_a_row_on_the_boundary_of_two_adjacent_items_goes_to_the_second(kind, off):
    """The plan's ranges under the home-base shift (row_chunks.h): two transcripts whose items abut, a row at every start and equal
    starts on the boundaries, so that for every pair of adjacent items [.., B) and [B, ..) there are rows with start + shift == B -- b1
    of the first, b0 of the second -- whatever the shift of (kind, offset)."""
    from mural_amd import tables
    lines = [D.bed12("chr1", "coding", "+", [(20, 60), (80, 130), (150, 170)], (30, 160)), D.bed12("chr1", "plain", "-", [(40, 90), (110, 180)])]
    names, meta, segments, features = tables.read_transcript_structure(io.StringIO("\n".join(lines) + "\n"))
    segments, features = segments["chr1"], features["chr1"]
    shift = off - (0 if kind == 1 else 1)
    b0, b1, tx = (np.asarray(features[key]) for key in ("feat_b0", "feat_b1", "feat_tx"))
    shared = sorted({int(b) for b, t in zip(b1, tx) if ((b0 == b) & (tx == t)).any()})      # b1 of an item = b0 of the same transcript's next
    assert len(shared) >= 6 and 30 in shared and 60 in shared and 90 in shared
    start = np.sort(np.concatenate([np.arange(5, 195), np.repeat(np.asarray(shared) - shift, 2)])).astype(np.int64)
    assert len(start) <= 220 and all((start + shift == b).sum() == 3 for b in shared)
    rng = np.random.default_rng(10 * kind + off)
    prob = rng.dirichlet(np.ones(8), size=len(start)).astype(np.float32)
    label = rng.integers(0, 8, size=len(start)).astype(np.int32)
    acc, status = _kernel(prob, start, label, 8, segments, features, len(names), kind, off)
    want = _twin(prob, start, label, 8, segments, features, len(names), kind, off)
    assert status == 0 == want[2] and _same(acc, want, len(names))
    assert int(want[1][0, 0]) > 150 and int(want[1][1, 0]) > 120      # both transcripts count the rows of their spans


# ---- 3. status, and calls that launch nothing -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("what,bit", [("start", 1), ("label", 2), ("nan", 8), ("above", 8)])
def test_bad_rows_are_skipped_and_set_status(record, what, bit):
    prob, start, label = I.rows(record["seq"], 8, seed=3, dtype=np.float32)
    at = 1030
    if what == "start":
        start[0] = -4                                          # (the rows still ascend)
    elif what == "label":
        label[at] = 8
    else:
        prob[at, 7] = dict(nan=np.nan, above=1.5)[what]
    prob[at + 1, 0] = np.nan                                   # class 0's probability is never read
    acc, status, want = _both(record, prob, start, label, 8, 1)
    assert status == bit == want[2] and _same(acc, want, record["n_tx"])


def test_a_descending_pair_sets_status_4_and_touches_nothing_out_of_bounds(record):
    """The tables sit between guard words: a descending pair leaves the guards as they are."""
    prob, start, label = I.rows(record["seq"], 8, seed=3, dtype=np.float32, extra=0)
    start[100], start[101] = start[101], start[100]
    n_tx, dev = record["n_tx"], _dev()
    big = torch.full((n_tx * 32 + 128,), 7, dtype=torch.int64, device=dev)
    acc = _acc(n_tx)
    acc["table"], acc["rows"] = big[64:64 + n_tx * 30], big[64 + n_tx * 30:64 + n_tx * 32]
    acc["table"].zero_()
    acc["rows"].zero_()
    for kind in (0, 1, 2):
        _, status = _kernel(prob, start, label, 8, record["segments"], record["features"], n_tx, kind, into=acc)
        assert status == 4
    assert (big[:64] == 7).all() and (big[64 + n_tx * 32:] == 7).all()


def test_broken_links_end_the_walk(record):
    from mural_amd import tables
    prob, start, label = I.rows(record["seq"], 8, seed=2, dtype=np.float32)
    prev, nxt = tables.structure_links(record["features"])
    bad_next, bad_prev = nxt.copy(), prev.copy()
    other = int(np.nonzero(record["features"]["feat_tx"] != record["features"]["feat_tx"][41])[0][0])
    bad_next[5], bad_next[40], bad_next[41], bad_prev[50], bad_prev[51] = len(nxt) + 3, -7, other, 1 << 30, other
    for kind in (0, 1, 2):
        args = (8, record["segments"], record["features"], record["n_tx"], kind)
        acc, status = _kernel(prob, start, label, *args, links=(bad_prev, bad_next))
        assert status == 0 and _same(acc, _twin(prob, start, label, *args, links=(bad_prev, bad_next)), record["n_tx"])


def test_calls_that_launch_nothing_leave_the_tables_untouched(record):
    n_tx = record["n_tx"]
    prob, start, label = I.rows(record["seq"], 8, seed=2, dtype=np.float32)
    acc, status = _kernel(prob[:0], start[:0], label[:0], 8, record["segments"], record["features"], n_tx, 0, into=_acc(n_tx, 7))
    assert status == 0 and (acc["table"] == 7).all() and (acc["rows"] == 7).all()
    none = {key: v[:0] if key.startswith("feat_") else v for key, v in record["features"].items()}
    acc, status = _kernel(prob, start, label, 8, record["segments"], none, n_tx, 0, into=_acc(n_tx, 7))
    assert status == 0 and (acc["table"] == 7).all() and (acc["rows"] == 7).all()
    from mural_amd.predict import SummarySink
    sink = SummarySink(None, indel_transcripts=record["tx"], indel_kind="insertion")      # a chromosome the file does not name
    sink({"chrom": "chrZ", "start": _up(start), "end": _up(start + 1), "strand": _up(np.zeros(len(start), np.uint8)),
          "label": _up(label.astype(np.float32)), "prob": _up(prob), "n_class": 8, "calibrated": False, "aligned": True})
    assert not sink._reducers["indel_structure"].dev
    sink.close()
    assert not sink.indel_structure_sums()[0].any() and not sink.indel_structure_sums()[1].any()


def test_refusals_and_the_short_workspace(record):
    from mural_amd import tables
    L = _lib()
    lib = L.lib()
    prob, start, label = I.rows(record["seq"], 8, seed=2, dtype=np.float32)
    n_tx = record["n_tx"]
    links = tables.structure_links(record["features"])

    def call(ws_short=False, lengths=None, **fields):
        """The return code of one call with `fields` overridden; the arrays are the record's."""
        dev = _dev()
        acc = _acc(n_tx)
        keep = [_up(prob), _up(start), _up(label)] + [_up(record["features"][k]) for k in ("feat_b0", "feat_b1", "feat_tx", "feat_kind", "feat_seg")]
        keep += [_up(links[0]), _up(links[1])]
        keep += [_up(record["segments"][k]) for k in ("seg_b0", "seg_b1", "seg_cds0", "seg_tx", "tx_strand", "tx_cds_len")]
        s = L.MuralSummaryTxindelRows()
        s.prob, s.prob_f64, s.prob_stride, s.start, s.label, s.label_kind = keep[0].data_ptr(), 0, 8, keep[1].data_ptr(), keep[2].data_ptr(), 2
        s.n, s.n_class, s.n_transcripts, s.kind, s.breakpoint_offset, s.chrom_length = len(start), 8, n_tx, 1, 1, -1
        for c, (lo, hi) in enumerate(tables.check_indel_lengths(lengths, 8).tolist()):
            s.class_len[c][0], s.class_len[c][1] = lo, hi
        s.feat_b0, s.feat_b1, s.feat_tx, s.feat_kind, s.feat_seg, s.feat_prev, s.feat_next = (x.data_ptr() for x in keep[3:10])
        s.n_features = len(record["features"]["feat_b0"])
        s.seg_b0, s.seg_b1, s.seg_cds0, s.seg_tx, s.tx_strand, s.tx_cds_len = (x.data_ptr() for x in keep[10:16])
        s.n_segments = len(record["segments"]["seg_b0"])
        s.table, s.rows, s.status = acc["table"].data_ptr(), acc["rows"].data_ptr(), acc["status"].data_ptr()
        for key, v in fields.items():
            if key == "class_len":
                s.class_len[v[0]][0], s.class_len[v[0]][1] = v[1], v[2]
            else:
                setattr(s, key, v)
        need = int(lib.mural_summary_txindel_workspace_bytes(s.n_features))
        ws = torch.empty(need // 8 + 1, dtype=torch.int64, device=dev)
        rc = lib.mural_summary_txindel_rows(C.byref(s), ws.data_ptr(), need - 8 if ws_short else need, L.current_stream_ptr(dev))
        torch.cuda.synchronize()
        return rc, acc

    rc, acc = call()
    want = _twin(prob, start, label, 8, record["segments"], record["features"], n_tx, 1)
    assert rc == 0 and _same(acc, want, n_tx)
    invalid = 1
    for fields in (dict(n_class=1), dict(n_class=17), dict(kind=3), dict(kind=-1), dict(breakpoint_offset=2), dict(n=(1 << 31) + 1), dict(n=-1),
                   dict(n_features=(1 << 22) + 1), dict(label_kind=3), dict(prob_stride=7), dict(feat_kind=None), dict(feat_next=None),
                   dict(feat_prev=None), dict(seg_cds0=None), dict(table=None), dict(class_len=(3, 0, 2)), dict(class_len=(7, 5, 4)),
                   dict(class_len=(1, 1, 65))):
        rc, acc = call(**fields)
        assert rc == invalid and not acc["table"].any(), fields
    rc, acc = call(ws_short=True)
    assert rc != 0 and rc != invalid and not acc["table"].any()          # MURAL_E_WORKSPACE
    with pytest.raises(ValueError, match="class_len"):
        L.check(call(class_len=(2, 9, 3))[0])


# ---- 4. in flight ---------------------------------------------------------------------------------------------------------------------------
def _table_rows(path, k):
    """(prob float64 [n][k], start, label) of a written prediction table."""
    lines = open(path).read().splitlines()
    f = [ln.split("\t") for ln in lines[1:]]
    header = lines[0].split("\t")
    first = header.index("prob0")
    return (np.array([[float(v) for v in r[first:first + k]] for r in f]), np.array([int(r[1]) for r in f], np.int64),
            np.array([int(r[header.index("mut_type")]) for r in f], np.int64))


def test_sink_behind_an_indel_regions_run(files, tmp_path):
    """A small UNet_Small over regions: the sink's sums equal the twin over the rows of the same run; ``tables.indel_structure_table`` on
    the table that run wrote equals the twin over that file's rows word for word, counts the same rows as the sink, and its sums lie
    within the table's four printed digits of the sink's."""
    from mural_amd import predict as P
    from mural_amd import tables
    from tests import _util as U
    from tests.test_gpu_indel import product_from
    d, fa = files
    fx = U.load("indel_synth_small.npz")
    model = product_from(fx)
    model.load_state_dict(U.indel_state_for(fx, U.indel_oracle_from_hp(fx["hp"], fx["down"])))
    model = model.cuda().eval()
    fwd = P.HipShardForward(model, fa, local_radius=R_LOCAL, local_order=3, distal_radius=int(fx["hp"][0]), model_type="indel",
                            poisson=False)      # (the raw softmax: the synthetic weights saturate it, and the Poisson step has no value for p = 1)
    rng = np.random.default_rng(5)
    lines = []
    for t in range(6):
        cuts = np.sort(rng.choice(np.arange(70, 410), size=2 * int(rng.integers(1, 6)), replace=False))
        blocks = [(int(a), int(b)) for a, b in zip(cuts[::2], cuts[1::2])]
        lines.append(D.bed12("chrA", f"tx{t}", "+-"[t & 1], blocks, None if t % 3 else (blocks[0][0], blocks[0][0])))
    tx = tables.read_transcript_structure(io.StringIO("\n".join(lines) + "\n"))
    out = str(tmp_path / "t.tsv")
    keep = _Keep()
    sink = P.SummarySink(str(tmp_path / "s"), indel_transcripts=tx, indel_kind="deletion_start", genome=fwd.genome, transcript_labels=False)
    n = P.predict_regions_sharded(fwd, "chrA:61-420", "ANY", model_type="indel", sink=P.TeeSink(keep, P.TsvSink(out), sink), collect=False)
    k = sink._n_class      # (the rows' probability block is wider than the classes)
    assert k == 8
    prob, start, label, _ = (np.concatenate([p[i] for p in keep.rows["chrA"]]) for i in range(4))
    got = sink.indel_structure_sums()
    args = (k, tx[2].get("chrA"), tx[3]["chrA"], len(tx[0]), 1, 1, None)
    want = _twin(prob, start, label, *args, chrom_length=len(MAIN))
    assert n == len(start) > 200 and want[2] == 0 and int(want[1][:, 0].sum()) > 300
    assert got[0].tobytes() == want[0].tobytes() and got[1].tobytes() == want[1].tobytes()
    names, meta, table, rows = tables.indel_structure_table(out, tx, k, "deletion_start", chrom_lengths={"chrA": len(MAIN)}, chunk_bytes=16 << 10)
    file_prob, file_start, file_label = _table_rows(out, k)
    of_file = _twin(file_prob, file_start, file_label, *args, chrom_length=len(MAIN))
    assert names == tx[0] and table.tobytes() == of_file[0].tobytes() and rows.tobytes() == of_file[1].tobytes()
    assert np.array_equal(rows, got[1]) and np.array_equal(table[:, :, 0], got[0][:, :, 0])
    value = lambda t: np.array([[((int(h) << 40) + int(l)) / 2 ** 71 for _, h, l in cells] for cells in t.tolist()])      # noqa: E731
    assert (np.abs(value(table) - value(got[0])) <= 5e-4 * value(got[0]) + 1e-30).all()
    # the evaluate-style route takes the chromosomes' lengths from a FASTA index and writes the table's own sums
    fai = tmp_path / "g.fai"
    fai.write_text("".join(f"{name}\t{len(seq)}\t0\t60\t61\n" for name, seq in RECORDS.items()))

    class Args:
        pred_file, indel_transcripts, n_class, indel_kind, out_prefix, chrom_lengths = out, tx, k, "deletion_start", str(tmp_path / "calc"), str(fai)
    calc = open(tables.run_indel_structure_calc(Args)).read()
    assert calc == open(tables.write_indel_structure_outputs(names, meta, table, rows, 1, str(tmp_path / "direct"))).read()
    text = (tmp_path / "s.indel_structure.tsv").read_text().splitlines()
    assert [ln.split("\t")[0] for ln in text[1:]] == tx[0] and text[1].split("\t")[3] == "deletion_start" and text[1].split("\t")[7] == "NA"
