"""The INDEL structure table on the host: the numpy twin ``summary_txindel_host`` (the specification of mural_summary_txindel_rows)
against the brute-force oracle of tests/_txindel_data.py on the record of tests/_txstruct_data.py -- both strands, the three kinds, both
offsets, 2, 5, 8 and 16 classes, framed, mixed and always-shifting ranges --, the known answers, ``structure_links``, every refusal, the
writer, the command line's refusals and the compiler's report of the kernel."""
import importlib.util
import io
import os

import numpy as np
import pytest

from tests import _txindel_data as I

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def record():
    from mural_amd import tables
    seq, text, names = I.build()
    tx = tables.read_transcript_structure(io.StringIO(text))
    return dict(seq=seq, text=text, names=names, tx=tx, segments=tx[2]["chr1"], features=tx[3]["chr1"], n_tx=len(names))


def _twin(record, prob, start, label, k, kind, off, spec, chrom_length=None, **kw):
    from mural_amd.summaries import summary_txindel_host
    return summary_txindel_host(prob, start, label, k, record["segments"], record["features"], record["n_tx"], kind, off, spec,
                                chrom_length, **kw)


@pytest.mark.parametrize("kind,off,k", [(0, 1, 8), (0, 0, 5), (1, 1, 16), (1, 0, 2), (2, 1, 5), (2, 0, 16), (0, 1, 16), (1, 1, 8), (2, 1, 8)])
def test_twin_equals_the_oracle_on_the_record(record, kind, off, k):
    prob, start, label = I.rows(record["seq"], k, seed=kind + 3 * off)
    n = len(record["seq"])
    table, rows, status = _twin(record, prob, start, label, k, kind, off, I.LENGTHS[k], chrom_length=n)
    assert status == 0 and int(rows[:, 0].sum()) > 3000
    assert I.as_integers(table, rows) == I.oracle(record["text"], prob, start, label, k, kind, off, I.pairs(I.LENGTHS[k], k), n)
    if k == 16:
        assert (table[:, :, 0].sum(axis=0) > 0).all()                                 # every bin is reached
    # one transcript runs two bases past the record: a deletion start is clipped to the chromosome only where its length is given
    if kind == 1 and k == 16:
        free = _twin(record, prob, start, label, k, kind, off, I.LENGTHS[k])
        past = record["names"].index("past_the_end")
        others = np.arange(record["n_tx"]) != past
        assert free[0][past].tobytes() != table[past].tobytes() and free[0][others].tobytes() == table[others].tobytes()
        assert I.as_integers(free[0], free[1]) == I.oracle(record["text"], prob, start, label, k, kind, off, I.pairs(I.LENGTHS[k], k))


def test_the_tables_depend_on_the_set_of_rows_alone(record):
    prob, start, label = I.rows(record["seq"], 8, seed=5, dtype=np.float32)
    want = _twin(record, prob, start, label, 8, 1, 1, None)
    perm = np.random.default_rng(0).permutation(len(start))
    got = _twin(record, prob[perm], start[perm], label[perm], 8, 1, 1, None)
    assert got[0].tobytes() == want[0].tobytes() and got[1].tobytes() == want[1].tobytes()
    into = None
    for part in np.array_split(perm, 5):
        t, r, _ = _twin(record, prob[part], start[part], label[part], 8, 1, 1, None, into=into)
        into = (t, r)
    assert into[0].tobytes() == want[0].tobytes() and into[1].tobytes() == want[1].tobytes()


def _known(strand, kind, starts, spec, k, off=1):
    from mural_amd import tables
    from mural_amd.summaries import summary_txindel_host
    text = I.KNOWN % strand
    names, meta, segments, features = tables.read_transcript_structure(io.StringIO(text))
    start = np.asarray(starts, np.int64)
    prob = np.full((len(start), k), 2.0 ** -10)
    label = np.zeros(len(start), np.int64)
    table, rows, status = summary_txindel_host(prob, start, label, k, segments["chr1"], features["chr1"], 1, kind, off, spec)
    assert status == 0
    got = I.as_integers(table, rows)
    assert got == I.oracle(text, prob, start, label, k, kind, off, I.pairs(spec, k))
    unit = 1 << 61                                                                      # 2^-10 in units of 2^-71
    return {b: v[1] // unit for b, v in got[0][0].items() if v[1]}, got[1][0][0]


@pytest.mark.parametrize("strand", "+-")
def test_known_insertions(strand):
    """One row per start 9 .. 58, offset 1: 49 count; per class cell of p = 2^-10."""
    cells, n_rows = _known(strand, 0, range(9, 59), "1,2,3,4-6", 5)
    assert n_rows == 49
    # 4 classes per row: utr5 5 rows, start_lost 2, splice 4, intron 14, utr3 5; the 19 frame rows: classes 1, 2 shift, 3 keeps, 4-6 is mixed
    assert cells == dict(utr5=20, start_lost=8, splice=16, intron=56, utr3=20, frameshift=38, inframe=19, cds_mixed=19)
    one, n_rows = _known(strand, 0, range(9, 59), "1", 2)
    assert n_rows == 49 and one == dict(utr5=5, start_lost=2, splice=4, intron=14, utr3=5, frameshift=19)


def test_known_insertion_boundaries():
    for js, want in (((11, 15), "utr5"), ((16, 17), "start_lost"), ((18, 20, 30, 40, 50, 54), "inframe"), ((21, 29, 41, 49), "splice"),
                     ((22, 28, 42, 48), "intron"), ((55, 59), "utr3")):
        for j in js:
            assert _known("+", 0, [j - 1], "3", 2) == ({want: 1}, 1), j
    assert _known("+", 0, [9], "3", 2) == ({}, 0) and _known("+", 0, [59], "3", 2) == ({}, 0)      # base j - 1 or base j outside the span
    assert _known("+", 0, [11], "3", 2, off=0) == ({"utr5": 1}, 1) and _known("+", 0, [10], "3", 2, off=0) == ({}, 0)


def test_known_deletions():
    for kind, length, j, want in ((1, 3, 18, "splice"), (1, 3, 31, "inframe"), (1, 2, 14, "start_lost"), (1, 3, 53, "frameshift"),
                                  (2, 3, 33, "inframe"), (2, 3, 31, "splice")):
        assert _known("+", kind, [j - 1], str(length), 2) == ({want: 1}, 1), (kind, length, j)
        assert _known("+", kind, [j], str(length), 2, off=0) == ({want: 1}, 1)


def test_structure_links_round_trip(record):
    from mural_amd import tables
    f = record["features"]
    prev, nxt = tables.structure_links(f)
    assert prev.dtype == np.int32 and nxt.dtype == np.int32 and len(prev) == len(nxt) == len(f["feat_b0"])
    seen = 0
    for t in np.unique(f["feat_tx"]):
        mine = np.nonzero(f["feat_tx"] == t)[0]
        first = [i for i in mine if prev[i] < 0]
        assert len(first) == 1
        walk, at = [], first[0]
        while at >= 0:
            walk.append(at)
            assert f["feat_tx"][at] == t and (nxt[at] < 0 or (prev[nxt[at]] == at and f["feat_b0"][nxt[at]] == f["feat_b1"][at]))
            at = nxt[at]
        assert sorted(walk) == sorted(mine.tolist())
        seen += len(walk)
    assert seen == len(prev)
    before = {k: v.copy() for k, v in f.items()}
    tables.structure_links(f)
    assert set(f) == set(before) and all(np.array_equal(f[k], before[k]) for k in f)      # the features are left as they are
    assert len(tables.read_transcript_structure(io.StringIO(record["text"]))) == 4


def test_broken_links_end_the_walk(record):
    """A link out of range or into another transcript: the walk ends there, nothing else changes."""
    from mural_amd import tables
    prob, start, label = I.rows(record["seq"], 8, seed=2, dtype=np.float32)
    prev, nxt = tables.structure_links(record["features"])
    want = _twin(record, prob, start, label, 8, 1, 1, None)
    bad = nxt.copy()
    bad[5], bad[40], bad[41] = len(nxt) + 3, -7, int(np.nonzero(record["features"]["feat_tx"] != record["features"]["feat_tx"][41])[0][0])
    got = _twin(record, prob, start, label, 8, 1, 1, None, links=(prev, bad))
    assert got[2] == 0 and got[1].tobytes() == want[1].tobytes() and got[0].tobytes() != want[0].tobytes()
    assert int(got[0][:, :, 0].sum()) == int(want[0][:, :, 0].sum())


def test_refusals(record):
    from mural_amd import tables
    from mural_amd.predict import SummarySink
    prob, start, label = I.rows(record["seq"], 8, seed=2, dtype=np.float32)
    for k, kind, off, spec, match in ((1, 0, 1, None, "2 .. 16"), (17, 0, 1, None, "2 .. 16"), (8, 3, 1, None, "indel_kind"), (8, "ins", 1, None, "indel_kind"),
                                      (8, 0, 2, None, "breakpoint_offset"), (5, 0, 1, None, "need their own"), (8, 0, 1, "1,2,3", "entries"),
                                      (5, 0, 1, "0,1,2,3", "lo <= hi"), (5, 0, 1, "1,2,3,65", "lo <= hi"), (5, 0, 1, "1,2,5-4,6", "lo <= hi"),
                                      (5, 0, 1, "1,2,x,6", "neither")):
        with pytest.raises(ValueError, match=match):
            _twin(record, prob[:, :max(k, 2)] if k <= 8 else np.zeros((len(start), k)), start, label, k, kind, off, spec)
    assert tables.check_indel_lengths(None, 8).tolist() == [[0, 0], [1, 1], [2, 2], [3, 3], [4, 4], [5, 5], [6, 6], [7, 20]]
    assert tables.check_indel_lengths([1, (2, 3)]).tolist() == [[0, 0], [1, 1], [2, 3]]
    assert tables.check_indel_lengths(np.array([(1, 1), (2, 3)])).tolist() == [[0, 0], [1, 1], [2, 3]]      # an array of pairs is a sequence of pairs
    assert tables.check_indel_lengths(np.array([4, 5])).tolist() == [[0, 0], [4, 4], [5, 5]]
    own = tables.check_indel_lengths("1,2,4-6")
    assert tables.check_indel_lengths(own, 4).tolist() == own.tolist() == [[0, 0], [1, 1], [2, 2], [4, 6]]     # its own result: row 0 is no class
    with pytest.raises(ValueError, match="lo <= hi"):
        tables.check_indel_lengths(np.array([(0, 1), (2, 3)]))
    assert [tables.check_indel_kind(v) for v in ("insertion", "deletion_start", "deletion_end", 2)] == [0, 1, 2, 2]
    # bad rows are skipped and set the status bits; class 0's probability is never read
    want = _twin(record, prob, start, label, 8, 2, 1, None)
    for at, col, value, bit in ((7, None, -3, 1), (900, "label", 8, 2), (901, 3, np.nan, 8), (902, 7, 1.5, 8)):
        p, s, lab = prob.copy(), start.copy(), label.copy()
        if col is None:
            s[at] = value
        elif col == "label":
            lab[at] = value
        else:
            p[at, col] = value
        p[at + 1, 0] = np.nan
        keep = np.arange(len(s)) != at
        got = _twin(record, p, s, lab, 8, 2, 1, None)
        less = _twin(record, prob[keep], start[keep], label[keep], 8, 2, 1, None)
        assert got[2] == bit and got[0].tobytes() == less[0].tobytes() and got[1].tobytes() == less[1].tobytes() != want[1].tobytes()
    # the sink
    tx = record["tx"]
    with pytest.raises(ValueError, match="indel_kind"):
        SummarySink(None, indel_transcripts=tx)
    with pytest.raises(ValueError, match="go with indel_transcripts"):
        SummarySink(None, windows=(100,), indel_kind="insertion")
    with pytest.raises(ValueError, match="go with indel_transcripts"):
        SummarySink(None, windows=(100,), breakpoint_offset=0)
    with pytest.raises(ValueError, match="breakpoint_offset"):
        SummarySink(None, indel_transcripts=tx, indel_kind=0, breakpoint_offset=2)
    with pytest.raises(ValueError, match="lo <= hi"):
        SummarySink(None, indel_transcripts=tx, indel_kind=0, indel_lengths="1,99")
    shard = {"chrom": "chr1", "start": start, "end": start + 1, "strand": np.zeros(len(start), np.uint8), "label": label, "prob": prob,
             "n_class": 8, "calibrated": False}
    with pytest.raises(ValueError, match="entries"):
        SummarySink(None, indel_transcripts=tx, indel_kind=0, indel_lengths="1,2")(shard)
    with pytest.raises(ValueError, match="INDEL tables are out of scope"):      # transcripts= keeps refusing INDEL rows, word for word
        SummarySink(None, transcripts=tx[:3], genome=lambda name: record["seq"])(shard)


def test_sink_on_the_host_and_the_writer(record, tmp_path):
    from mural_amd import tables
    from mural_amd.predict import SummarySink
    prob, start, label = I.rows(record["seq"], 8, seed=4, dtype=np.float32)
    sink = SummarySink(str(tmp_path / "s"), indel_transcripts=record["tx"], indel_kind="deletion_start", genome=lambda name: record["seq"])
    for part in np.array_split(np.random.default_rng(1).permutation(len(start)), 3):
        sink({"chrom": "chr1", "start": start[part], "end": start[part] + 1, "strand": np.zeros(len(part), np.uint8), "label": label[part],
              "prob": prob[part], "n_class": 8, "calibrated": False})
    sink.close()
    want = _twin(record, prob, start, label, 8, 1, 1, None, chrom_length=len(record["seq"]))
    names, table, rows = sink.result()["indel_structure"]
    assert names == record["names"] and table.tobytes() == want[0].tobytes() and rows.tobytes() == want[1].tobytes()
    assert sink.indel_structure_sums()[0] is table
    lines = (tmp_path / "s.indel_structure.tsv").read_text().splitlines()
    header = lines[0].split("\t")
    want_header = ["name", "chrom", "strand", "kind", "n_rows", "n_nonmut"]
    for what in I.BINS + ("lof", "lof_upper"):
        want_header += [f"expected_{what}", f"observed_{what}"]
    assert header == want_header and len(lines) == 1 + len(names)
    col = {h: i for i, h in enumerate(header)}
    for t, line in enumerate(lines[1:]):
        f = line.split("\t")
        cells = table[t].tolist()
        assert f[:6] == [names[t], record["tx"][1]["chrom"][t], "-" if record["tx"][1]["strand"][t] else "+", "deletion_start",
                         str(int(rows[t, 0])), str(int(rows[t, 1]))]
        value = lambda bins: sum((cells[b][1] << 40) + cells[b][2] for b in bins)      # noqa: E731
        assert f[col["observed_lof"]] == str(sum(cells[b][0] for b in (3, 6, 7)))
        assert f[col["observed_lof_upper"]] == str(sum(cells[b][0] for b in (3, 6, 7, 9)))
        assert f[col["expected_lof"]] == tables._float_text(value((3, 6, 7)) / (1 << 71))
        assert f[col["expected_lof_upper"]] == tables._float_text(value((3, 6, 7, 9)) / (1 << 71))
        assert f[col["expected_frameshift"]] == tables._float_text(value((7,)) / (1 << 71))
    path = tables.write_indel_structure_outputs(names, record["tx"][1], table, rows, 1, str(tmp_path / "na"), labels=False)
    na = open(path).read().splitlines()[1].split("\t")
    assert path == str(tmp_path / "na.indel_structure.tsv") and set(na[7::2]) == {"NA"} and na[6::2] == lines[1].split("\t")[6::2]


def test_the_lof_sum_is_added_as_integers(tmp_path):
    """Three cells whose float64 values do not add up exactly: the writer adds the limbs first."""
    from mural_amd import tables
    table = np.zeros((1, 10, 3), np.uint64)
    table[0, 3], table[0, 6], table[0, 7] = (1, 1 << 30, 1), (2, 0, 3), (4, 5, (1 << 40) - 1)
    meta = dict(chrom=["chr1"], strand=np.zeros(1, np.uint8))
    f = open(tables.write_indel_structure_outputs(["t"], meta, table, np.array([[9, 2]], np.uint64), "insertion", str(tmp_path / "x"))).read()
    f = f.splitlines()[1].split("\t")
    total = ((1 << 30) << 40) + 1 + 3 + (5 << 40) + (1 << 40) - 1
    assert f[3:6] == ["insertion", "9", "2"] and f[6 + 2 * 10] == tables._float_text(total / (1 << 71)) and f[7 + 2 * 10] == "7"


def test_command_line_refusals(tmp_path):
    spec = importlib.util.spec_from_file_location("predict_files", os.path.join(ROOT, "tools", "predict_files.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    bed = tmp_path / "tx.bed"
    bed.write_text(I.KNOWN % "+")
    base = ["model", "genome.fa", str(tmp_path / "out.tsv"), "--regions", "chr1:1-100", "--summary", str(tmp_path / "s")]
    for extra, match in ((["--indel_transcripts", str(bed), "--indel_kind", "insertion"], "goes with --indel"),
                         (["--indel", "--indel_transcripts", str(bed)], "needs --indel_kind"),
                         (["--indel", "--window_size", "100", "--indel_kind", "insertion"], "go with --indel_transcripts"),
                         (["--indel", "--window_size", "100", "--breakpoint_offset", "0"], "go with --indel_transcripts"),
                         (["--indel", "--indel_transcripts", str(bed), "--indel_kind", "inversion"], "indel_kind"),
                         (["--indel", "--indel_transcripts", str(bed), "--indel_kind", "insertion", "--breakpoint_offset", "2"], "breakpoint_offset"),
                         (["--indel", "--indel_transcripts", str(bed), "--indel_kind", "insertion", "--indel_lengths", "1,0"], "lo <= hi"),
                         (["--indel", "--indel_transcripts", str(tmp_path / "none.bed"), "--indel_kind", "insertion"], "--indel_transcripts"),
                         (["--indel", "--transcripts", str(bed)], "--transcripts takes SNV rows: it does not go with --indel"),
                         (["--indel", "--transcripts", str(bed), "--transcript_structure"], "--transcript_structure takes SNV rows: it does not go with --indel")):
        with pytest.raises(SystemExit, match=match):
            mod.main(base + extra)
    with pytest.raises(SystemExit, match="needs --summary PREFIX"):
        mod.main(base[:5] + ["--indel", "--indel_transcripts", str(bed), "--indel_kind", "insertion"])
    assert not (tmp_path / "out.tsv").exists()


def test_the_reduce_kernel_reports_no_scratch():
    path = os.path.join(ROOT, "mural_amd", "csrc", "summary_txindel.resources.txt")
    text = open(path).read()
    blocks = text.split("Function Name: ")[1:]
    reduce = [b for b in blocks if "summary_txindel_reduce_kernel" in b.splitlines()[0]]
    assert len(reduce) == 2                                                            # float and double
    for b in blocks:
        assert "ScratchSize [bytes/lane]: 0" in b, b.splitlines()[0]
    make = open(os.path.join(ROOT, "mural_amd", "csrc", "Makefile")).read()
    assert "summary_txindel" in next(ln for ln in make.splitlines() if ln.startswith("REPORTED")).split()


def test_read_chrom_lengths(tmp_path):
    from mural_amd import tables
    fai = tmp_path / "g.fa.fai"
    fai.write_text("chr1\t3400\t6\t60\t61\nchr2\t17\t3500\t60\t61\n")
    assert tables.read_chrom_lengths(str(fai)) == {"chr1": 3400, "chr2": 17} and tables.read_chrom_lengths({"a": 1}) == {"a": 1}
    fai.write_text("chr1\tlong\n")
    with pytest.raises(ValueError, match="length"):
        tables.read_chrom_lengths(str(fai))
