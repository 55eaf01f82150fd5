"""The consequence table on the host: ``tables.read_transcripts`` (BED12 -> CDS segments) and the numpy twin ``summary_conseq_host``
against the brute-force oracle of tests/_conseq_data.py (Python integers and strings), the known answers of the standard code, both
strands, codons that straddle one and two splice junctions, incomplete and masked codons, the status bits, the reader's refusals,
non-default codon table and alternative order, and the table's invariance under any split of the rows."""
import gzip
import io

import numpy as np
import pytest

from tests import _conseq_data as D


def _tables():
    from mural_amd import tables
    return tables


def _twin(seq, segments, n_tx, prob, start, strand, label, **kw):
    from mural_amd.summaries import summary_conseq_host
    return summary_conseq_host(seq, prob, start, strand, label, segments, n_tx, **kw)


@pytest.fixture(scope="module")
def record(tmp_path_factory):
    seq, text, names = D.build()
    path = tmp_path_factory.mktemp("tx") / "tx.bed"
    path.write_text(text)
    got_names, meta, segments = _tables().read_transcripts(str(path))
    assert got_names == names
    return dict(seq=seq, text=text, names=names, meta=meta, segments=segments, path=path)


def _single(cds, strand="+", sizes=(), p=2.0 ** -10, row_strand=0, code=None, alt_order=None):
    """Twin and oracle tables of ONE transcript whose CDS is `cds`, every base a row: ({bin: (count, sum)}, counters)."""
    rng = np.random.default_rng(1)
    body = cds if strand == "+" else D.revcomp(cds)
    piece, blocks = D._cut(body, list(sizes), rng, 5)
    seq = "ACGTA" + piece + "TTGCA"
    text = D.bed12("chr1", "t", strand, blocks) + "\n"
    _, meta, segments = _tables().read_transcripts(io.StringIO(text), code)
    start = np.array([q for a, b in blocks for q in range(a, b)], np.int64)
    n = len(start)
    prob = np.full((n, 4), p)
    label = (np.arange(n) % 4).astype(np.int64)
    rs = np.full(n, row_strand, np.uint8)
    table, counters, status = _twin(seq, segments["chr1"], 1, prob, start, rs, label, aa=meta["aa"], alt_order=alt_order)
    assert status == 0
    kw = {}
    if code is not None:
        kw["code"] = code
    if alt_order is not None:
        kw["alt"] = {"ACGT"[r]: "".join("ACGT"[a] for a in np.asarray(_tables().check_alt_order(alt_order))[r]) for r in range(4)}
    want = D.oracle(seq, text, prob, start, rs, label, **kw)
    got = D.as_integers(table, counters)
    assert got == want
    return got[0][0], got[1][0], table


def _pairs(cell):
    """{bin: number of (row, class) pairs} of a cell whose every probability is 2^-10."""
    return {b: v[1] >> 61 for b, v in cell.items()}


# ---- 1. known answers --------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("strand", ["+", "-"])
@pytest.mark.parametrize("sizes", [(), (1, 1, 2, 3, 1, 1, 1, 4, 2, 1, 5, 1, 1, 2, 7)])
def test_the_64_codons_of_the_standard_code(strand, sizes):
    """576 (row, class) pairs: syn 138, mis 392, stop gained 23, stop lost 23; on '-', and cut into blocks of 1, 1, 2, 3, ... bases
    (codons straddle one and two junctions) the table is the same."""
    cell, counters, table = _single(D.ALL_CODONS, strand, sizes)
    assert _pairs(cell) == {"syn": 138, "mis": 392, "stop_gained": 23, "stop_lost": 23, "unresolved": 0}
    assert counters == [192, 48]
    den = 1 << 71
    expected = [((int(h) << 40) + int(l)) / den for _, h, l in table[0].tolist()]
    assert expected == [138 * 2.0 ** -10, 392 * 2.0 ** -10, 23 * 2.0 ** -10, 23 * 2.0 ** -10, 0.0]
    plain, _, plain_table = _single(D.ALL_CODONS)
    assert np.array_equal(table[:, :, 1:], plain_table[:, :, 1:])


@pytest.mark.parametrize("codon,want", [("ATG", dict(mis=9)), ("TGG", dict(mis=7, stop_gained=2)), ("TAA", dict(syn=2, stop_lost=7)),
                                        ("AAA", dict(syn=1, mis=7, stop_gained=1))])
@pytest.mark.parametrize("strand,row_strand", [("+", 0), ("-", 0), ("+", 1), ("-", 1)])
def test_single_codons(codon, want, strand, row_strand):
    """Every strand of transcript and row: the nine substitutions of a codon are the same set, whatever the strand names them on."""
    cell, counters, _ = _single(codon, strand, row_strand=row_strand)
    full = dict(syn=0, mis=0, stop_gained=0, stop_lost=0, unresolved=0)
    full.update(want)
    assert _pairs(cell) == full and counters[0] == 3


def test_rows_on_the_minus_strand_take_their_alternatives_from_their_own_base():
    """Codon GAA on '+'.  Row at the G on '-': own base C, classes C>A, C>G, C>T = G>T, G>C, G>A on the reference: TAA stop | CAA Q | AAA K
    -- class 1 is the stop.  On '+' (own base G: G>A, G>C, G>T) class 3 is."""
    seq, text = "GAA", D.bed12("chr1", "t", "+", [(0, 3)]) + "\n"
    _, meta, segments = _tables().read_transcripts(io.StringIO(text))
    for rs, stop_class in ((1, 1), (0, 3)):
        prob = np.array([[0.0, 0.25, 0.5, 0.125]])
        for lab in (1, 2, 3):
            table, _, _ = _twin(seq, segments["chr1"], 1, prob, np.array([0]), np.array([rs], np.uint8), np.array([lab]))
            assert int(table[0, 2, 0]) == (lab == stop_class) and int(table[0, 1, 0]) == (lab != stop_class)
            assert int(table[0, 2, 1]) == int(prob[0, stop_class] * 2 ** 31)


def test_non_default_codon_table_and_alt_order():
    code = D.CODE.replace("W", "*")                 # TGG a stop as well
    cell, _, _ = _single("TGG", code=code)
    assert _pairs(cell)["stop_lost"] == 7 and _pairs(cell)["syn"] == 2
    order = "TGC,TGA,TCA,GCA"                       # descending
    a, _, ta = _single(D.ALL_CODONS, alt_order=order)
    b, _, tb = _single(D.ALL_CODONS)
    assert _pairs(a) == _pairs(b) and not np.array_equal(ta[:, :, 0], tb[:, :, 0])      # the same pairs, other classes
    T = _tables()
    assert np.array_equal(T.check_alt_order("CGT,AGT,ACT,ACG"), T.check_alt_order(None))
    for bad in ("AGT,AGT,ACT,ACG", "CCT,AGT,ACT,ACG", "CGT,AGT,ACT", np.zeros((4, 3), int)):
        with pytest.raises(ValueError):
            T.check_alt_order(bad)
    with pytest.raises(ValueError):
        T.check_codon_table("K" * 63)


# ---- 2. the record: nested, overlapping, both strands, incomplete and masked codons ----------------------------------------------------------
@pytest.mark.parametrize("dtype", [np.float64, np.float32])
def test_twin_equals_the_oracle_on_the_record(record, dtype):
    prob, start, strand, label = D.rows(record["seq"], dtype=dtype)
    table, counters, status = _twin(record["seq"], record["segments"]["chr1"], len(record["names"]), prob, start, strand, label)
    assert status == 0
    got = D.as_integers(table, counters)
    want = D.oracle(record["seq"], record["text"], prob, start, strand, label)
    assert got == want
    cells = dict(zip(record["names"], got[0]))
    counts = dict(zip(record["names"], got[1]))
    assert cells["codons_plus"]["unresolved"] == [0, 0] and counts["noncoding"] == [0, 0] and counts["elsewhere"] == [0, 0]
    for nm in ("outer_plus", "inner_minus", "past_the_end"):      # 3 k + 1, 3 k + 2 with masked bases, a codon past the record
        assert cells[nm]["unresolved"][1] > 0, nm
    assert cells["same_blocks_plus"] != cells["overlap_minus"] and counts["same_blocks_plus"] == counts["overlap_minus"]
    assert len(record["segments"]["chr1"]["seg_b0"]) > 300 and len(record["names"]) > 40


def test_cds_length_remainders_and_the_record_end(record):
    meta, names = record["meta"], record["names"]
    assert meta["cds_length"][names.index("outer_plus")] % 3 == 1 and meta["cds_length"][names.index("inner_minus")] % 3 == 2
    assert meta["cds_length"][names.index("noncoding")] == 0 and meta["n_segments"][names.index("noncoding")] == 0
    assert meta["n_segments"][names.index("utr_only_block")] == 1          # one block is UTR, one is past thickEnd
    # the trailing bases of a 3 k + 2 CDS: on '-' they are the lowest genomic positions of the first segment
    seq, text = "ACGTACGTAC", D.bed12("chr1", "t", "-", [(1, 9)]) + "\n"
    _, meta, segments = _tables().read_transcripts(io.StringIO(text))
    prob = np.full((10, 4), 0.25)
    table, counters, _ = _twin(seq, segments["chr1"], 1, prob, np.arange(10), None, np.zeros(10, np.int64))
    assert counters.tolist() == [[8, 8]]
    assert int(table[0, 4, 1]) == 2 * 3 * (1 << 29) and int(table[0, :4, 1].sum()) == 6 * 3 * (1 << 29)


def test_an_n_inside_a_codon_and_a_codon_at_the_record_end():
    text = D.bed12("chr1", "t", "+", [(0, 9)]) + "\n"
    _, meta, segments = _tables().read_transcripts(io.StringIO(text))
    prob, lab = np.full((9, 4), 0.5), np.ones(9, np.int64)
    table, _, _ = _twin("ATGANGTTT", segments["chr1"], 1, prob, np.arange(9), None, lab)
    assert int(table[0, 4, 0]) == 3 and int(table[0, :4, 0].sum()) == 6
    table, _, _ = _twin("ATGAAGTT", segments["chr1"], 1, prob[:8], np.arange(8), None, lab[:8])      # the record ends inside the last codon
    assert int(table[0, 4, 0]) == 2 and int(table[0, :4, 0].sum()) == 6


# ---- 3. status, equal starts, split invariance ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("what,bit", [("start", 1), ("label", 2), ("nan", 8), ("above", 8), ("negative", 8)])
def test_each_status_bit_skips_its_row(record, what, bit):
    prob, start, strand, label = D.rows(record["seq"], seed=3)
    at = 40                                                    # inside codons_plus
    want = _twin(record["seq"], record["segments"]["chr1"], len(record["names"]), np.delete(prob, at, 0), np.delete(start, at),
                 np.delete(strand, at), np.delete(label, at))
    if what == "start":
        start = start.copy()
        start[at] = -5
    elif what == "label":
        label[at] = 4
    else:
        prob[at, 2] = dict(nan=np.nan, above=1.5, negative=-0.25)[what]
    prob[at + 1, 0] = np.nan                                   # class 0's probability is never read
    got = _twin(record["seq"], record["segments"]["chr1"], len(record["names"]), prob, start, strand, label)
    assert got[2] == bit and want[2] == 0
    assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1])


def test_equal_starts_count_once_each(record):
    prob, start, strand, label = D.rows(record["seq"], seed=4, extra=0)
    twice = _twin(record["seq"], record["segments"]["chr1"], len(record["names"]), np.repeat(prob, 2, 0), np.repeat(start, 2),
                  np.repeat(strand, 2), np.repeat(label, 2))
    once = _twin(record["seq"], record["segments"]["chr1"], len(record["names"]), prob, start, strand, label)
    assert np.array_equal(twice[1], 2 * once[1]) and np.array_equal(twice[0][:, :, 0], 2 * once[0][:, :, 0])
    assert D.as_integers(*twice[:2])[0] == [{b: [2 * v[0], 2 * v[1]] for b, v in cell.items()} for cell in D.as_integers(*once[:2])[0]]


def test_the_table_is_the_same_for_any_split_of_the_rows(record):
    prob, start, strand, label = D.rows(record["seq"], seed=5, dtype=np.float32)
    n, n_tx, segs = len(start), len(record["names"]), record["segments"]["chr1"]
    whole = _twin(record["seq"], segs, n_tx, prob, start, strand, label)
    rng = np.random.default_rng(5)
    cuts = np.sort(rng.choice(np.arange(1, n), size=9, replace=False))
    for parts in ([np.arange(i, min(i + 64, n)) for i in range(0, n, 64)], np.split(rng.permutation(n), cuts)):
        into = None
        for part in parts:
            table, counters, status = _twin(record["seq"], segs, n_tx, prob[part], start[part], strand[part], label[part], into=into)
            into = (table, counters)
            assert status == 0
        assert into[0].tobytes() == whole[0].tobytes() and into[1].tobytes() == whole[1].tobytes()


def test_four_classes_only(record):
    prob, start, strand, label = D.rows(record["seq"])
    with pytest.raises(ValueError, match="4 classes"):
        _twin(record["seq"], record["segments"]["chr1"], len(record["names"]), prob, start, strand, label, n_class=2)


# ---- 4. the reader ------------------------------------------------------------------------------------------------------------------------------
def test_reader_layout(record):
    segs, meta = record["segments"]["chr1"], record["meta"]
    key = list(zip(segs["seg_b0"].tolist(), segs["seg_b1"].tolist(), segs["seg_tx"].tolist()))
    assert key == sorted(key) and set(record["segments"]) == {"chr1", "chr9"}
    assert segs["seg_b0"].dtype == segs["seg_cds0"].dtype == np.int64 and segs["seg_tx"].dtype == segs["seg_prev"].dtype == np.int32
    assert segs["tx_strand"].dtype == np.uint8 and segs["tx_cds_len"].dtype == np.int64 and meta["aa"].tobytes().decode() == D.CODE
    for t in range(len(record["names"])):
        mine = np.nonzero(segs["seg_tx"] == t)[0]
        if meta["chrom"][t] != "chr1":
            assert len(mine) == 0
            continue
        assert len(mine) == meta["n_segments"][t]
        if len(mine) == 0:
            continue
        first = [s for s in mine if segs["seg_prev"][s] < 0]
        assert len(first) == 1
        s, done, seen = first[0], 0, 0
        while s >= 0:                                           # the chain in transcript orientation covers the CDS once
            assert segs["seg_cds0"][s] == done
            done += segs["seg_b1"][s] - segs["seg_b0"][s]
            nxt = segs["seg_next"][s]
            if nxt >= 0:
                assert segs["seg_prev"][nxt] == s
                assert (segs["seg_b0"][nxt] < segs["seg_b0"][s]) == bool(meta["strand"][t])
            s, seen = nxt, seen + 1
        assert done == meta["cds_length"][t] and seen == len(mine)


def test_reader_takes_gzip_handles_and_its_own_result(record, tmp_path):
    T = _tables()
    gz = tmp_path / "tx.bed.gz"
    with gzip.open(gz, "wt") as fh:
        fh.write(record["text"])
    for source in (str(gz), io.StringIO(record["text"]), io.BytesIO(record["text"].encode()), open(record["path"])):
        names, meta, segments = T.read_transcripts(source)
        assert names == record["names"]
        for key, v in record["segments"]["chr1"].items():
            assert np.array_equal(segments["chr1"][key], v), key
    again = T.read_transcripts((record["names"], record["meta"], record["segments"]))
    assert again[2] is record["segments"]


@pytest.mark.parametrize("text,line,what", [
    (D.bed12("chr1", "a", "+", [(0, 9)]) + "\n" + D.bed12("chr1", "a", "-", [(20, 29)]), 3, "duplicate"),
    (D.bed12("chr1", "a", ".", [(0, 9)]), 2, "strand"),
    (D.bed12("chr1", "a", "+", [(0, 9), (5, 12)]), 2, "overlap"),
    ("chr1\t0\t20\ta\t0\t+\t0\t20\t0\t2\t5,5,\t10,0,", 2, "ascend"),
    ("chr1\t0\t20\ta\t0\t+\t0\t20\t0\t2\t5,15,\t0,10,", 2, "leaves"),
    ("chr1\t0\t20\ta\t0\t+\t0\t20", 2, "12 columns"),
])
def test_reader_refusals_name_the_line(text, line, what):
    with pytest.raises(ValueError, match=rf"<transcripts>:{line}: .*{what}"):
        _tables().read_transcripts(io.StringIO("# header\n" + text + "\n"))


# ---- 5. the sink on host shards and the file ------------------------------------------------------------------------------------------------
def test_sink_on_host_shards_writes_the_table(record, tmp_path):
    from mural_amd.predict import SummarySink
    prob, start, strand, label = D.rows(record["seq"], seed=6, dtype=np.float32)
    want = _twin(record["seq"], record["segments"]["chr1"], len(record["names"]), prob, start, strand, label)
    for labels in (True, False):
        sink = SummarySink(str(tmp_path / f"s{int(labels)}"), transcripts=str(record["path"]), genome=lambda name: record["seq"],
                           annotations={"chr1": [(0, 500, "first")]}, transcript_labels=labels)
        for part in np.array_split(np.arange(len(start)), 3):
            sink({"chrom": "chr1", "start": start[part], "end": start[part] + 1, "strand": strand[part], "label": label[part].astype(np.float32),
                  "prob": prob[part], "n_class": 4, "calibrated": False, "aligned": True})
        sink.close()
        table, counters = sink.consequence_sums()
        assert table.tobytes() == want[0].tobytes() and counters.tobytes() == want[1].tobytes()
        lines = (tmp_path / f"s{int(labels)}.consequence.mut_rates.tsv").read_text().splitlines()
        assert lines[0].split("\t") == ["name", "chrom", "strand", "cds_length", "n_rows", "n_nonmut", "n_unresolved", "expected_syn",
                                        "observed_syn", "expected_mis", "observed_mis", "expected_stop_gained", "observed_stop_gained",
                                        "expected_stop_lost", "observed_stop_lost"]
        assert [ln.split("\t")[0] for ln in lines[1:]] == record["names"]
        row = lines[1 + record["names"].index("codons_minus")].split("\t")
        assert row[1:5] == ["chr1", "-", "192", str(int(want[1][1, 0]))]
        assert row[8] == (str(int(want[0][1, 0, 0])) if labels else "NA")
        assert float(row[7]) == pytest.approx(((int(want[0][1, 0, 1]) << 40) + int(want[0][1, 0, 2])) / 2 ** 71, rel=1e-5)
    with pytest.raises(ValueError, match="genome"):
        SummarySink(None, transcripts=str(record["path"]))
    with pytest.raises(ValueError, match="transcripts"):
        SummarySink(None, codon_table=D.CODE)
    sink = SummarySink(None, transcripts=str(record["path"]), genome=lambda name: record["seq"])
    with pytest.raises(ValueError, match="4 classes"):
        sink({"chrom": "chr1", "start": start[:5], "end": start[:5] + 1, "strand": strand[:5], "label": np.zeros(5, np.float32),
              "prob": prob[:5, :2], "n_class": 2, "calibrated": False, "aligned": True})
