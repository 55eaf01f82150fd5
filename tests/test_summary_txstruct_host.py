"""The structure table on the host: ``tables.read_transcript_structure`` (BED12 -> items that tile each transcript's span) and the numpy
twin ``summary_txstruct_host`` against the brute-force oracle of tests/_txstruct_data.py (Python integers and strings), the known answer
of a three-exon transcript on both strands, the defining identity with ``summary_conseq_host``, the status bits, the table's invariance
under any split of the rows, the reader's layout and refusals, the sink on host shards with its file, and the build's resource report."""
import gzip
import io
import os

import numpy as np
import pytest

from tests import _conseq_data as D
from tests import _txstruct_data as S

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _tables():
    from mural_amd import tables
    return tables


def _twin(seq, tx, chrom, prob, start, strand, label, **kw):
    from mural_amd.summaries import summary_txstruct_host
    return summary_txstruct_host(seq, prob, start, strand, label, tx[2].get(chrom), tx[3].get(chrom), len(tx[0]), **kw)


@pytest.fixture(scope="module")
def record(tmp_path_factory):
    seq, text, names = S.build()
    path = tmp_path_factory.mktemp("tx") / "tx.bed"
    path.write_text(text)
    tx = _tables().read_transcript_structure(str(path))
    assert tx[0] == names
    return dict(seq=seq, text=text, names=names, tx=tx, path=path)


# ---- 1. the oracle --------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", [np.float64, np.float32])
def test_twin_equals_the_oracle_on_the_record(record, dtype):
    prob, start, strand, label = S.rows(record["seq"], dtype=dtype)
    table, counters, status = _twin(record["seq"], record["tx"], "chr1", prob, start, strand, label)
    assert status == 0
    got = S.as_integers(table, counters)
    want = S.oracle(record["seq"], record["text"], prob, start, strand, label)
    assert got == want
    cells, counts = dict(zip(record["names"], got[0])), dict(zip(record["names"], got[1]))
    assert counts["elsewhere"] == [0, 0] and counts["noncoding"][0] > 0
    assert all(v == [0, 0] for b, v in cells["noncoding"].items() if b not in ("noncoding_exon", "splice_utr", "intron"))
    for b in S.BINS:                                             # every bin is reached
        assert sum(c[b][1] for c in got[0]) > 0, b
    for tag in "pm":
        one = cells[f"one_exon_{tag}"]
        assert one["utr5"][1] > 0 and one["utr3"][1] > 0 and one["intron"] == [0, 0] and counts[f"one_exon_{tag}"][0] >= 100
        assert cells[f"short_introns_all_cds_{tag}"]["splice_donor"][1] > 0 and cells[f"short_introns_all_cds_{tag}"]["intron"][1] > 0
        assert cells[f"thick_at_block_start_{tag}"]["splice_utr"][1] > 0 and cells[f"thick_at_block_start_{tag}"]["splice_donor"][1] > 0
        assert cells[f"thick_at_block_end_{tag}"]["splice_donor"] == [0, 0]
        assert cells[f"short_cds_{tag}"]["start_lost"] == [0, 0] and cells[f"short_cds_{tag}"]["cds"][1] > 0      # cds_length < 3
    assert counts["gaps_at_the_ends"][0] >= 60 and cells["gaps_at_the_ends"]["splice_utr"][1] > 0


# ---- 2. the known answer ----------------------------------------------------------------------------------------------------------------------
def _known(strand, thick=(15, 55)):
    """Blocks [10,20) [30,40) [50,60) with a row at every base 10 .. 59, every p_c = 2^-10, ATG as the first codon in transcript
    orientation: ({bin: (row, class) pairs}, counters)."""
    seq = list("".join(np.random.default_rng(3).choice(list("CGT"), size=70)))
    if strand == "+":
        seq[thick[0]:thick[0] + 3] = "ATG"
    else:
        seq[thick[1] - 3:thick[1]] = D.revcomp("ATG")
    seq = "".join(seq)
    text = D.bed12("chr1", "t", strand, [(10, 20), (30, 40), (50, 60)], thick) + "\n"
    tx = _tables().read_transcript_structure(io.StringIO(text))
    start = np.arange(10, 60)
    prob, label = np.full((50, 4), 2.0 ** -10), np.zeros(50, np.int64)
    table, counters, status = _twin(seq, tx, "chr1", prob, start, None, label)
    assert status == 0 and S.as_integers(table, counters) == S.oracle(seq, text, prob, start, None, label)
    return {b: v[1] >> 61 for b, v in S.as_integers(table, counters)[0][0].items()}, counters.tolist()


@pytest.mark.parametrize("strand", ["+", "-"])
def test_known_answer(strand):
    """Rows per bin: utr5 5, utr3 5, donor 4, acceptor 4, intron 12, splice_utr 0; over the 20 CDS rows start_lost 9 and cds 51 class
    cells (ATG: all nine substitutions change the amino acid).  '-' mirrors it: the 5'UTR is [55, 60)."""
    pairs, counters = _known(strand)
    assert pairs == dict(utr5=15, utr3=15, noncoding_exon=0, splice_donor=12, splice_acceptor=12, splice_utr=0, intron=36, start_lost=9,
                         cds=51)
    assert counters == [[50, 50]]


def test_moving_thick_start_turns_the_first_introns_sites_into_splice_utr():
    pairs, _ = _known("+", (35, 55))
    assert pairs["splice_utr"] == 12 and pairs["splice_donor"] == 6 and pairs["splice_acceptor"] == 6 and pairs["intron"] == 36
    assert pairs["utr5"] == 3 * 15 and pairs["start_lost"] == 9 and pairs["cds"] == 3 * 10 - 9
    pairs, _ = _known("-", (15, 35))      # the mirror: the intron on the 5' side of the CDS is the second one
    assert pairs["splice_utr"] == 12 and pairs["splice_donor"] == 6 and pairs["splice_acceptor"] == 6


def test_the_utr_of_a_minus_transcript_lies_at_or_above_thick_end():
    text = D.bed12("chr1", "t", "-", [(10, 20), (30, 40), (50, 60)], (15, 55)) + "\n"
    feats = _tables().read_transcript_structure(io.StringIO(text))[3]["chr1"]
    items = list(zip(feats["feat_b0"].tolist(), feats["feat_b1"].tolist(), feats["feat_kind"].tolist()))
    assert items == [(10, 15, 1), (15, 20, 5), (20, 30, 3), (30, 40, 5), (40, 50, 3), (50, 55, 5), (55, 60, 0)]


# ---- 3. the defining identity -----------------------------------------------------------------------------------------------------------------
def test_start_lost_plus_cds_is_the_consequence_table(record):
    from mural_amd.summaries import summary_conseq_host
    prob, start, strand, label = S.rows(record["seq"], seed=2, dtype=np.float32)
    table, _, _ = _twin(record["seq"], record["tx"], "chr1", prob, start, strand, label)
    conseq, _, _ = summary_conseq_host(record["seq"], prob, start, strand, label, record["tx"][2]["chr1"], len(record["names"]))
    assert conseq[:, :, 0].sum() > 1000
    assert np.array_equal(table[:, 7, 0] + table[:, 8, 0], conseq[:, :, 0].sum(axis=1))
    value = lambda cells: [sum((int(h) << 40) + int(l) for _, h, l in t) for t in cells.tolist()]      # noqa: E731
    assert value(table[:, 7:9]) == value(conseq)


# ---- 4. rows ------------------------------------------------------------------------------------------------------------------------------------
def test_the_table_is_the_same_for_any_split_of_the_rows(record):
    prob, start, strand, label = S.rows(record["seq"], seed=5, dtype=np.float32)
    n = len(start)
    whole = _twin(record["seq"], record["tx"], "chr1", prob, start, strand, label)
    rng = np.random.default_rng(5)
    cuts = np.sort(rng.choice(np.arange(1, n), size=9, replace=False))
    for parts in ([np.arange(i, min(i + 64, n)) for i in range(0, n, 64)], np.split(rng.permutation(n), cuts)):
        into = None
        for part in parts:
            table, counters, status = _twin(record["seq"], record["tx"], "chr1", prob[part], start[part], strand[part], label[part], into=into)
            into = (table, counters)
            assert status == 0
        assert into[0].tobytes() == whole[0].tobytes() and into[1].tobytes() == whole[1].tobytes()


def test_equal_starts_count_once_each(record):
    prob, start, strand, label = S.rows(record["seq"], seed=4, extra=0)
    twice = _twin(record["seq"], record["tx"], "chr1", np.repeat(prob, 2, 0), np.repeat(start, 2), np.repeat(strand, 2), np.repeat(label, 2))
    once = _twin(record["seq"], record["tx"], "chr1", prob, start, strand, label)
    assert np.array_equal(twice[1], 2 * once[1]) and np.array_equal(twice[0][:, :, 0], 2 * once[0][:, :, 0])
    assert S.as_integers(*twice[:2])[0] == [{b: [2 * v[0], 2 * v[1]] for b, v in cell.items()} for cell in S.as_integers(*once[:2])[0]]


@pytest.mark.parametrize("what,bit", [("start", 1), ("label", 2), ("nan", 8), ("above", 8), ("negative", 8)])
def test_each_status_bit_skips_its_row(record, what, bit):
    prob, start, strand, label = S.rows(record["seq"], seed=3)
    at = 1030                                                  # inside one_exon_p / one_exon_m
    want = _twin(record["seq"], record["tx"], "chr1", np.delete(prob, at, 0), np.delete(start, at), np.delete(strand, at), np.delete(label, at))
    if what == "start":
        start = start.copy()
        start[at] = -5
    elif what == "label":
        label[at] = 4
    else:
        prob[at, 2] = dict(nan=np.nan, above=1.5, negative=-0.25)[what]
    prob[at + 1, 0] = np.nan                                   # class 0's probability is never read
    got = _twin(record["seq"], record["tx"], "chr1", prob, start, strand, label)
    assert got[2] == bit and want[2] == 0
    assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1])


def test_four_classes_only(record):
    prob, start, strand, label = S.rows(record["seq"])
    with pytest.raises(ValueError, match="4 classes"):
        _twin(record["seq"], record["tx"], "chr1", prob, start, strand, label, n_class=2)


# ---- 5. the reader ------------------------------------------------------------------------------------------------------------------------------
def test_reader_layout_and_tiling(record):
    names, meta, segments, features = record["tx"]
    assert set(features) == {"chr1", "chr9"}
    feats, segs = features["chr1"], segments["chr1"]
    key = list(zip(feats["feat_b0"].tolist(), feats["feat_b1"].tolist(), feats["feat_tx"].tolist()))
    assert key == sorted(key)
    assert feats["feat_b0"].dtype == feats["feat_b1"].dtype == np.int64 and feats["feat_tx"].dtype == feats["feat_seg"].dtype == np.int32
    assert feats["feat_kind"].dtype == np.uint8 and feats["tx_strand"] is segs["tx_strand"] and feats["tx_cds_len"] is segs["tx_cds_len"]
    assert (feats["feat_b0"] < feats["feat_b1"]).all() and set(feats["feat_kind"].tolist()) == {0, 1, 2, 3, 4, 5}
    cds = feats["feat_kind"] == 5
    assert (feats["feat_seg"][~cds] == -1).all() and sorted(feats["feat_seg"][cds].tolist()) == list(range(len(segs["seg_b0"])))
    for key in ("b0", "b1", "tx"):
        assert np.array_equal(segs["seg_" + key][feats["feat_seg"][cds]], feats["feat_" + key][cds])
    spans = {f[0]: (f[3], f[4]) for f in S.parse(record["text"]) if f[1] == "chr1"}
    for t, name in enumerate(names):
        mine = np.nonzero(feats["feat_tx"] == t)[0]
        if name not in spans:
            assert len(mine) == 0
            continue
        at = spans[name][0]
        for f in mine:                                          # (sorted by feat_b0: the items follow each other without a hole)
            assert feats["feat_b0"][f] == at
            at = feats["feat_b1"][f]
        assert at == spans[name][1]


def test_reader_takes_gzip_handles_and_its_own_result_and_refuses_a_triple(record, tmp_path):
    T = _tables()
    gz = tmp_path / "tx.bed.gz"
    with gzip.open(gz, "wt") as fh:
        fh.write(record["text"])
    plain = T.read_transcripts(str(record["path"]))
    for source in (str(gz), io.StringIO(record["text"]), io.BytesIO(record["text"].encode()), open(record["path"])):
        names, meta, segments, features = T.read_transcript_structure(source)
        assert names == plain[0] == record["names"] and meta["chrom"] == plain[1]["chrom"]
        for key in ("strand", "cds_length", "n_segments", "aa"):
            assert np.array_equal(meta[key], plain[1][key]), key
        assert set(segments) == set(plain[2])
        for key, v in plain[2]["chr1"].items():
            assert np.array_equal(segments["chr1"][key], v) and segments["chr1"][key].dtype == v.dtype, key
        for key, v in record["tx"][3]["chr1"].items():
            assert np.array_equal(features["chr1"][key], v), key
    assert T.read_transcript_structure(record["tx"]) is record["tx"]
    with pytest.raises(ValueError, match="path"):
        T.read_transcript_structure(plain)
    with pytest.raises(ValueError, match=r"<transcripts>:2: .*overlap"):
        T.read_transcript_structure(io.StringIO("# header\n" + D.bed12("chr1", "a", "+", [(0, 9), (5, 12)]) + "\n"))


# ---- 6. the sink on host shards, the file, the build -------------------------------------------------------------------------------------------
def test_sink_on_host_shards_writes_the_table(record, tmp_path):
    from mural_amd.predict import SummarySink
    prob, start, strand, label = S.rows(record["seq"], seed=6, dtype=np.float32)
    want = _twin(record["seq"], record["tx"], "chr1", prob, start, strand, label)
    for labels, source in ((True, str(record["path"])), (False, record["tx"])):
        prefix = tmp_path / f"s{int(labels)}"
        sink = SummarySink(str(prefix), transcripts=source, genome=lambda name: record["seq"], transcript_structure=True,
                           annotations={"chr1": [(0, 500, "first")]}, transcript_labels=labels)
        for part in np.array_split(np.arange(len(start)), 3):
            sink({"chrom": "chr1", "start": start[part], "end": start[part] + 1, "strand": strand[part], "label": label[part].astype(np.float32),
                  "prob": prob[part], "n_class": 4, "calibrated": False, "aligned": True})
        sink.close()
        table, counters = sink.structure_sums()
        assert table.tobytes() == want[0].tobytes() and counters.tobytes() == want[1].tobytes()
        names, res_table, res_rows = sink.result()["transcript_structure"]
        assert names == record["names"] and res_table is table and res_rows is counters
        lines = (tmp_path / f"s{int(labels)}.consequence.structure.tsv").read_text().splitlines()
        header = lines[0].split("\t")
        assert header[:5] == ["name", "chrom", "strand", "n_rows", "n_nonmut"]
        assert header[5:] == [f"{kind}_{b}" for b in S.BINS + ("lof",) for kind in ("expected", "observed")]
        assert [ln.split("\t")[0] for ln in lines[1:]] == record["names"]
        conseq = sink.consequence_sums()[0]
        den = 1 << 71
        for name in ("known_m", "outer_plus", "short_introns_all_cds_p"):
            t = record["names"].index(name)
            row = lines[1 + t].split("\t")
            assert row[1:5] == ["chr1", "-" if name.endswith("_m") else "+", str(int(want[1][t, 0])), str(int(want[1][t, 1]))]
            cells = want[0][t].tolist()
            for b in range(9):
                assert float(row[5 + 2 * b]) == pytest.approx(((cells[b][1] << 40) + cells[b][2]) / den, rel=1e-5)
                assert row[6 + 2 * b] == (str(cells[b][0]) if labels else "NA")
            lof = [conseq[t, 2].tolist(), cells[3], cells[4], cells[7]]
            assert float(row[23]) == pytest.approx(sum((c[1] << 40) + c[2] for c in lof) / den, rel=1e-5) and float(row[23]) > 0
            assert row[24] == (str(sum(c[0] for c in lof)) if labels else "NA")
    assert os.path.exists(tmp_path / "s1.consequence.mut_rates.tsv")
    # without the flag nothing new is computed or written; the flag needs transcripts=, and a path rather than a read_transcripts triple
    plain = SummarySink(str(tmp_path / "p"), transcripts=record["tx"], genome=lambda name: record["seq"])
    plain({"chrom": "chr1", "start": start, "end": start + 1, "strand": strand, "label": label.astype(np.float32), "prob": prob, "n_class": 4,
           "calibrated": False, "aligned": True})
    plain.close()
    assert "transcript_structure" not in plain.result() and [f for f in sorted(os.listdir(tmp_path)) if f.startswith("p.c")] == ["p.consequence.mut_rates.tsv"]
    assert plain.consequence_sums()[0].tobytes() == conseq.tobytes()
    with pytest.raises(ValueError, match="transcripts"):
        SummarySink(None, transcript_structure=True)
    with pytest.raises(ValueError, match="path"):
        SummarySink(None, transcripts=_tables().read_transcripts(str(record["path"])), genome=lambda name: record["seq"], transcript_structure=True)
    sink = SummarySink(None, transcripts=str(record["path"]), genome=lambda name: record["seq"], transcript_structure=True)
    with pytest.raises(ValueError, match="4 classes"):
        sink({"chrom": "chr1", "start": start[:5], "end": start[:5] + 1, "strand": strand[:5], "label": np.zeros(5, np.float32),
              "prob": prob[:5, :2], "n_class": 2, "calibrated": False, "aligned": True})


def test_a_chromosome_without_cds_is_reduced(tmp_path):
    """Only a transcript without CDS on the chromosome: there are items, and no segments."""
    from mural_amd.predict import SummarySink
    text = D.bed12("chr2", "nc", "-", [(5, 12), (20, 30)], (5, 5)) + "\n" + D.bed12("chr1", "c", "+", [(0, 9)]) + "\n"
    tx = _tables().read_transcript_structure(io.StringIO(text))
    assert "chr2" in tx[3] and "chr2" not in tx[2]
    seq = "ACGT" * 10
    start = np.arange(40)
    prob, label = np.full((40, 4), 0.25), np.ones(40, np.int64)
    sink = SummarySink(None, transcripts=tx, genome=lambda name: seq, transcript_structure=True)
    sink({"chrom": "chr2", "start": start, "end": start + 1, "strand": np.zeros(40, np.uint8), "label": label, "prob": prob, "n_class": 4,
          "calibrated": False, "aligned": True})
    sink.close()
    table, rows = sink.structure_sums()
    assert rows.tolist() == [[25, 0], [0, 0]] and table[0, :, 0].tolist() == [0, 0, 17, 0, 0, 4, 4, 0, 0]


def test_the_reduce_kernel_uses_no_scratch():
    report = os.path.join(ROOT, "mural_amd", "csrc", "summary_txstruct.resources.txt")
    assert os.path.exists(report), "the build keeps the compiler's resource report of summary_txstruct.hip"
    text = open(report).read()
    blocks = text.split("Function Name: ")[1:]
    reduce = [b for b in blocks if "summary_txstruct_reduce_kernel" in b.splitlines()[0]]
    assert len(reduce) == 2                                     # float and double rows
    for b in blocks:
        assert "ScratchSize [bytes/lane]: 0" in b, b.splitlines()[0]
