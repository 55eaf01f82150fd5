"""Shared data of the INDEL-structure tests: the record of tests/_txstruct_data.py (both strands, 1-bp exons, abutting blocks, gaps
shorter than 4, a transcript without CDS, a CDS of 2 bases, nested and overlapping isoforms, a transcript that runs past the record),
INDEL rows over it, and the brute-force oracle: Python integers that mark every base of every transcript from the raw BED12 fields,
independent of ``tables.read_transcript_structure`` and of the items' links."""
import numpy as np

from tests import _txstruct_data as S

BINS = ("utr5", "utr3", "noncoding_exon", "splice", "splice_utr", "intron", "start_lost", "frameshift", "inframe", "cds_mixed")
KNOWN = "chr1\t10\t60\tknown\t0\t%s\t15\t55\t0\t3\t10,10,10,\t0,20,40,\n"      # blocks [10,20) [30,40) [50,60), thick [15,55)

build = S.build


def rows(seq, n_class, seed=0, dtype=np.float64, extra=200):
    """(prob [n][n_class], start ascending with equal starts, label int64): a row at every base of the record, at -1 and `extra` more at
    random positions; exact edge probabilities among them."""
    rng = np.random.default_rng(seed + 300)
    start = np.sort(np.concatenate([np.arange(-1, len(seq)), rng.integers(0, len(seq), size=extra)])).astype(np.int64)
    start[0] = 0      # (a negative start is a bad row: the tests of the status bits set one)
    n = len(start)
    prob = rng.dirichlet(np.ones(n_class), size=n).astype(dtype)
    prob[rng.integers(0, n, size=6), rng.integers(1, n_class, size=6)] = [0.0, 1.0, 2.0 ** -60, 1e-30, 0.5, 1.0 - 2.0 ** -24]
    label = rng.integers(0, n_class, size=n).astype(np.int64)
    return prob, start, label


def frame_bin(lo, hi, n):
    if lo == hi:
        return "frameshift" if n % 3 else "inframe"
    lengths = range(lo, hi + 1)
    return "cds_mixed" if any(v % 3 == 0 for v in lengths) and any(v % 3 for v in lengths) else "frameshift"


def base_marks(tx_strand, start, end, t0, t1, blocks):
    """({position: mark}, cds_length) of every base of [start, end): ("cds", offset), "utr5", "utr3", "noncoding_exon" or ("gap", a, b,
    coding)."""
    in_block = {p for a, b in blocks for p in range(a, b)}
    coding = sorted(p for p in in_block if t0 <= p < t1)
    order = coding[::-1] if tx_strand == "-" else coding
    where = {p: ("cds", x) for x, p in enumerate(order)}
    for p in in_block - set(coding):
        where[p] = "noncoding_exon" if t0 == t1 else ("utr5" if (p < t0) == (tx_strand == "+") else "utr3")
    p = start
    while p < end:
        if p in in_block:
            p += 1
            continue
        a = b = p
        while b < end and b not in in_block:
            b += 1
        is_coding = any(c < a for c in coding) and any(c >= b for c in coding)
        for g in range(a, b):
            where[g] = ("gap", a, b, is_coding)
        p = b
    return where, len(coding)


def event_bin(marks, cds_len, tx_strand, span, kind, j, lo, hi, chrom_len=None):
    """The bin of one event of class lengths lo .. hi at boundary j, or None where the transcript does not count it."""
    s, e = span
    h = j if kind == 1 else j - 1
    if not s <= h < e or (kind == 0 and not j < e):
        return None
    is_cds = lambda m: isinstance(m, tuple) and m[0] == "cds"      # noqa: E731
    is_gap = lambda m: isinstance(m, tuple) and m[0] == "gap"      # noqa: E731
    if kind == 0:
        m1, m2 = marks[j - 1], marks[j]
        if is_cds(m1) or is_cds(m2):
            x = sum(1 for p, m in marks.items() if is_cds(m) and ((p >= j) if tx_strand == "-" else (p < j)))
            return "utr5" if x == 0 else "utr3" if x == cds_len else "start_lost" if x <= 2 else frame_bin(lo, hi, lo)
        if is_gap(m1) and is_gap(m2):
            assert m1 == m2
            _, a, b, coding = m1
            if b - a >= 4 and j in (a + 1, b - 1):
                return "splice" if coding else "splice_utr"
            return "intron"
        if is_gap(m1):
            return m2
        assert is_gap(m2) or m1 == m2
        return m1
    d = range(j, j + lo) if kind == 1 else range(j - lo, j)
    d = {p for p in d if s <= p < e and p >= 0 and (chrom_len is None or p < chrom_len)} | {h}
    got = [marks[p] for p in sorted(d)]
    n_cds = sum(1 for m in got if is_cds(m))
    site = lambda p, m: m[2] - m[1] >= 4 and (p < m[1] + 2 or p >= m[2] - 2)      # noqa: E731
    if any(is_cds(m) and m[1] < 3 for m in got):
        return "start_lost"
    if any(is_gap(marks[p]) and marks[p][3] and site(p, marks[p]) for p in d):
        return "splice"
    if n_cds:
        return frame_bin(lo, hi, n_cds)
    if any(is_gap(marks[p]) and not marks[p][3] and site(p, marks[p]) for p in d):
        return "splice_utr"
    for what in ("noncoding_exon", "utr5", "utr3"):
        if what in got:
            return what
    return "intron"


def oracle(text, prob, start, label, n_class, kind, offset, class_len, chrom_len=None, chrom="chr1"):
    """[{bin: [label count, sum in units of 2^-71]}, ...] and [[rows, rows of label 0]] per transcript of `text`, as Python integers.
    class_len: [(lo, hi)] of the classes 1 .. n_class - 1."""
    from mural_amd.summaries import kmer_quantise
    hi, lo, bad = kmer_quantise(np.asarray(prob)[:, 1:n_class])
    assert not bad.any()
    q = [[(h << 40) + l for h, l in zip(hr, lr)] for hr, lr in zip(hi.tolist(), lo.tolist())]
    starts, labels = np.asarray(start).tolist(), np.asarray(label).tolist()
    by_j = {}
    for i, st in enumerate(starts):
        by_j.setdefault(st + offset, []).append(i)
    cells, counters = [], []
    for name, tx_chrom, tx_strand, t_start, t_end, t0, t1, blocks in S.parse(text):
        cell, counter = {b: [0, 0] for b in BINS}, [0, 0]
        cells.append(cell)
        counters.append(counter)
        if tx_chrom != chrom:
            continue
        marks, cds_len = base_marks(tx_strand, t_start, t_end, t0, t1, blocks)
        for j in range(t_start, t_end + 1):
            for c in range(1, n_class):
                where = event_bin(marks, cds_len, tx_strand, (t_start, t_end), kind, j, *class_len[c - 1], chrom_len)
                if where is None:
                    break
                for i in by_j.get(j, ()):
                    if c == 1:
                        counter[0] += 1
                        counter[1] += labels[i] == 0
                    cell[where][0] += labels[i] == c
                    cell[where][1] += q[i][c - 1]
    return cells, counters


def as_integers(table, counters):
    """The oracle's two lists from integer tables [transcripts][10][3] and [transcripts][2], and a check of lo < 2^40."""
    t = np.asarray(table).astype(np.uint64)
    assert t.shape[1:] == (10, 3) and (t[:, :, 2] < np.uint64(1 << 40)).all()
    cells = [{b: [int(g[j][0]), (int(g[j][1]) << 40) + int(g[j][2])] for j, b in enumerate(BINS)} for g in t.tolist()]
    return cells, [[int(a), int(b)] for a, b in np.asarray(counters).tolist()]


# class lengths of the tests: framed, mixed (4-6, 7-20, 2-3) and always-shifting (1-2, 4-5) ranges
LENGTHS = {2: "3", 5: "1,2,3,4-6", 8: None, 16: "1,2,3,4,5,6,7-20,1-2,4-5,2-3,9,10,11,12,64"}


def pairs(spec, n_class):
    from mural_amd import tables
    return [tuple(r) for r in tables.check_indel_lengths(spec, n_class)[1:].tolist()]
