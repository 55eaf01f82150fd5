"""Shared data of the INDEL structure simulation tests: the toy three-exon transcript, a random structure of overlapping transcripts,
rows with strands, and a second brute-force oracle of the INDEL structure table, built anew here: it paints every base of every
transcript with a small integer code from the raw BED12 fields and decides an event from the painted bases alone -- no items, no links,
no ``tables.read_transcript_structure`` and none of the code of tests/_txindel_data.py."""
import io

import numpy as np

from tests import _conseq_data as D

KEY, SEED = 0x1DE1C0DE, (5 << 34) + 11
BINS = 10
# class lengths: framed, mixed (4-6, 7-20, 2-3) and always-shifting (1-2, 4-5) ranges
LENGTHS = {2: "3", 5: "1-2,3,4-5,4-6", 8: None}
TOY = "chr1\t10\t60\ttoy_%s\t0\t%s\t15\t55\t0\t3\t10,10,10,\t0,20,40,\n"      # blocks [10,20) [30,40) [50,60), thick [15,55)


def toy_text():
    return TOY % ("p", "+") + TOY % ("m", "-")


def random_text(seed=0, n_tx=20, span=(40, 900)):
    """About `n_tx` transcripts with overlapping spans on chr1: 1 .. 6 exons of 1 .. 40 bases, gaps of 0 .. 30 bases (abutting blocks and
    gaps below 4 among them), both strands, every third without CDS, one CDS of two bases."""
    rng = np.random.default_rng(seed + 77)
    lines = []
    for t in range(n_tx):
        at = int(rng.integers(span[0], span[1] - 300))
        blocks = []
        for _ in range(int(rng.integers(1, 7))):
            size = int(rng.integers(1, 41))
            blocks.append((at, at + size))
            at += size + int(rng.choice([0, 1, 3, 4, 5, int(rng.integers(6, 31))]))
        lo, hi = blocks[0][0], blocks[-1][1]
        if t % 3 == 2:
            thick = (lo, lo)
        elif t == 4:
            thick = (blocks[0][0], min(blocks[0][0] + 2, blocks[0][1]))
        else:
            a, b = sorted(int(v) for v in rng.integers(lo, hi + 1, size=2))
            thick = (a, max(b, a))
        lines.append(D.bed12("chr1", f"r{t}", "+-"[t & 1], blocks, thick))
    return "\n".join(lines) + "\n"


def read(text):
    from mural_amd import tables
    names, meta, segments, features = tables.read_transcript_structure(io.StringIO(text))
    return names, segments.get("chr1"), features["chr1"]


def rows(length, n_class, seed=0, dtype=np.float64, extra=150):
    """(prob [n][n_class], start ascending with equal starts, strand uint8, label int64): a row at every base of [0, length) and `extra`
    more at random positions."""
    rng = np.random.default_rng(seed + 900)
    start = np.sort(np.concatenate([np.arange(length), rng.integers(0, length, size=extra)])).astype(np.int64)
    n = len(start)
    prob = rng.dirichlet(np.ones(n_class), size=n).astype(dtype)
    prob[rng.integers(0, n, size=4), rng.integers(1, n_class, size=4)] = [0.0, 1.0, 2.0 ** -40, 0.5]
    return prob, start, rng.integers(0, 2, size=n).astype(np.uint8), rng.integers(0, n_class, size=n).astype(np.int64)


# ---- the oracle: codes per base -------------------------------------------------------------------------------------------------------
UTR5, UTR3, NONCODING, GAP_SITE, GAP_SITE_UTR, GAP = 0, 1, 2, 3, 4, 5      # (the bins of the same numbers); CDS bases: 100 + offset


def _fields(text):
    for line in text.splitlines():
        f = line.split("\t")
        if len(f) >= 12 and not line.startswith(("#", "track")):
            s = int(f[1])
            blocks = [(s + int(o), s + int(o) + int(z)) for z, o in zip(f[10].strip(",").split(","), f[11].strip(",").split(","))]
            yield f[0], f[5] == "-", s, int(f[2]), int(f[6]), int(f[7]), blocks


def _paint(minus, s, e, t0, t1, blocks):
    """(code per base of [s, e), the gap (first base, end, coding) per base or None, CDS length)."""
    code, gap = [GAP] * (e - s), [None] * (e - s)
    exon = [False] * (e - s)
    for a, b in blocks:
        for p in range(a, b):
            exon[p - s] = True
    cds = [p for p in range(s, e) if exon[p - s] and t0 <= p < t1]
    for x, p in enumerate(reversed(cds) if minus else cds):
        code[p - s] = 100 + x
    for p in range(s, e):
        if exon[p - s] and not t0 <= p < t1:
            code[p - s] = NONCODING if t0 >= t1 else (UTR5 if (p < t0) != minus else UTR3)
    p = s
    while p < e:
        if exon[p - s]:
            p += 1
            continue
        q = p
        while q < e and not exon[q - s]:
            q += 1
        coding = bool(cds) and cds[0] < p and cds[-1] >= q
        for g in range(p, q):
            gap[g - s] = (p, q, coding)
            if q - p >= 4 and (g < p + 2 or g >= q - 2):
                code[g - s] = GAP_SITE if coding else GAP_SITE_UTR
        p = q
    return code, gap, len(cds)


def _frame(lo, hi, n):
    if lo == hi:
        return 7 if n % 3 else 8
    return 9 if hi // 3 > (lo - 1) // 3 else 7


def _event(code, gap, cds_len, minus, s, e, kind, j, lo, hi, chrom_len):
    """The bin of an event at boundary j, or None where the transcript does not count it."""
    h = j if kind == 1 else j - 1
    if not s <= h < e or (kind == 0 and j >= e):
        return None
    if kind == 0:
        left, right = code[j - 1 - s], code[j - s]
        if left >= 100 or right >= 100:
            x = sum(1 for p in range(s, e) if code[p - s] >= 100 and ((p >= j) if minus else (p < j)))
            return 0 if x == 0 else 1 if x == cds_len else 6 if x <= 2 else _frame(lo, hi, lo)
        if gap[j - 1 - s] and gap[j - s]:      # (one gap: two gaps never abut)
            a, b, coding = gap[j - s]
            return (GAP_SITE if coding else GAP_SITE_UTR) if b - a >= 4 and j in (a + 1, b - 1) else GAP      # a dinucleotide is split
        return right if gap[j - 1 - s] else left
    deleted = {p for p in (range(j, j + lo) if kind == 1 else range(j - lo, j)) if s <= p < e and p >= 0 and (chrom_len is None or p < chrom_len)}
    got = [code[p - s] for p in deleted | {h}]
    n_cds = sum(1 for c in got if c >= 100)
    for test, where in ((lambda c: 100 <= c < 103, 6), (lambda c: c == GAP_SITE, 3)):
        if any(test(c) for c in got):
            return where
    if n_cds:
        return _frame(lo, hi, n_cds)
    for c in (GAP_SITE_UTR, NONCODING, UTR5, UTR3):
        if c in got:
            return c
    return GAP


def oracle(text, prob, start, label, n_class, kind, offset, class_len, chrom_len=None):
    """(table [transcripts][10][3] of Python integers: label count, hi, lo with lo < 2^40; rows [transcripts][2]) by brute force."""
    from mural_amd.summaries import kmer_quantise
    hi, lo, bad = kmer_quantise(np.asarray(prob)[:, 1:n_class])
    assert not bad.any()
    whole = [[(int(h) << 40) + int(v) for h, v in zip(hr, lr)] for hr, lr in zip(hi.tolist(), lo.tolist())]
    labels = np.asarray(label).tolist()
    at = {}
    for i, st in enumerate(np.asarray(start).tolist()):
        at.setdefault(st + offset, []).append(i)
    table, counters = [], []
    for chrom, minus, s, e, t0, t1, blocks in _fields(text):
        cells, counter = [[0, 0] for _ in range(BINS)], [0, 0]
        if chrom == "chr1":
            code, gap, cds_len = _paint(minus, s, e, t0, t1, blocks)
            for j in range(s, e + 1):
                for i in at.get(j, ()):
                    bins = [_event(code, gap, cds_len, minus, s, e, kind, j, *class_len[c - 1], chrom_len) for c in range(1, n_class)]
                    if bins[0] is None:
                        continue
                    counter[0] += 1
                    counter[1] += labels[i] == 0
                    for c, b in enumerate(bins, 1):
                        cells[b][0] += labels[i] == c
                        cells[b][1] += whole[i][c - 1]
        table.append([[n, v >> 40, v & ((1 << 40) - 1)] for n, v in cells])
        counters.append(counter)
    return table, counters
