"""Shared data of the structure-table tests: the record and rows of tests/_conseq_data.py (random transcripts on both strands, nested
and overlapping isoforms, a transcript without CDS, touching blocks, 1-bp exons) with more transcripts laid over the same bases -- a
single-exon transcript with both UTRs in one block on each strand, introns of length 0 .. 5 between exons of 1 .. 4 bases, thickStart and
thickEnd on block boundaries and inside an intron --, and the brute-force oracle: Python integers and strings that mark every base of
every transcript with its bin from the raw BED12 fields, independent of ``tables.read_transcript_structure``."""
import numpy as np

from tests import _conseq_data as D

BINS = ("utr5", "utr3", "noncoding_exon", "splice_donor", "splice_acceptor", "splice_utr", "intron", "start_lost", "cds")


def build(seed=0):
    """(sequence, BED12 text, names): the record of ``_conseq_data.build`` and the structure transcripts over it."""
    seq, text, names = D.build(seed)
    assert len(seq) > 3000
    lines = []
    for strand in "+-":
        tag = "p" if strand == "+" else "m"
        lines.append(D.bed12("chr1", f"one_exon_{tag}", strand, [(1000, 1100)], (1020, 1081)))
        # exons of 1 .. 4 bases, introns of 0, 1, 2, 3, 4 and 5 bases (abutting blocks give no gap)
        blocks, at = [], 1200
        for j, gap in enumerate((0, 1, 2, 3, 4, 5, 4, 0, 5)):
            size = 1 + (j + len(tag)) % 4
            blocks.append((at, at + size))
            at += size + gap
        blocks.append((at, at + 6))
        lines.append(D.bed12("chr1", f"short_introns_{tag}", strand, blocks, (blocks[1][0], blocks[-1][1] - 2)))
        lines.append(D.bed12("chr1", f"short_introns_all_cds_{tag}", strand, blocks))
        b3 = [(1400, 1410), (1420, 1430), (1440, 1450)]
        lines.append(D.bed12("chr1", f"thick_at_block_start_{tag}", strand, b3, (1420, 1445)))      # the first intron has no CDS 5' of it
        lines.append(D.bed12("chr1", f"thick_at_block_end_{tag}", strand, b3, (1410, 1430)))        # thickStart on the intron's first base
        lines.append(D.bed12("chr1", f"thick_in_intron_{tag}", strand, b3, (1405, 1435)))           # thickEnd inside the second intron
        lines.append(D.bed12("chr1", f"known_{tag}", strand, [(1510, 1520), (1530, 1540), (1550, 1560)], (1515, 1555)))
        lines.append(D.bed12("chr1", f"short_cds_{tag}", strand, [(1600, 1610), (1620, 1630)], (1608, 1610)))      # cds_length 2
    # blocks that reach neither end of the span: the rest of the span is a gap at each end
    lines.append("chr1\t1700\t1760\tgaps_at_the_ends\t0\t-\t1710\t1735\t0\t2\t10,10,\t5,30,")
    text += "\n".join(lines) + "\n"
    names = names + [ln.split("\t")[3] for ln in lines]
    return seq, text, names


rows = D.rows


def parse(text):
    """[(name, chrom, strand, start, end, thickStart, thickEnd, [(b0, b1)] blocks)] of a BED12 text: the oracle's own reading."""
    out = []
    for line in text.splitlines():
        if not line.startswith("chr"):
            continue
        f = line.split("\t")
        start = int(f[1])
        blocks = [(start + int(off), start + int(off) + int(size)) for size, off in zip(f[10].strip(",").split(","), f[11].strip(",").split(","))]
        out.append((f[3], f[0], f[5], start, int(f[2]), int(f[6]), int(f[7]), blocks))
    return out


def base_bins(seq, tx_strand, start, end, t0, t1, blocks):
    """{position: bin name, or ("cds", x, codon string)} of every base of [start, end) of one transcript."""
    in_block = {p for a, b in blocks for p in range(a, b)}
    coding = sorted(p for p in in_block if t0 <= p < t1)
    order = coding[::-1] if tx_strand == "-" else coding
    cds = "".join((seq[p] if p < len(seq) else "?") for p in order)
    if tx_strand == "-":
        cds = "".join(D.COMP.get(ch, ch) for ch in cds)
    where = {}
    for x, p in enumerate(order):
        where[p] = ("cds", x, cds[x - x % 3:x - x % 3 + 3])
    for p in in_block - set(coding):
        if t0 == t1:
            where[p] = "noncoding_exon"
        else:
            five = (p < t0) == (tx_strand == "+")
            where[p] = "utr5" if five else "utr3"
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
            site = None
            if b - a >= 4 and (g < a + 2 or g >= b - 2):
                five_end = (g < a + 2) == (tx_strand == "+")
                site = ("splice_donor" if five_end else "splice_acceptor") if is_coding else "splice_utr"
            where[g] = site or "intron"
        p = b
    return where


def oracle(seq, text, prob, start, strand, label, chrom="chr1", code=D.CODE, alt=D.ALT):
    """[{bin: [label count, sum in units of 2^-71]}, ...] and [[rows, rows of label 0]] per transcript of `text`, as Python integers."""
    from mural_amd.summaries import kmer_quantise
    hi, lo, bad = kmer_quantise(np.asarray(prob)[:, 1:4])
    assert not bad.any()
    q = [[(h << 40) + l for h, l in zip(hr, lr)] for hr, lr in zip(hi.tolist(), lo.tolist())]
    aa = {a + b + c: code[16 * i + 4 * j + k] for i, a in enumerate("ACGT") for j, b in enumerate("ACGT") for k, c in enumerate("ACGT")}
    starts, labels = np.asarray(start).tolist(), np.asarray(label).tolist()
    strands = [0] * len(starts) if strand is None else np.asarray(strand).tolist()
    by_pos = {}
    for i, s in enumerate(starts):
        by_pos.setdefault(s, []).append(i)
    cells, counters = [], []
    for name, tx_chrom, tx_strand, t_start, t_end, t0, t1, blocks in parse(text):
        cell, counter = {b: [0, 0] for b in BINS}, [0, 0]
        cells.append(cell)
        counters.append(counter)
        if tx_chrom != chrom:
            continue
        for p, what in base_bins(seq, tx_strand, t_start, t_end, t0, t1, blocks).items():
            for i in by_pos.get(p, ()):
                counter[0] += 1
                counter[1] += labels[i] == 0
                for c in (1, 2, 3):
                    where = what
                    if isinstance(what, tuple):
                        _, x, codon = what
                        where = "cds"
                        if x < 3 and len(codon) == 3 and all(ch in "ACGT" for ch in codon):
                            own = D.COMP[seq[p]] if strands[i] else seq[p]
                            new = alt[own][c - 1]
                            new = D.COMP[new] if strands[i] else new          # on the reference strand
                            new = D.COMP[new] if tx_strand == "-" else new    # on the transcript's strand
                            if aa[codon[:x] + new + codon[x + 1:]] != aa[codon]:
                                where = "start_lost"
                    cell[where][0] += labels[i] == c
                    cell[where][1] += q[i][c - 1]
    return cells, counters


def as_integers(table, counters):
    """The oracle's two lists from integer tables [transcripts][9][3] and [transcripts][2], and a check of lo < 2^40."""
    t = np.asarray(table).astype(np.uint64)
    assert t.shape[1:] == (9, 3) and (t[:, :, 2] < np.uint64(1 << 40)).all()
    cells = [{b: [int(g[j][0]), (int(g[j][1]) << 40) + int(g[j][2])] for j, b in enumerate(BINS)} for g in t.tolist()]
    return cells, [[int(a), int(b)] for a, b in np.asarray(counters).tolist()]
