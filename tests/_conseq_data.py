"""Shared data of the consequence-summary tests: a record of a few thousand bases with a BED12 transcript file over it (the 64 codons in
index order on '+', the same CDS on '-' and cut into blocks of 1, 1, 2, 3, ... bases, nested and overlapping transcripts on both strands,
CDS lengths that are no multiple of 3, masked bases, a CDS that runs past the record, a transcript without CDS, and a few dozen random
ones), rows over it, and the brute-force oracle -- Python integers and strings: each transcript's CDS string, reverse-complemented for
'-', one loop over codons and alternatives -- that the numpy twin ``summary_conseq_host`` is checked against."""
import numpy as np

CODE = "KNKNTTTTRSRSIIMIQHQHPPPPRRRRLLLLEDEDAAAAGGGGVVVV*Y*YSSSS*CWCLFLF"
ALT = {"A": "CGT", "C": "AGT", "G": "ACT", "T": "ACG"}
COMP = {"A": "T", "C": "G", "G": "C", "T": "A"}
BINS = ("syn", "mis", "stop_gained", "stop_lost", "unresolved")
ALL_CODONS = "".join(a + b + c for a in "ACGT" for b in "ACGT" for c in "ACGT")      # 192 bases: codon k at [3 k, 3 k + 3)


def revcomp(s):
    return "".join(COMP.get(ch, "N") for ch in reversed(s))


def bed12(chrom, name, strand, blocks, thick=None):
    """One BED12 line of blocks [(b0, b1)] (ascending); thick: (thickStart, thickEnd), default the whole transcript."""
    start, end = blocks[0][0], blocks[-1][1]
    t0, t1 = (start, end) if thick is None else thick
    return "\t".join([chrom, str(start), str(end), name, "0", strand, str(t0), str(t1), "0", str(len(blocks)),
                      ",".join(str(b - a) for a, b in blocks) + ",", ",".join(str(a - start) for a, _ in blocks) + ","])


def _cut(cds, sizes, rng, at):
    """The CDS cut into exons of `sizes` (the last takes the rest) with random introns between them, placed at `at`:
    (sequence, blocks)."""
    seq, blocks, done = "", [], 0
    for j in range(len(sizes) + 1):
        size = sizes[j] if j < len(sizes) else len(cds) - done
        if size <= 0:
            break
        size = min(size, len(cds) - done)
        blocks.append((at + len(seq), at + len(seq) + size))
        seq += cds[done:done + size]
        done += size
        if done < len(cds):
            seq += "".join(rng.choice(list("ACGT"), size=int(rng.integers(1, 6))))
    return seq, blocks


def build(seed=0, n_random=30):
    """(sequence, BED12 text, names): one record `chr1` and its transcripts (+ one transcript on `chr9`, which never arrives)."""
    rng = np.random.default_rng(seed)
    seq, lines = "", []

    def pad(n=7):
        nonlocal seq
        seq += "".join(rng.choice(list("ACGT"), size=n))

    lines += ["# transcripts of the consequence tests", "track name=tx"]
    lines.append(bed12("chr1", "codons_plus", "+", [(0, 192)]))
    seq += ALL_CODONS
    pad()
    at = len(seq)
    lines.append(bed12("chr1", "codons_minus", "-", [(at, at + 192)]))
    seq += revcomp(ALL_CODONS)
    pad()
    sizes = [1, 1, 2, 3, 1, 1, 1, 4, 2, 1, 5, 1, 1, 2, 7, 1, 1, 1, 1, 3, 2, 2, 1, 1, 9, 1, 40]
    piece, blocks = _cut(ALL_CODONS, sizes, rng, len(seq))
    lines.append(bed12("chr1", "codons_cut_plus", "+", blocks))
    seq += piece
    pad()
    piece, blocks = _cut(revcomp(ALL_CODONS), sizes[::-1], rng, len(seq))
    lines.append(bed12("chr1", "codons_cut_minus", "-", blocks))
    seq += piece
    pad()
    for nm, codon in (("atg", "ATG"), ("tgg", "TGG"), ("taa", "TAA"), ("aaa", "AAA")):
        at = len(seq)
        lines.append(bed12("chr1", nm, "+", [(at, at + 3)]))
        seq += codon
        pad(2)
    # a region of nested and overlapping transcripts on both strands, with UTRs, CDS lengths 3 k + 1 and 3 k + 2, masked bases
    at = len(seq)
    region = list(rng.choice(list("ACGT"), size=400))
    region[57], region[120], region[121], region[300] = "N", "R", "N", "Y"
    seq += "".join(region)
    lines.append(bed12("chr1", "outer_plus", "+", [(at + 10, at + 90), (at + 110, at + 200), (at + 250, at + 390)], (at + 20, at + 382)))      # 3 k + 1
    lines.append(bed12("chr1", "inner_minus", "-", [(at + 40, at + 70), (at + 115, at + 160)], (at + 42, at + 158)))                          # 3 k + 2
    lines.append(bed12("chr1", "overlap_minus", "-", [(at + 5, at + 60), (at + 180, at + 260), (at + 290, at + 330)]))
    lines.append(bed12("chr1", "same_blocks_plus", "+", [(at + 5, at + 60), (at + 180, at + 260), (at + 290, at + 330)]))
    lines.append(bed12("chr1", "noncoding", "+", [(at + 30, at + 80), (at + 100, at + 140)], (at + 30, at + 30)))
    lines.append(bed12("chr1", "utr_only_block", "+", [(at + 0, at + 8), (at + 12, at + 30), (at + 340, at + 360)], (at + 14, at + 29)))
    lines.append(bed12("chr9", "elsewhere", "+", [(0, 30)]))
    for j in range(n_random):
        at = len(seq)
        n_blocks = int(rng.integers(3, 16))
        blocks, pos = [], at
        for _ in range(n_blocks):
            pos += int(rng.integers(0, 9))            # touching blocks are legal
            size = int(rng.integers(1, 31))
            blocks.append((pos, pos + size))
            pos += size
        seq += "".join(rng.choice(list("ACGT"), size=pos - at))
        strand = "+-"[j & 1]
        thick = None
        if j % 3 and blocks[-1][1] - blocks[0][0] > 12:
            thick = (blocks[0][0] + int(rng.integers(0, 5)), blocks[-1][1] - int(rng.integers(0, 5)))
        lines.append(bed12("chr1", f"random{j}", strand, blocks, thick))
        if j % 4 == 0:                                # an isoform: some blocks dropped, the other strand
            keep = [b for i, b in enumerate(blocks) if i % 3 != 1]
            lines.append(bed12("chr1", f"random{j}_iso", "+-"[1 - (j & 1)], keep))
        seq = seq[:len(seq) - int(rng.integers(0, 4))]      # the next transcript may overlap this one's tail
    # the last transcript's CDS runs two bases past the record: its last codon has a position outside the record
    at = len(seq)
    seq += "".join(rng.choice(list("ACGT"), size=10))
    lines.append(bed12("chr1", "past_the_end", "+", [(at, at + 12)]))
    names = [ln.split("\t")[3] for ln in lines if ln.startswith("chr")]
    return seq, "\n".join(lines) + "\n", names


def rows(seq, seed=0, dtype=np.float64, extra=200):
    """(prob [n][4], start ascending with equal starts, strand uint8, label int64): a row at every base of the record and `extra` more
    at random positions, on random strands; exact edge probabilities among them."""
    rng = np.random.default_rng(seed + 100)
    start = np.sort(np.concatenate([np.arange(len(seq)), rng.integers(0, len(seq), size=extra)])).astype(np.int64)
    n = len(start)
    prob = rng.dirichlet(np.ones(4), size=n).astype(dtype)
    prob[rng.integers(0, n, size=6), rng.integers(1, 4, size=6)] = [0.0, 1.0, 2.0 ** -60, 1e-30, 0.5, 1.0 - 2.0 ** -24]
    strand = rng.integers(0, 2, size=n).astype(np.uint8)
    label = rng.integers(0, 4, size=n).astype(np.int64)
    return prob, start, strand, label


def parse(text):
    """[(name, chrom, strand, [(b0, b1)] CDS segments ascending)] of a BED12 text: the oracle's own reading of the file."""
    out = []
    for line in text.splitlines():
        if not line.startswith("chr"):
            continue
        f = line.split("\t")
        start, t0, t1 = int(f[1]), int(f[6]), int(f[7])
        segs = []
        for size, off in zip(f[10].strip(",").split(","), f[11].strip(",").split(",")):
            a, b = max(start + int(off), t0), min(start + int(off) + int(size), t1)
            if a < b:
                segs.append((a, b))
        out.append((f[3], f[0], f[5], segs))
    return out


def oracle(seq, text, prob, start, strand, label, chrom="chr1", code=CODE, alt=ALT):
    """[{bin: [label count, sum in units of 2^-71]}, ...] and [[rows, rows of label 0]] per transcript of `text`, as Python integers."""
    from mural_amd.summaries import kmer_quantise
    hi, lo, bad = kmer_quantise(np.asarray(prob)[:, 1:4])
    assert not bad.any()
    q = [[(h << 40) + l for h, l in zip(hr, lr)] for hr, lr in zip(hi.tolist(), lo.tolist())]
    aa = {a + b + c: code[16 * i + 4 * j + k] for i, a in enumerate("ACGT") for j, b in enumerate("ACGT") for k, c in enumerate("ACGT")}
    starts, strands, labels = np.asarray(start).tolist(), np.asarray(strand).tolist(), np.asarray(label).tolist()
    by_pos = {}
    for i, s in enumerate(starts):
        by_pos.setdefault(s, []).append(i)
    cells, counters = [], []
    for name, tx_chrom, tx_strand, segs in parse(text):
        cell, counter = {b: [0, 0] for b in BINS}, [0, 0]
        cells.append(cell)
        counters.append(counter)
        if tx_chrom != chrom:
            continue
        positions = [p for a, b in segs for p in range(a, b)]
        if tx_strand == "-":
            positions.reverse()
        cds = "".join((seq[p] if p < len(seq) else "?") for p in positions)
        if tx_strand == "-":
            cds = "".join(COMP.get(ch, ch) for ch in cds)
        for x, p in enumerate(positions):
            for i in by_pos.get(p, ()):
                counter[0] += 1
                counter[1] += labels[i] == 0
                codon = cds[x - x % 3:x - x % 3 + 3]
                resolved = len(codon) == 3 and all(ch in "ACGT" for ch in codon)
                if resolved:
                    own = COMP[seq[p]] if strands[i] else seq[p]
                for c in (1, 2, 3):
                    where = "unresolved"
                    if resolved:
                        new = alt[own][c - 1]
                        new = COMP[new] if strands[i] else new          # on the reference strand
                        new = COMP[new] if tx_strand == "-" else new    # on the transcript's strand
                        k = x % 3
                        assert new != codon[k]
                        ref_aa, alt_aa = aa[codon], aa[codon[:k] + new + codon[k + 1:]]
                        where = "syn" if ref_aa == alt_aa else "stop_gained" if alt_aa == "*" else "stop_lost" if ref_aa == "*" else "mis"
                    cell[where][0] += labels[i] == c
                    cell[where][1] += q[i][c - 1]
    return cells, counters


def as_integers(table, counters):
    """The oracle's two lists from integer tables [transcripts][5][3] and [transcripts][2], and a check of lo < 2^40."""
    t = np.asarray(table).astype(np.uint64)
    assert (t[:, :, 2] < np.uint64(1 << 40)).all()
    cells = [{b: [int(g[j][0]), (int(g[j][1]) << 40) + int(g[j][2])] for j, b in enumerate(BINS)} for g in t.tolist()]
    return cells, [[int(a), int(b)] for a, b in np.asarray(counters).tolist()]
