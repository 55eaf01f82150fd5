"""Shared data of the annotation-summary tests: a literal annotation BED, rows on two chromosomes and the brute-force oracle (Python
integers, one membership test per name, interval and row) that the numpy twin ``summary_annot_host`` is checked against."""
import numpy as np

# 12 names on chrA (rows start in 100 .. 899, none in 500 .. 509), two of them also on chrB, one on a chromosome that never arrives
BED = "\n".join([
    "# an annotation file: unsorted, overlapping, nested",
    "track name=test",
    "chrA\t300\t400\tinner",                 # nested in `outer`
    "chrA\t0\t2000\teverything",             # a piece over every row
    "chrA\t950\t990\tpast",                  # past the last row
    "chrA\t500\t510\tgap",                   # an empty piece between two rows
    "chrA\t200\t600\touter",
    "chrA\t140\t180\texons",                 # overlaps the next row of its name, which touches the one after it
    "chrA\t100\t150\texons",
    "chrA\t180\t190\texons",
    "chrA\t0\t100\tbefore",                  # before the first row
    "chrA\t700\t710\tgene",                  # three exons, given in descending order
    "chrA\t250\t260\tgene",
    "chrA\t210\t220\tgene",
    "chrB\t10\t60\tgene",                    # ... and one on another chromosome
    "chrA\t120\t121",                        # no name: chrA:120-121
    "chrA\t640\t650\tdup_end",               # ends on a run of equal starts (650), starts on another (640)
    "chrA\t899\t900\tlast",
    "chrC\t5\t50\tnever",                    # its chromosome never arrives
    "chrB\t0\t30\touter",
    "",
])
NAMES = ["inner", "everything", "past", "gap", "outer", "exons", "before", "gene", "chrA:120-121", "dup_end", "last", "never"]


def intervals(text=BED):
    """{name: [(chrom, start, end)]} of the literal BED, unmerged: what the oracle tests membership against."""
    out = {}
    for line in text.splitlines():
        if not line.strip() or line.startswith(("#", "track", "browser")):
            continue
        f = line.split("\t")
        out.setdefault(f[3] if len(f) > 3 else f"{f[0]}:{f[1]}-{f[2]}", []).append((f[0], int(f[1]), int(f[2])))
    return out


def intervals_dict(text=BED):
    """The literal BED as ``read_annotations``' dict input: {chrom: [(start, end[, name])]}."""
    out = {}
    for line in text.splitlines():
        if not line.strip() or line.startswith(("#", "track", "browser")):
            continue
        f = line.split("\t")
        out.setdefault(f[0], []).append((int(f[1]), int(f[2])) + tuple(f[3:4]))
    return out


def rows(n=300, n_class=4, seed=0, lo=100, hi=900, hole=(500, 510), dtype=np.float64):
    """(prob [n][n_class], start ascending with duplicates -- runs at 640 and 650 --, label int64) of one chromosome."""
    rng = np.random.default_rng(seed)
    start = rng.integers(lo, hi, size=n)
    start[(start >= hole[0]) & (start < hole[1])] = hole[1]
    start[:6] = [640, 640, 640, 650, 650, 650]
    start[6:10] = [lo, hi - 1, 120, 120]
    start = np.sort(start).astype(np.int64)
    prob = rng.dirichlet(np.ones(n_class), size=n).astype(dtype)
    prob[rng.integers(0, n, size=5), rng.integers(0, n_class, size=5)] = [0.0, 1.0, 2.0 ** -60, 1e-30, 0.5]
    label = rng.integers(0, n_class, size=n).astype(np.int64)
    return prob, start, label


def oracle(per_chrom, n_class, names, text=BED):
    """[[counts], [sums]] per name as Python integers, sums in units of 2^-71 (hi * 2^40 + lo): for each name and each row
    any(b0 <= start < b1) over the name's intervals on the row's chromosome.  `per_chrom`: {chrom: (prob, start, label)}."""
    from mural_amd.summaries import kmer_quantise
    iv = intervals(text)
    out = []
    for name in names:
        counts, sums = [0] * n_class, [0] * n_class
        for chrom, (prob, start, label) in per_chrom.items():
            hi, lo, bad = kmer_quantise(np.asarray(prob)[:, :n_class])
            assert not bad.any()
            hi, lo = hi.tolist(), lo.tolist()
            for i, s in enumerate(np.asarray(start).tolist()):
                if any(c == chrom and b0 <= s < b1 for c, b0, b1 in iv[name]):
                    counts[int(label[i])] += 1
                    for c in range(n_class):
                        sums[c] += (hi[i][c] << 40) + lo[i][c]
        out.append((counts, sums))
    return out


def as_integers(table):
    """[(counts, sums)] per group of an integer table [groups][3][n_class], and a check of lo < 2^40."""
    t = np.asarray(table).astype(np.uint64)
    assert (t[:, 2] < np.uint64(1 << 40)).all()
    t = t.tolist()
    return [(g[0], [(h << 40) + l for h, l in zip(g[1], g[2])]) for g in t]
