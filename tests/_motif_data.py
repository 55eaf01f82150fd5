"""Seeded inputs of the motif-table tests (tests/test_summary_motif_host.py, tests/test_gpu_summary_motif.py, tests/test_dist_motif_gloo.py)
and of their fixture generator (tools/make_motif_golden.py, which records what the reference's calc_motif_corr.run_motif_corr_calc
writes for them in tests/golden/motif.npz), with the specification row by row in plain Python.

Two chromosomes per case, in FASTA and table order `chrM2` (4 001 bases) then `chr10s` (29 bases): sorted by name the short one comes
first, so the order of first appearance ACROSS chromosomes tells table order from name order.  What the long one holds:

  * sites within m - 1 of both ends for every m of MOTIFS, so that slice starts go negative and wrap, and slice ends pass the end;
  * a run of Ns over the border of two nmask words and single Ns: rows beside them lose some windows, rows on them lose all;
  * a homopolymer run of HOMOPOLYMER[1] - HOMOPOLYMER[0] = 24 > 2 * 7 - 1 bases: a row in its middle adds m times to one cell;
  * INDEL rows of 1, 2 and 3 bases: a window of a row of d bases is d + m - 1 long before clipping, so only rows of one base have
    windows inside the chromosome; a longer row keeps exactly the windows that the chromosome's end clips to m bases.

A WRAPPED slice of exactly m bases, which one might look for on the short chromosome, does not exist for any chromosome length L: the
slice chrom[a:b] of a row has -(m - 1) <= a < 0 only with b = a + d + m - 1 >= 1; Python reads it as [max(L + a, 0), min(b, L)).  With
L + a >= 0 its length is min(b, L) - L - a, which is -a < m for b >= L and b - a - L = d + m - 1 - L otherwise, m only for
L = d - 1 < b; with L + a < 0 its length is min(b, L) <= L < -a < m.  The short chromosome has every such slice all the same (every
site of it is a row, and 29 < 2 * 15), the golden records that the reference keeps none of them, and the tests assert it.

NO_WINDOW_CAP: at most this share of a case's rows may be left without any kept window at m = 3 (tests/test_summary_motif_host.py
asserts it against the reference's recorded counts), so that no test passes on a nearly empty table.

The probabilities of the tables are spread over 1.25e-9 .. 1.  The cells of the reduction hold sums of probabilities quantised to
2^-71 (an absolute error of at most 2^-72 = 2.1e-22 per term), which the golden tests compare with the reference's float64 sums to 1e-12
relative -- the figure tests/test_gpu_tables.py holds ``tables.kmer_table`` to --: that is within the format's reach for probabilities of
2.1e-10 and more, and a sum of smaller ones is below it by construction, not by an error of the code.  Probabilities below the quantum
(1e-30, the half-way cases 2^-72 and 3 * 2^-72) are in TINY, which the brute-force tests put into rows: there the comparison is exact."""
import os
from fractions import Fraction

import numpy as np

from tests._tables_data import _fasta, _table

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "motif.npz")

MOTIFS = (3, 5, 7)
CHROMS = (("chrM2", 4001), ("chr10s", 29))      # FASTA and table order; by name chr10s sorts first
N_RUN = (60, 69)               # Ns over the border of two 32-base nmask words
SINGLE_N = (201, 302, 403, 1000)
HOMOPOLYMER = (2000, 2024)     # a run of A
NO_WINDOW_CAP = 0.10
CASES = {"snv": dict(n_class=4, model_type="snv", seed=11), "indel": dict(n_class=8, model_type="indel", seed=12)}
assert sorted(n for n, _ in CHROMS) != [n for n, _ in CHROMS]


def sequences():
    rng = np.random.default_rng(20261018)
    out = {}
    for name, length in CHROMS:
        seq = rng.choice(list("ACGT"), size=length)
        if length > 100:
            seq[N_RUN[0]:N_RUN[1]] = "N"
            for at in SINGLE_N:
                seq[at] = "N"
            seq[HOMOPOLYMER[0]:HOMOPOLYMER[1]] = "A"
            seq[10:14] = list("acgt")      # lower case packs like upper case
        out[name] = "".join(seq)
    return out


SEQS = sequences()


def _positions(name, length, rng):
    if length <= 100:
        return np.arange(length, dtype=np.int64)
    edge = list(range(0, 16)) + list(range(length - 16, length))
    special = edge + list(range(N_RUN[0] - 8, N_RUN[1] + 8)) + [a + o for a in SINGLE_N for o in range(-7, 8)]
    special += list(range(HOMOPOLYMER[0] - 8, HOMOPOLYMER[1] + 8))
    return np.unique(np.r_[special, rng.choice(length, size=2 * length // 3, replace=False)].astype(np.int64))


TINY = (1e-30, 2.0 ** -72, 3 * 2.0 ** -72, 0.0, 1.0)


def _probs(rng, n, n_class):
    """Rows of probabilities spread over 1.25e-9 .. 1 (prob0 = 1 - the rest) as '%.4g' text."""
    p = 10.0 ** rng.uniform(-8, -0.8, size=(n, n_class - 1)) / n_class
    return [["%.4g" % (1.0 - r.sum())] + ["%.4g" % v for v in r] for r in p]


_CACHE = {}


def case(name):
    """{"n_class", "model_type", "table" (text), "fasta" (text), "rows": {chromosome: (prob float64 [n][n_class] as the table's '%.4g'
    text reads, start, end, label int64)} in table order}: about 3 000 rows."""
    if name in _CACHE:
        return _CACHE[name]
    c = CASES[name]
    rng = np.random.default_rng(c["seed"])
    nc, indel = c["n_class"], c["model_type"] == "indel"
    lines, rows = [], {}
    for chrom, length in CHROMS:
        start = _positions(chrom, length, rng)
        n = len(start)
        span = rng.choice([1, 2, 3], size=n, p=[0.94, 0.03, 0.03]) if indel else np.ones(n, np.int64)
        if indel:                      # rows of 2 and 3 bases whose windows the chromosome's end clips to m bases
            span[start >= length - 9] = np.where(np.arange((start >= length - 9).sum()) % 3 == 0, 1, span[start >= length - 9])
            span[(start >= length - 9) & (start % 2 == 0)] = 2
            span[start == length - 5] = 3
        end = start + span
        label = rng.integers(0, nc, n)
        text = _probs(rng, n, nc)
        for i in range(n):
            lines.append([chrom, str(start[i]), str(end[i]), "+-"[int(rng.integers(0, 2))], str(label[i])] + text[i])
        rows[chrom] = (np.array([[float(v) for v in r] for r in text]), start, end.astype(np.int64), label.astype(np.int64))
    out = dict(n_class=nc, model_type=c["model_type"], table=_table(lines, nc), fasta=_fasta(list(SEQS.items())), rows=rows)
    _CACHE[name] = out
    return out


def write_case(d, name, gz=False):
    """Write a case's files under directory d: (table path, fasta path)."""
    import gzip
    c = case(name)
    table, fasta = os.path.join(d, f"{name}.tsv" + (".gz" if gz else "")), os.path.join(d, f"{name}.fa")
    with open(table, "wb") as fh:
        fh.write(gzip.compress(c["table"].encode()) if gz else c["table"].encode())
    with open(fasta, "w") as fh:
        fh.write(c["fasta"])
    return table, fasta


_COMP = {"A": "T", "C": "G", "G": "C", "T": "A"}


def revcomp(s):
    return "".join(_COMP[b] for b in reversed(s))


def windows(seq, start, end, m, indel):
    """[(i, the window's m bases)] of a row by Python's own slices, in the reference's order: the kept windows only."""
    out = []
    for i in range(1 if indel else 0, m):
        a, b = (start - i + 1, end + m - i) if indel else (start - i, end + m - 1 - i)
        sub = seq[int(a):int(b)].upper()
        if len(sub) == m and all(ch in "ACGT" for ch in sub):
            out.append((i, sub))
    return out


def brute_force(name, m, prob_of=None):
    """The specification, row by row in table order: {entry name: [label counts [n_class], sums of round_half_even(p * 2^71) [n_class] as
    Python integers, (chromosome ordinal, start, i) of its first window]} in dict insertion order, and the number of rows without a
    window.  `prob_of`: chromosome -> the probabilities to use in place of the case's (another dtype)."""
    c = case(name)
    nc, indel = c["n_class"], c["model_type"] == "indel"
    out, empty = {}, 0
    for ordinal, (chrom, (prob, start, end, label)) in enumerate(c["rows"].items()):
        prob = prob if prob_of is None else prob_of[chrom]
        for r in range(len(start)):
            q = [round(Fraction(float(v)) * (1 << 71)) for v in prob[r, :nc]]      # (round() is half-even)
            kept = windows(SEQS[chrom], start[r], end[r], m, indel)
            empty += not kept
            for i, sub in kept:
                key = sub if sub in out else revcomp(sub) if revcomp(sub) in out else sub
                cell = out.setdefault(key, [[0] * nc, [0] * nc, (ordinal, int(start[r]), i)])
                cell[0][int(label[r])] += 1
                cell[1] = [a + b for a, b in zip(cell[1], q)]
    return out, empty


def twin_tables(name, motifs=MOTIFS, prob_of=None):
    """``summary_motif_host`` over the case's chromosomes, the ordinal of each (table order) above its words: {m: (table, first)}."""
    from mural_amd.predict import _MOTIF_ORD_SHIFT, _MOTIF_POS_SHIFT, summary_motif_host
    c = case(name)
    out = {}
    for ordinal, (chrom, (prob, start, end, label)) in enumerate(c["rows"].items()):
        prob = prob if prob_of is None else prob_of[chrom]
        _, status = summary_motif_host(SEQS[chrom], prob, start, end, label, c["n_class"], motifs, c["model_type"] == "indel",
                                       order_base=ordinal << (_MOTIF_ORD_SHIFT - _MOTIF_POS_SHIFT), into=out)
        assert status == 0
    return out


def sums_as_dict(table, first, m):
    """(table, first) of one m in brute_force's form."""
    from mural_amd.predict import _MOTIF_ORD_SHIFT, motif_table_from_sums
    names, _ = motif_table_from_sums(table, first, m, table.shape[2])
    live = np.nonzero(table[:, 0].sum(axis=1) > 0)[0]
    order = live[np.argsort(first[live], kind="stable")]
    word = lambda f: (int(f) >> _MOTIF_ORD_SHIFT, (int(f) & ((1 << _MOTIF_ORD_SHIFT) - 1)) >> 5, (int(f) >> 1) & 15)      # noqa: E731
    return {nm: [[int(v) for v in table[g, 0]], [(int(h) << 40) + int(l) for h, l in zip(table[g, 1], table[g, 2])], word(first[g])]
            for nm, g in zip(names, order)}


def golden(name, m):
    """What the reference wrote for a case and a motif length: (entry names in order, avg_obs_rate [entries][n_class - 1], avg_pred_rate,
    counts int64 [entries][n_class] of number_of_mut1 .. and number_of_all, the correlation file's lines)."""
    fx = np.load(GOLDEN)
    nc = CASES[name]["n_class"]
    rows = [ln.split("\t") for ln in str(fx[f"{name}/motif{m}/rates"]).split("\n")[1:] if ln]
    return ([r[0] for r in rows], np.array([[float(v) for v in r[1:nc]] for r in rows]), np.array([[float(v) for v in r[nc:2 * nc - 1]] for r in rows]),
            np.array([[int(v) for v in r[2 * nc - 1:]] for r in rows], np.int64), str(fx[f"{name}/motif{m}/corr"]).split("\n")[:-1])
