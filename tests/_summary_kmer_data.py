"""Inputs of the k-mer summary tests (tests/test_summary_kmer_host.py for the numpy twin, tests/test_gpu_summary_kmer.py on the device):
one synthetic chromosome with the places where a k-mer key can go wrong, rows on it, and the specification row by row in plain Python."""
from fractions import Fraction

import numpy as np

L = 4099                       # no multiple of 16 (packed2 word) or 32 (nmask word)
KMERS = (1, 3, 5, 7)
SIZES = (1, 63, 64, 65, 2049)
N_RUN = (60, 69)               # Ns over the border of two 32-base nmask words
NEAR_N = {200: 201, 300: 302, 400: 403}      # site -> a single N 1, 2 and 3 bases from it
IUPAC = {500: "R", 1000: "Y"}
EDGES = (0, 1, 2, L - 3, L - 2, L - 1)      # the Python slice wraps / clamps here for k = 3, 5, 7
DUPLICATE = 777                # a row that comes three times


def _sequence():
    seq = np.random.default_rng(2024).choice(list("ACGT"), size=L)
    seq[N_RUN[0]:N_RUN[1]] = "N"
    for at in NEAR_N.values():
        seq[at] = "N"
    for at, code in IUPAC.items():
        seq[at] = code
    seq[10:14] = list("acgt")      # lower case packs like upper case
    return "".join(seq)


SEQ = _sequence()
assert len(SEQ) == L and L % 16 and L % 32 and N_RUN[0] // 32 != (N_RUN[1] - 1) // 32


def positions(n, seed=0):
    """`n` ascending starts: the edge sites, the sites next to Ns and IUPAC codes and the triple row first, random distinct positions
    behind them (rows of one start share their strand, so first appearance is decided by start alone)."""
    special = list(EDGES) + list(NEAR_N) + [N_RUN[0] - 1, N_RUN[1], 499, 501, 1001, 12] + [DUPLICATE] * 3
    if n <= len(special):
        return np.sort(np.array(special[:n], np.int64))
    rest = np.setdiff1d(np.arange(L), np.array(special))
    more = np.random.default_rng(seed + n).choice(rest, size=n - len(special), replace=False)
    return np.sort(np.r_[special, more].astype(np.int64))


def rows(n, n_class, dtype, indel=False, seed=0):
    """(prob (n, n_class + 1) with the focal base in the last column, start, end, strand uint8, label float32).  SNV rows are one base
    long; INDEL rows 1 .. 3 bases, so that their windows are k - 1, k and k + 1 bases long."""
    rng = np.random.default_rng(1000 * n_class + seed + n)
    start = positions(n, seed)
    prob = rng.random((n, n_class + 1)).astype(dtype)
    prob[:, :n_class] /= prob[:, :n_class].sum(axis=1, keepdims=True)
    prob[:, :n_class] = np.minimum(prob[:, :n_class], 1)
    prob[:, -1] = rng.integers(0, 4, n)
    prob[0, :n_class] = 0                      # the ends of the range: exactly 1 and exactly 0
    prob[0, 0] = 1
    if n > 3:
        prob[3, 1] = 1e-30                     # a tiny (scaled) probability: 2^-71 quantum, ~45 significant bits stay -- here none
        prob[2, 1] = 2.0 ** -72                # half-way cases of the lo limb: 0.5 quanta rounds to 0 (even) ...
    if n > 4:
        prob[4, 1] = 3 * 2.0 ** -72            # ... and 1.5 quanta to 2
    strand = (np.random.default_rng(7).integers(0, 2, L).astype(np.uint8))[start]      # by position: duplicates share it
    end = start + 1 + (rng.integers(0, 3, n) if indel else 0)
    same = np.r_[False, start[1:] == start[:-1]]
    end[same] = end[np.maximum.accumulate(np.where(same, 0, np.arange(n)))][same]
    return prob, start, end, strand, rng.integers(0, n_class, n).astype(np.float32)


def at_sites(n_class, dtype, seed=0):
    """Every A/T site of the chromosome (about 2 000 rows): A on '+', T on '-'."""
    start = np.array([p for p, b in enumerate(SEQ) if b in "ATat"], np.int64)
    rng = np.random.default_rng(seed + 5)
    prob = rng.random((len(start), n_class + 1)).astype(dtype)
    prob[:, :n_class] /= prob[:, :n_class].sum(axis=1, keepdims=True)
    prob[:, :n_class] = np.minimum(prob[:, :n_class], 1)
    strand = np.array([SEQ[p] in "Tt" for p in start], np.uint8)
    return prob, start, start + 1, strand, rng.integers(0, n_class, len(start)).astype(np.float32)


CASES = [(n, "rows") for n in SIZES] + [(0, "sites")]


def case(n, kind, n_class, dtype, indel=False):
    return at_sites(n_class, dtype) if kind == "sites" else rows(n, n_class, dtype, indel)


_COMP = {"A": "T", "C": "G", "G": "C", "T": "A"}


def brute_keys(start, end, minus, k, indel):
    """The k-mer of a row by Python's own slice: None unless it is k bases of A/C/G/T."""
    sub = SEQ[int(start) - k // 2 + (1 if indel else 0):int(end) + k // 2].upper()
    if len(sub) != k or any(b not in "ACGT" for b in sub):
        return None
    return "".join(_COMP[b] for b in reversed(sub)) if minus else sub


def brute_force(prob, start, end, strand, label, n_class, kmers, indel=False, mode=0, order_base=0):
    """The specification, row by row: {k: {k-mer: [label counts [n_class], sums of round_half_even(p * 2^71) [n_class] as Python
    integers, first appearance]}} (dicts in first-appearance order when the rows ascend in start)."""
    out = {k: {} for k in kmers}
    for i in range(len(start)):
        q = [round(Fraction(float(v)) * (1 << 71)) for v in prob[i, :n_class]]      # (float32 -> float is exact; round() is half-even)
        subs = [(0, False), (1, True)] if mode == 3 else [(0, mode == 2 or (mode == 0 and strand[i] != 0))]
        for k in kmers:
            for sub, minus in subs:
                name = brute_keys(start[i], end[i], minus, k, indel)
                if name is None:
                    continue
                cell = out[k].setdefault(name, [[0] * n_class, [0] * n_class, order_base + 2 * int(start[i]) + sub])
                cell[0][int(label[i])] += 1
                cell[1] = [a + b for a, b in zip(cell[1], q)]
                cell[2] = min(cell[2], order_base + 2 * int(start[i]) + sub)
    return out


def sums_as_dict(table, first, k):
    """``summary_kmer_host``'s (table, first) of one k in brute_force's form, in first-appearance order."""
    live = np.nonzero(table[:, 0].sum(axis=1) > 0)[0]
    order = live[np.argsort(first[live], kind="stable")]
    name = lambda g: "".join("ACGT"[(int(g) >> (2 * (k - 1 - j))) & 3] for j in range(k))      # noqa: E731
    return {name(g): [[int(v) for v in table[g, 0]], [(int(h) << 40) + int(l) for h, l in zip(table[g, 1], table[g, 2])], int(first[g])]
            for g in order}
