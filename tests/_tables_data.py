"""Seeded inputs of the prediction-table tests (tests/test_tables.py, tests/test_gpu_tables.py) and of their fixture generator
(tools/make_tables_golden.py, which records the reference scripts' outputs for them in tests/golden/tables.npz).

Each case is a prediction table (text), the FASTA it was predicted on (text), a benchmark-region BED (text) and the settings the
fixture was recorded with.  Everything is rebuilt from seeds: the fixture holds only the reference's outputs."""
import os

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "tables.npz")

SCALE_FACTOR = 0.37
GENOMEWIDE_MU = 5e-9
M_PROP, G_PROP = 0.355, 0.475
CASES = ("config1", "snv", "indel")


def _fasta(records):
    out = []
    for name, seq in records:
        out.append(f">{name} synthetic\n")
        out.extend(seq[i:i + 60] + "\n" for i in range(0, len(seq), 60))
    return "".join(out)


def _g4(v):
    return "%.4g" % v


def _probs(rng, n, n_class):
    """Rows of probabilities spread over 1e-12 .. 1 (prob0 = 1 - the rest), '%.4g' text; a few fields in other notations that the
    exact fast path does not cover (17 significant digits, exponents beyond 1e+-22)."""
    p = 10.0 ** rng.uniform(-12, -0.8, size=(n, n_class - 1)) / n_class
    cols = [[_g4(1.0 - s) for s in p.sum(axis=1)]] + [[_g4(v) for v in p[:, c]] for c in range(n_class - 1)]
    rows = [list(r) for r in zip(*cols)]
    for i in rng.choice(n, size=max(1, n // 50), replace=False):
        c = int(rng.integers(1, n_class))
        rows[i][c] = "%.17g" % p[i, c - 1] if i % 2 else "%.3e" % (p[i, c - 1] * 1e-25)
    return rows


def _genome(rng, length, n_frac=0.01, iupac=8, lower=0.2):
    seq = np.frombuffer(b"ACGT", np.uint8)[rng.integers(0, 4, size=length)].copy()
    seq[rng.random(length) < n_frac] = ord("N")
    seq[rng.integers(0, length, size=iupac)] = np.frombuffer(b"RYKMSW", np.uint8)[rng.integers(0, 6, size=iupac)]
    low = rng.random(length) < lower
    seq[low] = seq[low] + 32
    return seq.tobytes().decode()


def _table(rows, n_class):
    head = "\t".join(["chrom", "start", "end", "strand", "mut_type"] + [f"prob{i}" for i in range(n_class)]) + "\n"
    return head + "".join("\t".join(r) + "\n" for r in rows)


def _bed(rng, chroms):
    out = []
    for name, length in chroms:
        for _ in range(6):
            a = int(rng.integers(0, length - 10))
            b = min(length, a + int(rng.integers(5, length // 3)))
            out.append(f"{name}\t{a}\t{b}\n")
    return "".join(out)


def snv_case():
    rng = np.random.default_rng(20261016)
    chroms = [("chrA", 3000), ("01", 2000), ("chr_x", 2500)]
    genome = {name: _genome(rng, n) for name, n in chroms}
    rows = []
    for name, n in chroms:
        pos = np.unique(np.concatenate([[0, 1, 2, n - 3, n - 2, n - 1], rng.integers(0, n, size=n // 3)]))
        probs = _probs(rng, len(pos), 4)
        for p, pr in zip(pos, probs):
            rows.append([name, str(p), str(p + 1), "+-"[int(rng.integers(0, 2))], str(int(rng.integers(0, 4)))] + pr)
    return dict(table=_table(rows, 4), fasta=_fasta(list(genome.items())), bed=_bed(rng, chroms), n_class=4, model_type="snv",
                kmers=(3, 5, 7), windows=(100, 1000), strands=(None,))


def indel_case():
    rng = np.random.default_rng(7031)
    chroms = [("chrI", 4000), ("chrII", 3000)]
    genome = {name: _genome(rng, n) for name, n in chroms}
    rows = []
    for name, n in chroms:
        pos = np.unique(np.concatenate([[0, 1, n - 2, n - 1], rng.integers(0, n, size=n // 3)]))
        probs = _probs(rng, len(pos), 8)
        for p, pr in zip(pos, probs):
            span = 1 if rng.random() < 0.9 else 2
            rows.append([name, str(p), str(p + span), "+", str(int(rng.integers(0, 8)))] + pr)
    return dict(table=_table(rows, 8), fasta=_fasta(list(genome.items())), bed=_bed(rng, chroms), n_class=8, model_type="indel",
                kmers=(2, 4, 6), windows=(100, 1000), strands=("+", "-", "both"))


def config1_case():
    """table_calibrated of tests/golden/config1_example.npz (the reference's own predict output) on its seeded synthetic chr2L,
    rebuilt as tests/test_gpu_config5.py does."""
    fx = np.load(os.path.join(ROOT, "tests", "golden", "config1_example.npz"))
    rows = [ln.split("\t") for ln in str(fx["bed"]).split("\n") if ln]
    rng = np.random.default_rng(int(fx["genome_seed"]))
    seq = np.frombuffer(b"ACGT", np.uint8)[rng.integers(0, 4, size=int(fx["genome_len"]))].copy()
    for c, s_, e_, name, score, strand in rows:
        seq[int(s_)] = ord("A") if strand == "+" else ord("T")
    seq = seq.tobytes().decode()
    bed = "chr2L\t1000\t150000\nchr2L\t100000\t250000\nchr2L\t300000\t320000\n"
    return dict(table=str(fx["table_calibrated"]), fasta=_fasta([("chr2L", seq)]), bed=bed, n_class=4, model_type="snv",
                kmers=(3, 5, 7), windows=(10000, 100000), strands=(None,))


def case(name):
    return {"config1": config1_case, "snv": snv_case, "indel": indel_case}[name]()


def write_case(d, name, gz=False):
    """Write a case's files under directory d: (table path, fasta path, bed path)."""
    import gzip
    c = case(name)
    table = os.path.join(d, f"{name}.tsv" + (".gz" if gz else ""))
    with open(table, "wb") as fh:
        fh.write(gzip.compress(c["table"].encode()) if gz else c["table"].encode())
    fasta, bed = os.path.join(d, f"{name}.fa"), os.path.join(d, f"{name}.bed")
    with open(fasta, "w") as fh:
        fh.write(c["fasta"])
    with open(bed, "w") as fh:
        fh.write(c["bed"])
    return table, fasta, bed


def strand_tag(strand):
    return {None: "row", "+": "pos", "-": "neg", "both": "both"}[strand]
