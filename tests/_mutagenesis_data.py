"""Shared material of the mutagenesis tests: a small chromosome with an N run and one IUPAC code, edge sites on both strands, the
substitution cases of the encoder contract, and the brute force they are judged against (patch the sequence STRING, then run the oracle
encoders of oracle/encode_ref.py on it)."""
import numpy as np

from oracle import encode_ref

LENGTH = 401
N_RUN = (150, 163)            # [lo, hi)
IUPAC_POS = 230               # an 'R'
CONFIGS = [(6, 5, 3), (100, 10, 3), (100, 7, 1)]        # (radius, local_radius, local_order)


def sequence(seed=5):
    rng = np.random.default_rng(seed)
    raw = rng.choice(np.frombuffer(b"ACGT", np.uint8), size=LENGTH)
    raw[N_RUN[0]:N_RUN[1]] = ord("N")
    raw[IUPAC_POS] = ord("R")
    raw[40] = ord("N")
    return raw.tobytes().decode()


def sites():
    """(pos, strand): 0, 1, n-1, n-2, next to and inside the N run, next to the IUPAC code, both strands each."""
    n = LENGTH
    p = [0, 1, n - 1, n - 2, N_RUN[0] - 1, N_RUN[0], N_RUN[0] + 5, N_RUN[1], IUPAC_POS - 2, IUPAC_POS, 77, 300]
    pos = np.array(p + p, np.int64)
    strand = np.array([0] * len(p) + [1] * len(p), np.uint8)
    return pos, strand


def substitution_cases(pos, strand, radius, local_radius, local_order):
    """Rows (pos, strand, sub_pos, sub_base) for every site: the substitution at window column 0, at the last column, at the focal base,
    at the first and last base of the local window (exactly the outermost k-mer column changes), inside the N run, on the IUPAC
    position, outside the window, outside the chromosome (both ends) and sub_base = 255."""
    rows = []
    for p, s in zip(pos.tolist(), strand.tolist()):
        offs = [-radius, radius, 0, -local_radius, local_radius, -local_radius + local_order - 1, 1]
        targets = [p + o for o in offs] + [N_RUN[0] + 3, IUPAC_POS, p + radius + 1, p - radius - 1, -1, LENGTH, LENGTH + 7, -radius]
        for k, t in enumerate(targets):
            rows.append((p, s, t, (k + p) % 4))
        rows.append((p, s, p, 255))
        rows.append((p, s, p + 1, 4))              # above 3: no substitution either
    a = np.array(rows, np.int64)
    return a[:, 0].copy(), a[:, 1].astype(np.uint8), a[:, 2].copy(), a[:, 3].astype(np.uint8)


def patched(seq, sub_pos, sub_base):
    if sub_base > 3 or sub_pos < 0 or sub_pos >= len(seq):
        return seq
    return seq[:sub_pos] + "ACGT"[sub_base] + seq[sub_pos + 1:]


_OHE_KEY = {tuple(np.round(row * 12).astype(int)): code for code, row in enumerate(encode_ref._OHE)}


def symbols_of_onehot(x):
    """(n, 4, W) one-hot / fractional columns -> (n, W) codes: the symbol view of ``onehot_encode``."""
    q = np.round(x * 12).astype(int).transpose(0, 2, 1)
    return np.array([[_OHE_KEY[tuple(col)] for col in row] for row in q], np.uint8)


def brute_force(seq, pos, strand, sub_pos, sub_base, radius, local_radius, local_order):
    """(symbols, cat_x) row by row from the patched string through the oracle encoders."""
    syms, cats = [], []
    cache = {}
    for p, s, sp, sb in zip(pos.tolist(), strand.tolist(), sub_pos.tolist(), sub_base.tolist()):
        text = patched(seq, sp, sb)
        if text not in cache:
            cache[text] = encode_ref.seq_to_codes(text)
        codes, st = cache[text], ["-" if s else "+"]
        syms.append(symbols_of_onehot(encode_ref.onehot_encode(codes, [p], st, radius))[0])
        cats.append(encode_ref.kmer_encode(codes, [p], st, local_radius, local_order)[0])
    return np.stack(syms), np.stack(cats)
