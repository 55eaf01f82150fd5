"""Shared material of the allele tests: the allele cases of the encoder contract on the chromosome of
tests/_mutagenesis_data.py, the rows they are encoded at (the edge sites plus sites placed so that an allele boundary falls on the
outermost columns), and the brute force they are judged against: patch the sequence STRING here, with the liveness rule written out
again, then run the oracle encoders of oracle/encode_ref.py on it at the alternate-haplotype position."""
import numpy as np

from oracle import encode_ref
from tests import _mutagenesis_data as D

LENGTH = D.LENGTH
INDEL_RADII = [6, 100]
INSERT_32 = "ACGTTGCAAGCTTCGATCGGATCCATGCAGTA"
assert len(INSERT_32) == 32

# (p, d, alt): every line of the case list of the issue; the last four are not live
LIVE = [
    (77, 0, "A"), (90, 0, "CGT"), (300, 0, INSERT_32),            # 1. insertions, k = 1, 3, 32
    (77, 1, ""), (200, 5, ""),                                    # 2. deletions, d = 1, 5
    (60, 250, ""), (250, 20, ""),                                 # 3. d > W (201 and 13): the window comes from beyond the deletion
    (120, 2, "ACGTA"), (310, 4, "G"),                             # 4. d != k, both nonzero
    (50, 3, "TGA"),                                               # 5. d = k = 3
    (77, 1, "C"),                                                 # 6. d = k = 1: the substitution encoder's case
    (D.N_RUN[0], D.N_RUN[1] - D.N_RUN[0], ""),                    # 7. a deletion that removes the N run
    (D.N_RUN[0] + 5, 0, "AC"),                                    # 8. an insertion inside the N run
    (D.IUPAC_POS - 1, 3, "TT"),                                   # 9. an allele covering the IUPAC position
    (0, 0, "GG"), (0, 2, ""), (0, 1, "TTT"),                      # 10. p = 0
    (LENGTH - 3, 3, "A"), (LENGTH - 1, 1, ""),                    # 11. p + d = length
    (LENGTH, 0, "ACG"),                                           # 12. an append
    (33, 0, ""),                                                  # d = k = 0: the identity
]
SUBST_CASE = 10                                                   # index of case 6
NOT_LIVE = [(LENGTH - 2, 5, "A"), (-1, 1, "A"), (LENGTH + 1, 0, "C"), (100, -1, "A")]
K33 = (140, 2, 33)                                                # (p, d, k) of the allele with 33 bases: built from raw arrays


def table():
    """(pos, ref_len, alt_len int64, alt uint64) of LIVE + NOT_LIVE + the k = 33 allele, packed here (base i in bits 2i, 2i+1)."""
    rows = LIVE + NOT_LIVE
    words = [sum("ACGT".index(ch) << (2 * i) for i, ch in enumerate(alt)) for _, _, alt in rows] + [0x1B1B1B1B1B1B1B1B]
    return (np.array([p for p, _, _ in rows] + [K33[0]], np.int64), np.array([d for _, d, _ in rows] + [K33[1]], np.int64),
            np.array([len(a) for _, _, a in rows] + [K33[2]], np.int64), np.array(words, np.uint64))


def patched(seq, v):
    """the sequence string of table entry v (-1 or out of the table: the sequence itself), the liveness rule written out"""
    rows = LIVE + NOT_LIVE
    if v < 0 or v >= len(rows):                                   # (the k = 33 entry is index len(rows): not live either)
        return seq
    p, d, alt = rows[v]
    if p < 0 or d < 0 or p + d > len(seq) or len(alt) > 32:
        return seq
    return seq[:p] + alt + seq[p + d:]


def rows_for(radius, local_radius, local_order, model_type="snv"):
    """(pos, strand, allele): for every table entry the edge sites of _mutagenesis_data.sites() and, for each allele boundary b (alternate
    coordinates p - 1, p, p + k - 1, p + k), the sites whose window column 0, last column, first local column, last local column and last
    k-mer column is b -- on both strands; then the same sites with allele -1 and with indices outside the table."""
    off0, W = (-radius, 2 * radius + 1) if model_type == "snv" else (-radius + 1, 2 * radius)
    base_pos, base_strand = D.sites()
    a_pos, _, a_k, _ = table()
    out = []
    for v in range(len(a_pos)):
        p, k = int(a_pos[v]), int(a_k[v])
        for s, st in zip(base_pos.tolist(), base_strand.tolist()):
            out.append((s, st, v))
        for b in (p - 1, p, p + k - 1, p + k):
            placed = [b - off0, b - off0 - (W - 1)]
            if model_type == "snv":
                placed += [b + local_radius, b - local_radius, b - local_radius + local_order - 1]
            for s in placed:
                out += [(s, 0, v), (s, 1, v)]
    for s, st in zip(base_pos.tolist(), base_strand.tolist()):
        out += [(s, st, -1), (s, st, len(a_pos)), (s, st, -7), (s, st, 1 << 40)]
    a = np.array(out, np.int64)
    return a[:, 0].copy(), a[:, 1].astype(np.uint8), a[:, 2].copy()


def brute_force(seq, pos, strand, allele, radius, local_radius, local_order, model_type="snv"):
    """(symbols, cat_x or None) row by row from the patched string through the oracle encoders"""
    syms, cats, cache = [], [], {}
    for p, s, v in zip(pos.tolist(), strand.tolist(), allele.tolist()):
        text = patched(seq, v)
        if text not in cache:
            cache[text] = encode_ref.seq_to_codes(text)
        codes, st = cache[text], ["-" if s else "+"]
        syms.append(D.symbols_of_onehot(encode_ref.onehot_encode(codes, [p], st, radius, model_type))[0])
        if model_type == "snv":
            cats.append(encode_ref.kmer_encode(codes, [p], st, local_radius, local_order)[0])
    return np.stack(syms), (np.stack(cats) if cats else None)
