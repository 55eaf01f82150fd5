"""Shared material of the mutagenesis-profile tests: synthetic log-probabilities on the windows of tests/_mutagenesis_data.py whose
differences hit every edge of the quantisation and validity rules, and the brute force (Python ints over a ``delta`` map) the twin and
the device entry are judged against."""
from fractions import Fraction

import numpy as np

from tests import _mutagenesis_data as D

RADIUS, N_CLASS, N_GROUPS = 6, 4, 3
EDGE_SITE = 10                # pos 77 on '+': every column of its window is a plain base
F = np.float32
# delta of the edge site's first ids (its ref_logp is +0.0, so delta IS var_logp) and the q each must give; None: left out and counted
EDGE = [(F(0.0), 0), (F(-0.0), 0), (F(2.0 ** -31), 0), (F(-2.0 ** -31), 0),                # a tie at 0.5 goes to the even neighbour, 0
        (np.nextafter(F(2.0 ** -31), F(1)), 1), (-np.nextafter(F(2.0 ** -31), F(1)), -1),  # just past the tie
        (F(3 * 2.0 ** -31), 2), (F(-3 * 2.0 ** -31), -2),                                  # the tie at 1.5 goes to 2
        (F(2.0 ** -149), 0), (F(1.0), 1 << 30), (F(-1.5), -3 << 29),
        (F(255.99), int(Fraction(float(F(255.99))) * (1 << 30))), (np.nextafter(F(256), F(0)), (1 << 38) - (1 << 14)),
        (-np.nextafter(F(256), F(0)), -(1 << 38) + (1 << 14)),
        (F(256.0), None), (F(-256.0), None), (F(1e30), None), (F(np.inf), None), (F(-np.inf), None), (F(np.nan), None)]
EDGE_NONFINITE, EDGE_RANGE = 3, 3


def synthetic(seed=3):
    """(ref_logp (n, C), var_logp (n * W * 3, C), ref_symbols (n, W), group (n,) int32) of the 24 sites of D.sites() at R = 6: groups 0 .. 2
    and, among them, ids outside [0, 3) on both sides; ordinary differences of both signs everywhere, the EDGE values in class c = i % 4
    of id i of the edge site."""
    from mural_amd.mutagenesis import _codes, _window_symbols_host
    rng = np.random.default_rng(seed)
    pos, strand = D.sites()
    n, W = len(pos), 2 * RADIUS + 1
    ref_symbols, _ = _window_symbols_host(_codes(D.sequence()), pos, strand, RADIUS)
    assert (ref_symbols[EDGE_SITE] < 4).all() and (ref_symbols >= 4).any()          # dead columns: the N run, the IUPAC code, the ends
    ref_logp = np.log(rng.dirichlet(np.ones(N_CLASS), size=n)).astype(np.float32)
    ref_logp[EDGE_SITE] = 0.0
    var_logp = (np.repeat(ref_logp, W * 3, axis=0) + rng.normal(0, 0.7, size=(n * W * 3, N_CLASS))).astype(np.float32)
    base = EDGE_SITE * W * 3
    for i, (value, _) in enumerate(EDGE):
        var_logp[base + i, i % N_CLASS] = value
    group = (np.arange(n) % N_GROUPS).astype(np.int32)
    group[[3, 17]] = [-1, N_GROUPS]
    group[20] = np.int32(-2 ** 31)
    assert group[EDGE_SITE] in (0, 1, 2)
    return ref_logp, var_logp, ref_symbols, group


def quantise(d):
    """q of one float32 delta with Python's exact arithmetic (round() of a Fraction is to nearest, ties to even); None if it is left out."""
    d = float(d)
    if d != d or d in (float("inf"), float("-inf")) or abs(d) >= 256:
        return None
    return round(Fraction(d) * (1 << 30))


def brute_force(delta, ref_symbols, group, n_groups):
    """(table uint64 (n_groups, W, 4, 3, C, 5), (bits, nonfinite, out of range)) from a ``delta`` map (n, W, 4, C), term by term in Python
    ints.  The alternatives of a column are the three bases that are not its reference, ascending."""
    n, W, _, C = delta.shape
    table = np.zeros((n_groups, W, 4, 3, C, 5), np.uint64)
    cells = {}
    nonfinite = out_of_range = 0
    for s in range(n):
        g = 0 if group is None else int(group[s])
        if not 0 <= g < n_groups:
            continue
        for j in range(W):
            ref = int(ref_symbols[s, j])
            if ref > 3:
                continue
            for a, alt in enumerate(b for b in range(4) if b != ref):
                for c in range(C):
                    d = float(delta[s, j, alt, c])
                    q = quantise(d)
                    if q is None:
                        if d != d or abs(d) == float("inf"):
                            nonfinite += 1
                        else:
                            out_of_range += 1
                        continue
                    cell = cells.setdefault((g, j, ref, a, c), [0, 0, 0, 0, 0])
                    cell[0] += 1
                    cell[1] += q
                    cell[2] += abs(q)
                    cell[3] += (q * q) % (1 << 40)
                    cell[4] += (q * q) >> 40
    for key, cell in cells.items():
        table[key] = [x % (1 << 64) for x in cell]
    return table, ((1 if nonfinite else 0) | (2 if out_of_range else 0), nonfinite, out_of_range)


def delta_map(ref_logp, var_logp, ref_symbols):
    """The whole ``delta`` map of the synthetic rows through ``mutagenesis_reduce_host``."""
    from mural_amd.mutagenesis import mutagenesis_reduce_host
    n, W = ref_symbols.shape
    delta = np.full((n, W, 4, ref_logp.shape[1]), np.float32(7.0))
    with np.errstate(invalid="ignore", over="ignore"):
        return mutagenesis_reduce_host(ref_logp, var_logp, ref_symbols, 0, delta)
