"""Rows and hand-computed tables shared by the tests of the calibration-metrics summary (mural_summary_calib_rows and its numpy twin
``predict.summary_calib_host``)."""
import math

import numpy as np

LO_BITS, SCORE_BITS, NLL_BITS = 46, 16, 13      # the scaling stated above predict.summary_calib_host


def cell(nc, nb, g, b):
    """index of the first of the four cells (rows, score hi, score lo, hits) of bin b of group g"""
    return 6 + nc + 4 * (g * nb + b)


def pair_value(table, at, bits):
    """the real value of the two-limb sum at table[at], table[at + 1]"""
    t = np.asarray(table).tolist()
    return ((t[at] << LO_BITS) + t[at + 1]) / (1 << (bits + LO_BITS))


# ---- edge rows at n_class = 4, n_bins = 10: every score is exact (the positive probabilities of a row are equal, so softmax(log p)
# is 1 / their number whatever the math library), and so is every cell but the NLL pair
EDGE_NC, EDGE_NB = 4, 10
EDGE_PROB = np.array([[1.0, 0.0, 0.0, 0.0],            # label 0: confidence 1.0 -> the last bin, NLL term 0
                      [0.5, 0.5, 0.0, 0.0],            # label 2: q_label = 0 -> inf_rows; 0.5 sits ON a bound: bin 4 = (0.4, 0.5]
                      [0.25, 0.25, 0.25, 0.25],        # label 3: the first maximum (class 0) is the prediction: no hit
                      [0.0, 0.0, 1.0, 0.0]])           # label 2
EDGE_LABEL = np.array([0, 2, 3, 2])
# rows that are skipped everywhere: (probabilities, label, status bit)
BAD_ROWS = [([0.7, 0.1, 0.1, 0.1], -1, 2), ([0.7, 0.1, 0.1, 0.1], 4, 2), ([np.nan, 0.5, 0.25, 0.25], 1, 8),
            ([-0.25, 0.75, 0.25, 0.25], 1, 8), ([1.5, 0.0, 0.0, 0.0], 0, 8)]


def edge_table():
    """The table of the four EDGE rows, worked out by hand; the NLL pair is left at zero (its one non-zero term, -log 0.25 of the
    third row, goes through a logarithm): ``EDGE_NLL`` is its value."""
    nc, nb = EDGE_NC, EDGE_NB
    t = np.zeros(6 + nc + 4 * nb * (nc + 1), np.uint64)
    one = 1 << SCORE_BITS                                  # a score of 1.0 as a hi limb; halves and quarters are exact hi limbs too
    t[0], t[1] = 4, 1
    t[2:2 + nc] = [1, 0, 2, 1]
    t[4 + nc] = int((0.0 + 1.5 + 0.75 + 0.0) * one)        # Brier: 0 | .25 + .25 + 1 | 3 * .0625 + .5625 | 0
    # top-label bins: two rows of confidence 1.0 in bin 9 (both hits), 0.5 in bin 4 (prediction 0, label 2), 0.25 in bin 2 (0 vs 3)
    t[cell(nc, nb, 0, 9):cell(nc, nb, 0, 9) + 4] = [2, 2 * one, 0, 2]
    t[cell(nc, nb, 0, 4):cell(nc, nb, 0, 4) + 4] = [1, one // 2, 0, 0]
    t[cell(nc, nb, 0, 2):cell(nc, nb, 0, 2) + 4] = [1, one // 4, 0, 0]
    # class bins; a score of exactly 0 falls in no bin
    t[cell(nc, nb, 1, 9):cell(nc, nb, 1, 9) + 4] = [1, one, 0, 1]            # class 0: 1.0 (label 0)
    t[cell(nc, nb, 1, 4):cell(nc, nb, 1, 4) + 4] = [1, one // 2, 0, 0]       #          0.5 (label 2)
    t[cell(nc, nb, 1, 2):cell(nc, nb, 1, 2) + 4] = [1, one // 4, 0, 0]       #          0.25 (label 3)
    t[cell(nc, nb, 2, 4):cell(nc, nb, 2, 4) + 4] = [1, one // 2, 0, 0]       # class 1: 0.5 (label 2), 0.25 (label 3)
    t[cell(nc, nb, 2, 2):cell(nc, nb, 2, 2) + 4] = [1, one // 4, 0, 0]
    t[cell(nc, nb, 3, 2):cell(nc, nb, 3, 2) + 4] = [1, one // 4, 0, 0]       # class 2: 0.25 (label 3), 1.0 (label 2)
    t[cell(nc, nb, 3, 9):cell(nc, nb, 3, 9) + 4] = [1, one, 0, 1]
    t[cell(nc, nb, 4, 2):cell(nc, nb, 4, 2) + 4] = [1, one // 4, 0, 1]       # class 3: 0.25 (label 3)
    return t


EDGE_NLL = math.log(4.0)                                   # the sum of the finite NLL terms: 0 + (inf row left out) + log 4 + 0


def nll_tolerance(dtype):
    """-log 0.25 is evaluated in the probabilities' own precision: one unit in the last place of that format at log 4 (2^-23 for
    float32, 2^-52 for float64, log 4 lies in [1, 2)) bounds a faithfully rounded logarithm, whichever library computes it."""
    return 2.0 ** -23 if np.dtype(dtype) == np.float32 else 2.0 ** -52


def without_nll(table, nc):
    t = np.array(table, np.uint64)
    t[2 + nc:4 + nc] = 0
    return t


def random_rows(n, nc, seed, dtype=np.float64, sharp=True):
    """Dirichlet rows shaped like a mutation-rate model's (class 0 near 1) with labels drawn from them."""
    rng = np.random.default_rng(seed)
    prob = rng.dirichlet([40.0 if sharp else 2.0] + [1.0] * (nc - 1), size=n).astype(dtype)
    label = np.array([rng.choice(nc, p=p / p.sum()) for p in prob.astype(np.float64)], np.int64) if n else np.zeros(0, np.int64)
    return prob, label


def metrics_float64(prob, label, nb, bounds, n_seen=None):
    """NLL / ECE / CwECE / Brier by their definitions in plain float64 numpy (valid rows only): an independent statement of what
    ``calib_metrics_from_sums`` derives from the integer tables."""
    prob = np.asarray(prob, np.float64)
    n, nc = prob.shape
    q = prob / prob.sum(axis=1, keepdims=True)
    bounds = np.asarray(bounds, np.float64)

    def ece(score, hit):
        tot = 0.0
        for lo, hi in zip(bounds[:-1], bounds[1:]):
            inb = (score > lo) & (score <= hi)
            if inb.any():
                tot += abs(score[inb].mean() - hit[inb].mean()) * inb.sum() / n
        return tot

    n_seen = int(label.max()) + 1 if n_seen is None else n_seen      # ClasswiseECELoss: max(labels) + 1 classes
    return {"nll": float(-np.log(q[np.arange(n), label]).mean()), "ece": ece(q.max(axis=1), q.argmax(axis=1) == label),
            "c_ece": float(np.mean([ece(q[:, c], label == c) for c in range(n_seen)])),
            "brier": float((((label[:, None] == np.arange(nc)) - q) ** 2).sum() / n)}
