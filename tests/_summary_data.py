"""Inputs of the summary tests (tests/test_gpu_summary.py on the device, tests/test_summary_host.py for the numpy path): the rows of one
chromosome, ascending in start, with the places where a segmented reduction over fixed chunks of rows can go wrong."""
import numpy as np

CHUNK = 2048                   # rows of a workgroup's chunk (mural_summary_chunk_rows(); the device test asserts it)
WINDOWS = (64, 1000, 1, 10 ** 9)      # the layouts below are built on the 64 bp windows; 1 bp; one window for the whole span
SIZES = (1, 63, 64, 65, CHUNK + 1, 3 * CHUNK + 17)


def starts(n, layout, seed=0):
    """`n` ascending starts.  "mixed": start 0 three times (duplicates), a window of one row, 50 empty windows in a row, runs of 1 .. 150
    rows, a new window beginning exactly at the first chunk border, one row before the second and one row behind the third.  "long": one
    window from row 0 over three whole chunks, the rest behind it."""
    rng = np.random.default_rng(seed + n)
    heads = {0}
    if layout == "long":
        assert n > 3 * CHUNK + 2
        heads |= {3 * CHUNK + 2} | {int(h) for h in range(3 * CHUNK + 3, n, 4)}
    else:
        heads |= {3, 4}
        at = 4
        while at < n:
            at += int(rng.integers(1, 150))
            heads.add(at)
        heads |= {CHUNK, 2 * CHUNK - 1, 3 * CHUNK + 1}
        heads -= {2 * CHUNK, 3 * CHUNK}
    first = np.zeros(n, bool)
    first[[h for h in heads if h < n]] = True
    step = first.astype(np.int64)
    if layout == "mixed":
        if n > 3:
            step[3] = 2                # window 1 stays empty, window 2 is the one row 3
        if n > 4:
            step[4] = 51               # 50 empty windows
    step[0] = 0
    window = np.cumsum(step)
    run = np.cumsum(first) - 1
    off = rng.integers(0, 64, n)
    if layout == "mixed":
        off[:3] = 0
    order = np.lexsort((off, run))     # ascending inside every run
    out = window * 64 + off[order]
    assert (np.diff(out) >= 0).all() and out[0] >= 0
    return out.astype(np.int64)


def rows(n, n_class, dtype, layout="mixed", seed=0):
    """(prob (n, n_class + 1) with the focal base in the last column, start, end, label float32)"""
    rng = np.random.default_rng(1000 * n_class + seed + n)
    prob = rng.random((n, n_class + 1)).astype(dtype)
    prob[:, :n_class] /= prob[:, :n_class].sum(axis=1, keepdims=True)
    prob[:, -1] = rng.integers(0, 4, n)
    start = starts(n, layout, seed)
    return prob, start, start + 1 + rng.integers(0, 3, n), rng.integers(0, n_class, n).astype(np.float32)


def brute_force(prob, start, end, label, n_class, windows, regions=None):
    """The specification, row by row in plain Python: ({W: {window index: [rows, label counts .., prob sums ..]}}, prob_sum, n_sites).
    `regions`: [(lo, hi)] of the chromosome; a row counts once per region that overlaps [start, end)."""
    tables = {W: {} for W in windows}
    total, n_sites = 0.0, 0
    for i in range(len(start)):
        p = [float(v) for v in prob[i, :n_class]]
        for W in windows:
            cell = tables[W].setdefault(int(start[i]) // W, [0.0] * (1 + 2 * n_class))
            cell[0] += 1
            cell[1 + int(label[i])] += 1
            for c in range(n_class):
                cell[1 + n_class + c] += p[c]
        w = 1 if regions is None else sum(1 for lo, hi in regions if lo < end[i] and hi > start[i])
        if w:
            r = 0.0
            for c in range(1, n_class):
                r += p[c]
            total += w * r
            n_sites += w
    return tables, total, n_sites


def dense(per_window, n_class):
    """(first window, table) of one brute_force table"""
    lo, hi = min(per_window), max(per_window)
    t = np.zeros((hi - lo + 1, 1 + 2 * n_class))
    for b, cell in per_window.items():
        t[b - lo] = cell
    return lo, t
