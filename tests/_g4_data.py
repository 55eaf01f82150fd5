"""Values at which a '%.4g' formatter can go wrong, shared by tests/test_tsv.py (host compile of csrc/tsv.hip) and
tests/test_gpu_tsv.py (device compile): the decimal ties (N + 0.5) x 10^(e10 - 3), N = 1000 .. 9999, rounded to the table's type, with
their +-1 and +-2 ulp neighbours, and every tie that the type holds exactly.

The groups of a type (each a sorted array of distinct finite values of that type):
  prob    all N in the decades e10 = -8 .. 0, the decades a probability table holds;
  routes  all N in the decades either side of each change of the formatter's rounding route, p = 3 - e10 in {-23, -22, 22, 23} and,
          for float64, {300, 301};
  edges   all N in the lowest decades (float64: the subnormal ones; float32: around 1e-38 and 1e-45) and the highest finite one;
  sparse  every 37th N from a seeded offset in every other decade of the type's range;
  ties    every exactly representable tie with its +-1 ulp neighbours.
"""
import functools
from fractions import Fraction

import numpy as np

GROUPS = ("prob", "routes", "edges", "sparse", "ties")
DTYPES = {"float32": np.float32, "float64": np.float64}
EXACT_TIES = {"float32": 48_934, "float64": 160_334}      # over every N and every decade of the double range

_RANGE = {"float32": (-46, 38), "float64": (-324, 308)}      # decades of the smallest subnormal and of the largest finite value
_ALL_N = {
    "float32": {"prob": range(-8, 1), "routes": (26, 25, -19, -20), "edges": (-46, -45, -44, -39, -38, -37, 38)},
    "float64": {"prob": range(-8, 1), "routes": (26, 25, -19, -20, -297, -298), "edges": tuple(range(-324, -307)) + (308,)},
}
_SEED = 20240611


def _tie_f64(ns, e10):
    """The float64 nearest to (N + 0.5) x 10^(e10 - 3) for each N (float() of a decimal string rounds correctly; inf past the range)."""
    return np.array([float("%d5e%d" % (n, e10 - 4)) for n in ns], np.float64)


def _tie_f32(ns, e10):
    """The float32 nearest to the same ties.  Rounding the nearest float64 once more is right unless that float64 IS the mid-point of
    two float32 values (the tie itself then lies to one side of it): those are settled with exact fractions."""
    d = _tie_f64(ns, e10)
    with np.errstate(over="ignore"):
        f = d.astype(np.float32)
    r = d - f.astype(np.float64)
    g = np.nextafter(f, np.where(r > 0, np.inf, -np.inf).astype(np.float32))
    with np.errstate(invalid="ignore"):
        mid = 0.5 * f.astype(np.float64) + 0.5 * g.astype(np.float64)
    for i in np.nonzero((r != 0) & (mid == d) & np.isfinite(f) & np.isfinite(g))[0]:
        tie = Fraction(10 * int(ns[i]) + 5) * Fraction(10) ** (e10 - 4)
        da, db = abs(Fraction(float(f[i])) - tie), abs(Fraction(float(g[i])) - tie)
        if db < da or (db == da and int(g[i:i + 1].view(np.uint32)[0]) % 2 == 0):
            f[i] = g[i]
    return f


def _neighbours(c, reach):
    """c and its neighbours up to `reach` ulps either side, in c's type; the finite ones, sorted, each once."""
    out = [c]
    for direction in (np.inf, -np.inf):
        w = c
        for _ in range(reach):
            w = np.nextafter(w, c.dtype.type(direction))
            out.append(w)
    v = np.concatenate(out)
    return np.unique(v[np.isfinite(v)])


@functools.lru_cache(maxsize=None)
def exact_ties(dtype):
    """Every (N + 0.5) x 10^(e10 - 3), N = 1000 .. 9999, that `dtype` holds exactly, as a sorted array of that type.  A tie is
    (2N + 1) x 5^k x 2^(k - 1) with k = e10 - 3: for k < 0 it needs 5^-k | 2N + 1 <= 19999 (k >= -6), for k >= 0 the odd part
    (2N + 1) x 5^k has to fit the significand (k <= 18 for float64); the loop is wider than that and the test is the exact one."""
    if dtype == "float32":
        d = exact_ties("float64")
        f = d.astype(np.float32)
        return f[f.astype(np.float64) == d]
    found = []
    for k in range(-9, 25):
        scale = Fraction(10) ** k / 2
        for n in range(1000, 10000):
            tie = (2 * n + 1) * scale
            v = float(tie)
            if Fraction(v) == tie:
                found.append(v)
    return np.unique(np.array(found, np.float64))


@functools.lru_cache(maxsize=None)
def values(dtype, group):
    """The values of one group (module docstring) as a read-only array of `dtype`."""
    nearest = _tie_f32 if dtype == "float32" else _tie_f64
    all_n = _ALL_N[dtype]
    if group == "ties":
        v = _neighbours(exact_ties(dtype), 1)
    elif group == "sparse":
        rng = np.random.default_rng(_SEED)
        dense = {e for decades in all_n.values() for e in decades}
        lo, hi = _RANGE[dtype]
        v = _neighbours(np.concatenate([nearest(range(1000 + int(rng.integers(0, 37)), 10000, 37), e10)
                                        for e10 in range(lo, hi + 1) if e10 not in dense]), 2)
    else:
        v = _neighbours(np.concatenate([nearest(range(1000, 10000), e10) for e10 in all_n[group]]), 2)
    assert v.dtype == DTYPES[dtype]
    v.setflags(write=False)
    return v


_P10 = np.array([float("1e%d" % k) for k in range(309)])      # correctly rounded, as the formatter's table


def _scale10(a, p):
    """a x 10^p in float64 the way the formatter scales (one rounding for |p| <= 22, a few ulp beyond)."""
    with np.errstate(all="ignore"):
        up = np.where(p > 300, a * _P10[300] * _P10[np.clip(p - 300, 0, 308)], a * _P10[np.clip(p, 0, 300)])
    return np.where(p >= 0, up, a / _P10[np.clip(-p, 0, 308)])


def far_and_near_half(v):
    """How many of the float64 values `v` take the formatter's far-exponent route (|p| > 22, p = 3 - floor(log10 |v|)) AND scale to
    within 1e-6 of the half-way point N + 0.5: the values whose rounding only the exact big-integer comparison decides.  (The scaled
    value carries a few ulp of 1e4, ~1e-11, so the count takes 5e-7 to stay inside the formatter's own 1e-6.)"""
    a = np.abs(np.asarray(v, np.float64))
    a = a[a > 0]
    e10 = np.floor(np.log10(a)).astype(np.int64)
    for _ in range(2):      # log10 may be one off at a power of ten
        s = _scale10(a, 3 - e10)
        e10 = e10 - (s < 1000.0) + (s >= 10000.0)
    p = 3 - e10
    s = _scale10(a, p)
    return int(np.count_nonzero((np.abs(p) > 22) & (np.abs(s - (np.floor(s) + 0.5)) <= 5e-7)))


def g4_rows(vals):
    """CPython's '%.4g' of each value, as the text of table rows 'c 0 1 + 0 <value>' (what the formatters write for one class,
    chromosome 'c', start 0, end 1, strand '+', label 0)."""
    head = "c\t0\t1\t+\t0\t"
    return "".join([head + "%.4g\n" % x for x in np.asarray(vals, np.float64).tolist()]).encode()


def assert_same_rows(got, want, vals, what):
    """got == want, reported by the first rows that differ (a plain comparison first: an `assert` on the texts themselves would have
    pytest diff megabytes)."""
    if got != want:
        raise AssertionError("%s: %d rows, first differences (value, got, wanted): %r"
                             % (what, len(vals), first_differences(got, want, vals)))


def first_differences(got, want, vals, limit=5):
    """The first `limit` rows at which two row texts differ: (value as a hex float, got, wanted)."""
    g, w = got.split(b"\n"), want.split(b"\n")
    out = []
    for i, v in enumerate(np.asarray(vals, np.float64).tolist()):
        a = g[i] if i < len(g) else None
        if a != w[i]:
            out.append((v.hex(), a, w[i]))
            if len(out) == limit:
                break
    return out
