"""The two tolerance rules of the per-op parity tests (tests/test_gpu_train_ops.py, tests/test_gpu_first_layer.py) and the table of worst
cases they print.  Tolerances are derived, never tuned:
  * float32 sums of n terms may differ from float64 by 2 (n + 2) 2^-24 sum|a_k b_k| per output element: the forward error bound of
    any summation order, doubled for fma / non-fma products and the final rounding (``_sum_check``);
  * a chain with expf / logf / rsqrt in it may be 8 times as far from float64 as torch's own float32 CPU result on the same inputs, at
    least 4 ulp of the output's largest magnitude (``_loose``).  The measured quantity is the reference, never the kernel."""
import math

import numpy as np
import torch

U24 = 2.0 ** -24
NAN = float("nan")
EPS, MOMENTUM = 1e-5, 0.1


class _Stats:
    """worst case (kernel error / bound) per checked output, printed at the end of a test"""

    def __init__(self, test, tag="train_ops"):
        self.test, self.tag, self.rows = test, tag, {}

    def add(self, what, ref_err, err, bound, case):
        ratio = err / bound if bound > 0 else (0.0 if err == 0 else math.inf)
        old = self.rows.get(what)
        if old is None or ratio >= old[0]:
            self.rows[what] = (ratio, ref_err, err, bound, case)

    def show(self):
        for what, (ratio, ref_err, err, bound, case) in self.rows.items():
            ref = "      n/a" if ref_err is None else f"{ref_err:9.3e}"
            print(f"[{self.tag}] {self.test:12s} {what:18s} torch-f32 err {ref}  kernel err {err:9.3e}  bound {bound:9.3e}  at {case}")


def _ulp4(want):
    return 4.0 * float(np.spacing(np.float32(float(want.abs().max()))))


def _loose(got, want64, ref32, what, case, stats, other=None):
    """got within 8 x (torch float32's distance from float64), at least 4 ulp, of float64; or, with ``other``, of that second result"""
    ref_err = float((ref32.detach().double() - want64).abs().max())
    err = float((got.detach().double().cpu() - (want64 if other is None else other.detach().double().cpu())).abs().max())
    bound = max(8.0 * ref_err, _ulp4(want64))
    stats.add(what, ref_err, err, bound, case)
    assert err <= bound, f"{what} at {case}: kernel is {err:.3e} from {'float64' if other is None else 'its other result'}, " \
                         f"allowed {bound:.3e} (torch float32: {ref_err:.3e})"


def _sum_check(got, want64, S, n, what, case, stats):
    """|got - want| <= 2 (n + 2) 2^-24 S element by element; n: number of terms (a number or a tensor shaped like want)"""
    bound = 2.0 * (torch.as_tensor(n, dtype=torch.float64) + 2.0) * U24 * S
    err = (got.detach().double().cpu() - want64).abs()
    bound = bound.expand_as(err)
    ok = err <= bound                                    # (a NaN is not ok)
    ratio = torch.where(bound > 0, err / bound, torch.where(err == 0, 0.0, math.inf))      # (reported: the element nearest its bound)
    worst = int(torch.argmax(torch.nan_to_num(ratio, nan=math.inf).flatten()))
    e, b = float(err.flatten()[worst]), float(bound.flatten()[worst])
    stats.add(what, None, e, b, case)
    assert bool(ok.all()), f"{what} at {case}: {int((~ok).sum())} of {err.numel()} elements beyond the summation bound, worst {e:.3e} > {b:.3e}"
