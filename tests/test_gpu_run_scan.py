"""The one-workgroup run scan that the table kernels share (csrc/common.h: run_excl_scan; the scan kernels of simulate.hip,
summary_conseq.hip, summary_annot.hip, sites.hip, tsv.hip and tables.hip are wrappers around it) on its own, through
mural_debug_run_scan, against numpy.cumsum.  A thread owns a run of ceil(m / T) elements: from m = T + 1 on the last threads own a
short run and empty runs (m = 3 T + 7: runs of 4, the last busy thread has 3 elements and a quarter of the threads have none)."""
import numpy as np
import pytest
import torch

from mural_amd import _lib

pytestmark = pytest.mark.gpu

_GUARD = -7      # the words between the scanned ones (stride > 1) and behind them


def _sizes(T):
    return [0, 1, 63, 64, 65, T - 1, T, T + 1, 3 * T + 7]


def _scan(values, T, stride):
    """(exclusive prefix as the hook leaves it, total, the untouched words) of `values` laid out with `stride`"""
    m = values.shape[0]
    host = np.full(m * stride + 5, _GUARD, np.int64)
    host[:m * stride:stride] = values
    v = torch.from_numpy(host).cuda()
    total = torch.full((1,), _GUARD, dtype=torch.int64, device="cuda")
    _lib.check(_lib.lib().mural_debug_run_scan(v.data_ptr(), m, stride, T, total.data_ptr(), _lib.current_stream_ptr(v.device)))
    got = v.cpu().numpy()
    rest = np.delete(got, np.arange(0, m * stride, stride))
    return got[:m * stride:stride], int(total.item()), rest


def _check(values, T, stride):
    got, total, rest = _scan(values, T, stride)
    incl = np.cumsum(values, dtype=np.int64)
    assert np.array_equal(got, incl - values)
    assert total == (int(incl[-1]) if values.shape[0] else 0)
    assert (rest == _GUARD).all()


@pytest.mark.parametrize("stride", [1, 3])
@pytest.mark.parametrize("T,m", [(T, m) for T in (256, 1024) for m in _sizes(T)])
def test_run_scan_equals_cumsum(T, m, stride):
    rng = np.random.default_rng(1000 * T + m)
    _check(rng.integers(0, 1 << 40, size=m, dtype=np.int64), T, stride)


@pytest.mark.parametrize("T", [256, 1024])
def test_run_scan_of_equal_values(T):
    _check(np.full(3 * T + 7, (1 << 40) - 1, np.int64), T, 1)


def test_run_scan_refuses_other_thread_counts():
    v = torch.zeros(8, dtype=torch.int64, device="cuda")
    st = _lib.current_stream_ptr(v.device)
    assert _lib.lib().mural_debug_run_scan(v.data_ptr(), 4, 1, 512, v.data_ptr() + 32, st) != 0
    assert _lib.lib().mural_debug_run_scan(v.data_ptr(), 4, 0, 256, v.data_ptr() + 32, st) != 0
    assert not v.any()
