"""The training / validation split by segment (``batching.split_segments``, what ``EpochLoader.split`` divides its groups by) and
``epoch_order`` over a subset of the segments.  Index logic only: no GPU."""
import numpy as np
import pytest
import torch

from mural_amd.data.batching import epoch_order, segment_rows, split_segments
from tests import _util as U
from tests.test_epoch_order_host import CASES

# (n_segments, valid_ratio, split_seed); the first is the smallest split there is: one segment on each side
TRIPLES = [(2, 0.5, 0), (12, 0.2, 5), (37, 0.1, 123)]


@pytest.mark.parametrize("n_segments,ratio,seed", TRIPLES)
def test_split_is_random_split_over_segment_numbers(n_segments, ratio, seed):
    n_valid = int(n_segments * ratio)
    a, b = torch.utils.data.random_split(range(n_segments), [n_segments - n_valid, n_valid], torch.Generator().manual_seed(seed))
    train, valid = split_segments(n_segments, ratio, seed)
    assert train == list(a.indices)                      # the order the split gave them
    assert valid == sorted(b.indices) and len(valid) == n_valid
    assert sorted(train + valid) == list(range(n_segments))
    assert all(type(i) is int for i in train + valid)
    assert split_segments(n_segments, ratio, seed) == (train, valid)
    if n_segments > 2:
        assert split_segments(n_segments, ratio, seed + 1) != (train, valid)


def test_smallest_split_has_one_validation_segment():
    train, valid = split_segments(*TRIPLES[0])
    assert len(valid) == 1 and len(train) == 1


@pytest.mark.parametrize("n_segments,ratio", [(12, 0.0), (12, 0.05), (12, 1.0), (1, 0.5), (3, 1.5), (0, 0.5)])
def test_degenerate_ratios_raise(n_segments, ratio):
    assert not 1 <= int(n_segments * ratio) < n_segments          # (the case is one: no validation segment, or no training segment)
    with pytest.raises(ValueError, match="at least one segment"):
        split_segments(n_segments, ratio, 1)


@pytest.mark.parametrize("n_segments,ratio,seed", TRIPLES)
def test_the_views_rows_partition_the_table(n_segments, ratio, seed):
    sizes = np.random.default_rng(seed).integers(1, 40, size=n_segments)
    train, valid = split_segments(n_segments, ratio, seed)
    starts = np.r_[0, np.cumsum(sizes)]
    rt, rv = segment_rows(sizes, train), segment_rows(sizes, valid)
    assert rt.dtype == np.int64 and len(rt) == sizes[train].sum() and len(rv) == sizes[valid].sum()
    assert np.array_equal(np.sort(np.r_[rt, rv]), np.arange(sizes.sum()))
    for g in valid:                                      # a view's rows are exactly the rows of its segments
        assert set(range(starts[g], starts[g + 1])) <= set(rv.tolist())
    assert np.array_equal(rv, np.sort(rv))               # validation segments ascending: the rows in table order
    # an epoch of each view yields exactly its rows, whatever the shuffle; the unshuffled validation epoch yields them in table order
    for groups, rows in ((train, rt), (valid, rv)):
        for shuffle in (False, True):
            order, bounds = epoch_order(sizes, 3, 16, shuffle=shuffle, generator=torch.Generator().manual_seed(9), groups=groups)
            assert np.array_equal(np.sort(order.numpy()), np.sort(rows)) and int(bounds[-1]) == len(rows)
    assert np.array_equal(epoch_order(sizes, 3, 16, shuffle=False, groups=valid)[0].numpy(), rv)


@pytest.mark.parametrize("case", ["a", "b", "c", "d"])
def test_epoch_order_without_groups_is_unchanged_on_the_golden_cases(case):
    fx = U.load("batching.npz")
    bs, nseg = [int(v) for v in fx[f"{case}_bs_nseg"]]
    sizes = fx[f"{case}_sizes"].tolist()
    order, bounds = epoch_order(sizes, nseg, bs, shuffle=False)
    assert order.tolist() == fx[f"{case}_rows"].tolist()
    assert np.diff(bounds.numpy()).tolist() == fx[f"{case}_cuts"].tolist()
    # every segment named in table order is the same epoch, draw for draw
    for shuffle in (False, True):
        a = epoch_order(sizes, nseg, bs, shuffle=shuffle, generator=torch.Generator().manual_seed(3))
        b = epoch_order(sizes, nseg, bs, shuffle=shuffle, generator=torch.Generator().manual_seed(3), groups=range(len(sizes)))
        assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])


@pytest.mark.parametrize("group_sizes,batch_segment,batch_size", [c for c in CASES if len(c[0]) >= 2])
def test_epoch_order_over_a_subset_is_the_epoch_of_those_segments_alone(group_sizes, batch_segment, batch_size):
    """A subset in any order: the epoch of a table that holds only those segments (the argument omitted: today's path), its row
    numbers mapped back to the whole table."""
    groups = torch.randperm(len(group_sizes), generator=torch.Generator().manual_seed(1))[:max(len(group_sizes) - 1, 1)].tolist()
    rows = segment_rows(group_sizes, groups)
    for shuffle in (False, True):
        sub = epoch_order([group_sizes[g] for g in groups], batch_segment, batch_size, shuffle=shuffle, generator=torch.Generator().manual_seed(4))
        got = epoch_order(group_sizes, batch_segment, batch_size, shuffle=shuffle, generator=torch.Generator().manual_seed(4), groups=groups)
        assert got[0].dtype == torch.int64 and np.array_equal(got[0].numpy(), rows[sub[0].numpy()]) and torch.equal(got[1], sub[1])


def test_epoch_order_refuses_bad_groups():
    for bad in ([0, 0], [3], [-1]):
        with pytest.raises(ValueError, match="groups"):
            epoch_order([4, 4, 4], 2, 4, groups=bad)
