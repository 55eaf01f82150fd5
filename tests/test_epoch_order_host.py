"""``batching.epoch_order`` against ``generate_data_batches`` itself: the batching runs over a fake segment loader whose "tensors" are
the row numbers, so the concatenation of its batches IS the epoch's row order.  No GPU."""
import pytest
import torch

from mural_amd.data.batching import epoch_order, generate_data_batches


def _fake_segments(group_sizes):
    """Segments shaped like the reference's DataLoader output (leading dim 1) whose y / cat_x / distal_x all hold the row numbers."""
    row = 0
    for n in group_sizes:
        rows = torch.arange(row, row + n, dtype=torch.int64)
        row += n
        yield rows.reshape(1, n, 1), torch.zeros((1, n, 1), dtype=torch.float64), rows.reshape(1, n, 1), rows.reshape(1, n, 1)


def _reference(group_sizes, batch_segment, batch_size, shuffle, generator):
    order, bounds = [], [0]
    for y, cont, cat, dist in generate_data_batches(_fake_segments(group_sizes), batch_segment, batch_size, shuffle=shuffle, generator=generator):
        assert torch.equal(y, cat) and torch.equal(y, dist) and cont.shape == (y.shape[0], 1)
        order.append(y.reshape(-1))
        bounds.append(bounds[-1] + y.shape[0])
    return (torch.cat(order) if order else torch.zeros(0, dtype=torch.int64)), bounds


CASES = [
    # (group_sizes, batch_segment, batch_size)
    ([3, 2, 4, 1, 5], 2, 7),             # groups smaller than a batch; tails carried across consecutive groups
    ([3, 3, 3, 3, 3, 3], 1, 7),          # a tail carried across two consecutive groups that emit nothing themselves (3, 6, then 9 rows)
    ([5, 6, 4, 9, 2], 2, 4),             # tails of 3, then of (3 + 13) % 4 = 0, then the last group
    ([8, 8, 4], 2, 8),                   # a group of exactly 2 * batch_size rows: no carry
    ([12], 1, 4),                        # one single group, exact
    ([13], 3, 5),                        # one single group, short last batch
    ([4, 4, 1], 1, 4),                   # a final batch of one row
    ([6, 3], 1, 4),                      # the tail of the first group reshuffled with the last group; final batch of one row
    ([], 2, 7),                          # an empty BED
    ([0, 5, 0, 3], 2, 3),                # empty segments never come out of bed_order, but cost nothing to allow
    ([17, 1, 1, 30, 2, 9, 11], 3, 10),
    ([2, 2], 5, 100),                    # everything smaller than one batch
]


@pytest.mark.parametrize("shuffle", [False, True])
@pytest.mark.parametrize("group_sizes,batch_segment,batch_size", CASES)
def test_epoch_order_reproduces_generate_data_batches(group_sizes, batch_segment, batch_size, shuffle):
    g_ref, g_new = torch.Generator().manual_seed(20240), torch.Generator().manual_seed(20240)
    want_order, want_bounds = _reference(group_sizes, batch_segment, batch_size, shuffle, g_ref)
    order, bounds = epoch_order(group_sizes, batch_segment, batch_size, shuffle=shuffle, generator=g_new)
    n = sum(group_sizes)
    assert order.dtype == torch.int64 and bounds.dtype == torch.int64
    assert torch.equal(order, want_order)
    assert bounds.tolist() == want_bounds
    # coverage: every row once
    assert torch.equal(torch.sort(order).values, torch.arange(n, dtype=torch.int64))
    # both sides consumed the generator alike: the next draw agrees (unshuffled, nothing was drawn at all)
    if not shuffle:
        assert g_new.get_state().equal(torch.Generator().manual_seed(20240).get_state())
    assert torch.equal(torch.randint(0, 2 ** 40, (4,), generator=g_ref), torch.randint(0, 2 ** 40, (4,), generator=g_new))


def test_epoch_order_shuffles_and_depends_on_the_seed():
    sizes = [17, 1, 1, 30, 2, 9, 11]
    a, _ = epoch_order(sizes, 3, 10, generator=torch.Generator().manual_seed(1))
    b, _ = epoch_order(sizes, 3, 10, generator=torch.Generator().manual_seed(1))
    c, bc = epoch_order(sizes, 3, 10, generator=torch.Generator().manual_seed(2))
    plain, bp = epoch_order(sizes, 3, 10, shuffle=False)
    assert torch.equal(a, b) and not torch.equal(a, c) and not torch.equal(a, plain)
    assert torch.equal(plain, torch.arange(sum(sizes)))      # unshuffled, a carried tail goes first in its next group: still in order
    assert torch.equal(bc, bp)                               # the batch boundaries do not depend on the shuffle


def test_epoch_order_refuses_bad_arguments():
    for bad in (([3, -1], 2, 4), ([3], 0, 4), ([3], 1, 0)):
        with pytest.raises(ValueError):
            epoch_order(*bad)
