"""Annotation tables on the device (csrc/summary_annot.hip: mural_summary_annot_rows; mural_amd.predict.SummarySink(annotations=...);
mural_amd.tables.annotation_table): every case goes through the entry point and is compared bit for bit with the numpy twin
``summary_annot_host`` -- piece ends on and around the tile boundaries, runs of equal starts, nested names, the class counts, both
probability types and the three label kinds, the status bits, additivity over calls and chromosomes, the limb edge past the slice bound,
more pieces than one piece launch takes, and the table route against the in-flight sink."""
import ctypes as C
import itertools

import numpy as np
import pytest
import torch

from tests import _annot_data as D

pytestmark = pytest.mark.gpu

LABEL_DTYPES = {0: np.float32, 1: np.int32, 2: np.int64}


def _dev():
    return torch.device("cuda", torch.cuda.current_device())


def _lib():
    from mural_amd import _lib
    return _lib


def _tile():
    return int(_lib().lib().mural_summary_annot_tile_rows())


def _up(a):
    return a if isinstance(a, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(a)).to(_dev())


def _kernel(prob, start, label, n_class, pieces, n_groups, into=None, pad=0):
    """One mural_summary_annot_rows call on device copies of the arrays (or on device tensors): (table tensor int64
    [n_groups * 3 * n_class], status).  `pad`: extra columns behind the probabilities (a padded stride)."""
    L = _lib()
    lib, dev = L.lib(), _dev()
    if pad and not isinstance(prob, torch.Tensor):
        prob = np.concatenate([prob, np.full((len(prob), pad), 0.25, prob.dtype)], axis=1)
    prob_d, start_d, label_d = _up(prob), _up(start), _up(label)
    b0, b1, grp = (_up(np.asarray(x, dt)) for x, dt in zip(pieces, (np.int64, np.int64, np.int32)))
    n = int(start_d.shape[0])
    table = torch.zeros(max(n_groups, 1) * 3 * n_class, dtype=torch.int64, device=dev) if into is None else into
    status = torch.zeros(1, dtype=torch.int32, device=dev)
    need = int(lib.mural_summary_annot_workspace_bytes(n, n_class))
    ws = torch.empty(need // 8 + 1, dtype=torch.int64, device=dev)
    s = L.MuralSummaryAnnotRows()
    s.prob, s.prob_f64, s.prob_stride = prob_d.data_ptr(), int(prob_d.dtype == torch.float64), prob_d.stride(0) if n else n_class
    s.start, s.label = start_d.data_ptr(), label_d.data_ptr()
    s.label_kind = {torch.float32: 0, torch.int32: 1, torch.int64: 2}[label_d.dtype]
    s.n, s.n_class, s.n_groups = n, n_class, n_groups
    s.piece_b0, s.piece_b1, s.piece_group, s.n_pieces = b0.data_ptr(), b1.data_ptr(), grp.data_ptr(), int(b0.shape[0])
    s.table, s.status = table.data_ptr(), status.data_ptr()
    L.check(lib.mural_summary_annot_rows(C.byref(s), ws.data_ptr(), ws.numel() * 8, L.current_stream_ptr(dev)))
    return table, int(status.item())


def _host(table, n_groups, n_class):
    return table.cpu().numpy().view(np.uint64)[:n_groups * 3 * n_class].reshape(n_groups, 3, n_class)


def _twin(prob, start, label, n_class, pieces, n_groups, into=None):
    from mural_amd.predict import summary_annot_host
    return summary_annot_host(prob, start, label, n_class, pieces, n_groups, into=into)


def _rows(n, n_class, dtype, label_kind, seed=0):
    rng = np.random.default_rng(seed)
    prob = rng.dirichlet(np.ones(n_class), size=n).astype(dtype)
    return prob, rng.integers(0, n_class, size=n).astype(LABEL_DTYPES[label_kind])


def _all_pairs(ends):
    """Every [a, b) of the sorted positions as a piece of its own group: the pieces nest and overlap in every way."""
    pairs = list(itertools.combinations(sorted(set(ends)), 2))
    return (np.array([a for a, _ in pairs], np.int64), np.array([b for _, b in pairs], np.int64), np.arange(len(pairs), dtype=np.int32)), len(pairs)


# ---- 1. the kernel against the twin around the tile boundaries ---------------------------------------------------------------------------
def test_the_tile_is_a_wave_and_the_workspace_is_the_tile_prefixes():
    lib = _lib().lib()
    T = _tile()
    assert T == 64 and int(lib.mural_summary_annot_slice_rows()) == 1 << 23
    assert int(lib.mural_summary_annot_workspace_bytes(5_000_000, 4)) == (-(-5_000_000 // T) + 1) * 12 * 8     # 7.5 MB
    assert int(lib.mural_summary_annot_workspace_bytes(1 << 30, 8)) == ((1 << 23) // T + 1) * 24 * 8            # a slice's, whatever n


@pytest.mark.parametrize("n_class,dtype,label_kind,pad", [(2, np.float32, 0, 3), (4, np.float64, 1, 0), (8, np.float32, 2, 1)])
@pytest.mark.parametrize("which", range(5))
def test_kernel_equals_the_twin_for_piece_ends_on_and_around_every_tile_boundary(which, n_class, dtype, label_kind, pad):
    """Rows at start = 3 i + 5; piece ends at rows 0, T - 1, T, T + 1, the multiples of T, n - 1, n and past n -- on the row's start, one
    below and one above it (between two rows: [3 i + 6, 3 i + 7) is an empty piece) --, every pair of them a piece of its own name."""
    T = _tile()
    n = [1, T - 1, T, T + 1, 3 * T + 5][which]
    prob, label = _rows(n, n_class, dtype, label_kind, seed=which)
    start = 3 * np.arange(n, dtype=np.int64) + 5
    at = [i for i in (0, 1, T - 1, T, T + 1, 2 * T, 3 * T, n - 1, n, n + 7) if i <= n + 7]
    pieces, n_groups = _all_pairs([0] + [3 * i + 5 + d for i in at for d in (-1, 0, 1, 2)])
    got, status = _kernel(prob, start, label, n_class, pieces, n_groups, pad=pad)
    want, _ = _twin(prob, start, label, n_class, pieces, n_groups)
    assert status == 0 and want[:, 0].sum() > 0
    assert np.array_equal(_host(got, n_groups, n_class), want)
    empty = [g for g, (a, b) in enumerate(zip(*pieces[:2])) if b - a == 1 and (a - 5) % 3 != 0]
    assert empty and not want[empty].any()


def test_runs_of_equal_starts_straddle_the_tile_boundaries():
    """An INDEL table holds equal starts: runs over rows T - 3 .. T + 2 and 2 T - 1 .. 2 T, piece ends on those values."""
    T = _tile()
    n = 3 * T + 5
    prob, label = _rows(n, 4, np.float64, 2, seed=9)
    start = 2 * np.arange(n, dtype=np.int64)
    start[T - 3:T + 3] = start[T - 3]
    start[2 * T - 1:2 * T + 1] = start[2 * T - 1]
    v, w = int(start[T]), int(start[2 * T])
    pieces, n_groups = _all_pairs([0, v - 1, v, v + 1, w - 1, w, w + 1, int(start[-1]), int(start[-1]) + 1])
    got, status = _kernel(prob, start, label, 4, pieces, n_groups)
    want, _ = _twin(prob, start, label, 4, pieces, n_groups)
    assert status == 0 and np.array_equal(_host(got, n_groups, 4), want)
    j = [g for g, (a, b) in enumerate(zip(*pieces[:2])) if (a, b) == (v, v + 1)][0]
    assert int(want[j, 0].sum()) == 6                          # the whole run, on both sides of the boundary


def test_two_names_whose_pieces_nest_and_the_literal_bed():
    from mural_amd.tables import read_annotations
    names, _, pieces = read_annotations(D.intervals_dict())
    table, want = None, None
    per_chrom = {"chrA": D.rows(300, 4, 0, dtype=np.float32), "chrB": D.rows(40, 4, 1, lo=0, hi=70, hole=(62, 64), dtype=np.float32)}
    for chrom, (prob, start, label) in per_chrom.items():      # two chromosomes' piece lists into one table
        table, status = _kernel(prob, start, label, 4, pieces[chrom], len(names), into=table)
        assert status == 0
        want, _ = _twin(prob, start, label, 4, pieces[chrom], len(names), into=want)
    got = _host(table, len(names), 4)
    assert np.array_equal(got, want) and D.as_integers(got) == D.oracle(per_chrom, 4, names)
    inner, outer = got[names.index("inner")], got[names.index("outer")]
    assert 0 < inner[0].sum() < outer[0].sum()


# ---- 2. status ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("what,bit", [("nan", 8), ("above", 8), ("label", 2)])
def test_bad_rows_inside_a_piece_are_skipped_and_set_status(what, bit):
    T = _tile()
    n = 2 * T + 9
    prob, label = _rows(n, 4, np.float32, 1, seed=4)
    start = np.arange(n, dtype=np.int64)
    at = T + 2
    if what == "nan":
        prob[at, 1] = np.nan
    elif what == "above":
        prob[at, 2] = 1.5
    else:
        label[at] = 4
    pieces = (np.array([0, T - 5]), np.array([n, T + 5]), np.array([0, 1]))
    got, status = _kernel(prob, start, label, 4, pieces, 2)
    want, want_status = _twin(prob, start, label, 4, pieces, 2)
    assert status == bit == want_status
    assert np.array_equal(_host(got, 2, 4), want) and int(want[0, 0].sum()) == n - 1 and int(want[1, 0].sum()) == 9


def test_a_descending_pair_sets_status_4():
    T = _tile()
    n = T + 10
    prob, label = _rows(n, 2, np.float32, 2)
    start = np.arange(n, dtype=np.int64)
    start[T], start[T - 1] = start[T - 1], start[T]            # across the tile boundary
    _, status = _kernel(prob, start, label, 2, (np.array([0]), np.array([n]), np.array([0])), 1)
    assert status == 4
    start = np.sort(start)
    start[5] = start[4]                                        # equal starts are legal
    _, status = _kernel(prob, start, label, 2, (np.array([0]), np.array([n]), np.array([0])), 1)
    assert status == 0


def test_no_rows_or_no_pieces_leave_the_table_untouched():
    prob, label = _rows(10, 2, np.float32, 2)
    start = np.arange(10, dtype=np.int64)
    table = torch.full((3 * 3 * 2,), 7, dtype=torch.int64, device=_dev())
    none = (np.zeros(0, np.int64), np.zeros(0, np.int64), np.zeros(0, np.int32))
    _, status = _kernel(prob, start, label, 2, none, 3, into=table)
    assert status == 0 and (table == 7).all()
    _, status = _kernel(prob[:0], start[:0], label[:0], 2, (np.array([0]), np.array([5]), np.array([1])), 3, into=table)
    assert status == 0 and (table == 7).all()


# ---- 3. additivity --------------------------------------------------------------------------------------------------------------------------
def test_one_two_and_seven_consecutive_calls_give_identical_tables():
    T = _tile()
    n = 5 * T + 11
    prob, label = _rows(n, 4, np.float32, 0, seed=2)
    start = np.sort(np.random.default_rng(2).integers(0, 2 * n, size=n)).astype(np.int64)      # with equal starts
    pieces, n_groups = _all_pairs(np.random.default_rng(3).integers(0, 2 * n + 5, size=24).tolist())
    want, _ = _twin(prob, start, label, 4, pieces, n_groups)
    for parts in (1, 2, 7):
        table = None
        for rows in np.array_split(np.arange(n), parts):
            table, status = _kernel(prob[rows], start[rows], label[rows], 4, pieces, n_groups, into=table)
            assert status == 0
        assert np.array_equal(_host(table, n_groups, 4), want), parts


def _shards(per_chrom, parts, device):
    for chrom, (prob, start, label) in per_chrom.items():
        for rows in np.array_split(np.arange(len(start)), parts):
            cols = {"start": start[rows], "end": start[rows] + 1, "strand": np.zeros(len(rows), np.uint8), "label": label[rows].astype(np.float32),
                    "prob": prob[rows]}
            if device:
                cols = {key: _up(v) for key, v in cols.items()}
            yield dict(cols, chrom=chrom, n_class=4, calibrated=False, aligned=True)


def _per_chrom():
    return {"chrA": D.rows(1200, 4, 0, dtype=np.float32), "chrB": D.rows(800, 4, 1, lo=0, hi=70, hole=(62, 64), dtype=np.float32)}


def test_sink_fed_device_shards_equals_one_fed_the_same_shards_on_the_host(tmp_path):
    from mural_amd.predict import SummarySink
    sinks = []
    for device in (True, False):
        sink = SummarySink(str(tmp_path / ("d" if device else "h")), annotations=D.intervals_dict())
        for shard in _shards(_per_chrom(), 3, device):
            sink(shard)
        sink.close()
        sinks.append(sink)
    assert sinks[0].annotation_sums().tobytes() == sinks[1].annotation_sums().tobytes()
    assert D.as_integers(sinks[0].annotation_sums()) == D.oracle(_per_chrom(), 4, D.NAMES)
    assert (tmp_path / "d.annotation.mut_rates.tsv").read_text() == (tmp_path / "h.annotation.mut_rates.tsv").read_text()
    assert (tmp_path / "d.annotation.corr.txt").read_text() == (tmp_path / "h.annotation.corr.txt").read_text()


# ---- 4. the launch bounds -------------------------------------------------------------------------------------------------------------------
def test_limb_edge_past_the_slice_bound():
    """n = 2^23 + T + 3 rows of (2^40 - 1) * 2^-71 in both classes: hi = 0 and lo = 2^40 - 1 in every row, so the unfolded lo prefix of a
    slice reaches 2^23 (2^40 - 1), just below 2^63.  The launch bound crossed is the slice of mural_summary_annot_slice_rows() = 2^23 rows
    (the entry loops over slices; no grid of it is capped: the tile grid of a slice is 2^15 workgroups): the second slice holds one whole
    tile and a partial one.  Expected cells in closed form: rows * (2^40 - 1) as a Python integer split into limbs."""
    T = _tile()
    S = int(_lib().lib().mural_summary_annot_slice_rows())
    n = S + T + 3
    dev = _dev()
    q = (1 << 40) - 1
    prob = torch.full((n, 2), float(q) * 2.0 ** -71, dtype=torch.float64, device=dev)
    start = torch.arange(n, dtype=torch.int64, device=dev)
    label = torch.zeros(n, dtype=torch.int32, device=dev)
    pieces = (np.array([0, n - 5, S - 10]), np.array([n, n, S + 10]), np.array([0, 1, 2]))      # all rows | the last 5 | across the bound
    got, status = _kernel(prob, start, label, 2, pieces, 3)
    assert status == 0
    got = _host(got, 3, 2).tolist()
    for g, rows in enumerate((n, 5, 20)):
        total = rows * q
        assert got[g] == [[rows, 0], [total >> 40] * 2, [total & q] * 2], g


def test_more_pieces_than_one_fold_of_the_table():
    """2^20 + 3 pieces over 130 rows, into two groups: more than the mural_summary_annot_fold_pieces() pieces of one piece launch, so the
    entry's loop over piece ranges runs twice and the second launch's range [p0, p1) is checked.  A launch-bound test only: these sums
    stay far below 2^64 with or without the fold between the two launches, so it does not show that the fold is needed."""
    P = int(_lib().lib().mural_summary_annot_fold_pieces()) + 3
    assert P == (1 << 20) + 3
    n = 130
    prob, label = _rows(n, 2, np.float64, 1, seed=6)
    prob[:, 0] = float((1 << 40) - 1) * 2.0 ** -71
    start = np.arange(n, dtype=np.int64)
    b0 = np.arange(P, dtype=np.int64) % 7
    pieces = (b0, b0 + 100 + np.arange(P) % 50, (np.arange(P) % 2).astype(np.int32))
    got, status = _kernel(prob, start, label, 2, pieces, 2)
    want, _ = _twin(prob, start, label, 2, pieces, 2)
    assert status == 0 and np.array_equal(_host(got, 2, 2), want)
    assert int(want[:, 0].sum()) == int((np.minimum(pieces[1], n) - b0).sum())


# ---- 5. the table route ---------------------------------------------------------------------------------------------------------------------
def test_annotation_table_on_the_written_table_equals_the_in_flight_sink(tmp_path):
    """2 000 rows on two chromosomes written by TsvSink; ``tables.annotation_table`` on the file through the same entry: names and counts
    identical to the in-flight sink's, the sums within the four digits the table prints."""
    from mural_amd import tables
    from mural_amd.predict import SummarySink, TsvSink
    annot = tables.read_annotations(D.intervals_dict())
    out = str(tmp_path / "t.tsv")
    tsv, sink = TsvSink(out), SummarySink(None, annotations=annot)
    for shard in _shards(_per_chrom(), 1, True):
        tsv(dict(shard))
        sink(dict(shard))
    tsv.close()
    sink.close()
    names, meta, table = tables.annotation_table(out, annot, 4, chunk_bytes=16 << 10)      # several chunks
    want_names, want_meta, want = sink.result()["annotations"]
    assert names == want_names and np.array_equal(meta, want_meta)
    assert np.array_equal(table[:, :5], want[:, :5]) and want[:, 0].sum() > 2000
    assert (np.abs(table[:, 5:] - want[:, 5:]) <= 5e-4 * want[:, 5:]).all()

    class Args:
        pred_file, annotations, n_class, out_prefix = out, annot, 4, str(tmp_path / "calc")
    tables.run_annotation_calc(Args)
    lines = (tmp_path / "calc.annotation.mut_rates.tsv").read_text().splitlines()
    assert [ln.split("\t")[0] for ln in lines[1:]] == names and (tmp_path / "calc.annotation.corr.txt").exists()
