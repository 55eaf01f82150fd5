"""Mutation sets drawn from the rates on the device (csrc/simulate.hip: mural_simulate_annot_rows, mural_simulate_rows;
mural_amd.predict.SummarySink(simulate=...); mural_amd.tables.simulate_table): every case goes through the entry points and is compared
for EQUALITY with the numpy twins ``simulate_annot_host`` / ``simulate_rows_host`` -- row counts around the wave and the chunk length,
the replicate counts around a Philox call and a block of 64, the class counts, both probability types, a padded stride, both strand
forms, empty and all-covering pieces, nesting, the three loop bounds of the entry, additivity over calls, the mutation list, and the
sink's routes: shard invariance, the table route and the round trip through ``mutations=``."""
import ctypes as C
import itertools

import numpy as np
import pytest
import torch

from tests.test_gpu_region_labels import REGIONS, Listed, _forward, files, snv_model  # noqa: F401  (fixtures)

pytestmark = pytest.mark.gpu

SEED, KEY = (1 << 63) + 0x1234567, 0x9E3779B1


def _dev():
    return torch.device("cuda", torch.cuda.current_device())


def _lib():
    from mural_amd import _lib
    return _lib


def _S():
    from mural_amd import summaries
    return summaries


def _up(a):
    return a if isinstance(a, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(a)).to(_dev())


def _chunk():
    return int(_lib().lib().mural_simulate_chunk_rows())


def _fill_rows(s, prob_d, start_d, strand_d, n_class):
    n = int(start_d.shape[0])
    s.prob, s.prob_f64, s.prob_stride, s.n_class = prob_d.data_ptr(), int(prob_d.dtype == torch.float64), prob_d.stride(0) if n else n_class, n_class
    s.start, s.strand, s.n = start_d.data_ptr(), None if strand_d is None else strand_d.data_ptr(), n
    s.chrom_key, s.seed = KEY, SEED
    return n


def _pad(prob, pad):
    return np.concatenate([prob, np.full((len(prob), pad), 0.25, prob.dtype)], axis=1) if pad else prob


def _annot(prob, start, strand, n_class, pieces, n_groups, n_rep, into=None, pad=0):
    """One mural_simulate_annot_rows call on device copies: (table tensor int32 [n_groups * (n_class - 1) * n_rep], status)."""
    L = _lib()
    lib, dev = L.lib(), _dev()
    prob_d, start_d, strand_d = _up(_pad(prob, pad)), _up(start), None if strand is None else _up(strand)
    b0, b1, grp = (_up(np.asarray(x, dt)) for x, dt in zip(pieces, (np.int64, np.int64, np.int32)))
    table = torch.zeros(max(n_groups * (n_class - 1) * n_rep, 1), dtype=torch.int32, device=dev) if into is None else into
    status = torch.zeros(1, dtype=torch.int32, device=dev)
    s = L.MuralSimulateAnnotRows()
    _fill_rows(s, prob_d, start_d, strand_d, n_class)
    s.n_rep = n_rep
    s.piece_b0, s.piece_b1, s.piece_group, s.n_pieces = b0.data_ptr(), b1.data_ptr(), grp.data_ptr(), int(b0.shape[0])
    s.n_groups, s.table, s.status = n_groups, table.data_ptr(), status.data_ptr()
    need = int(lib.mural_simulate_annot_workspace_bytes(int(b0.shape[0])))
    ws = torch.empty(need // 8 + 1, dtype=torch.int64, device=dev)
    L.check(lib.mural_simulate_annot_rows(C.byref(s), ws.data_ptr(), ws.numel() * 8, L.current_stream_ptr(dev)))
    return table, int(status.item())


def _host(table, n_groups, n_class, n_rep):
    return table.cpu().numpy().view(np.uint32)[:n_groups * (n_class - 1) * n_rep].reshape(n_groups, n_class - 1, n_rep)


def _twin(prob, start, strand, n_class, pieces, n_groups, n_rep, into=None):
    return _S().simulate_annot_host(prob, start, strand, n_class, KEY, SEED, pieces, n_groups, n_rep, into=into)


def _list(prob, start, strand, n_class, rep, pad=0):
    """One mural_simulate_rows call: (start, strand, label) of the list on the host, status."""
    L = _lib()
    lib, dev = L.lib(), _dev()
    prob_d, start_d, strand_d = _up(_pad(prob, pad)), _up(start), None if strand is None else _up(strand)
    s = L.MuralSimulateRows()
    n = _fill_rows(s, prob_d, start_d, strand_d, n_class)
    out = (torch.full((n,), -7, dtype=torch.int64, device=dev), torch.full((n,), 9, dtype=torch.uint8, device=dev),
           torch.full((n,), 9, dtype=torch.uint8, device=dev))
    count = torch.full((1,), -1, dtype=torch.int64, device=dev)
    status = torch.zeros(1, dtype=torch.int32, device=dev)
    s.replicate = rep
    s.out_start, s.out_strand, s.out_label, s.count, s.status = (out[0].data_ptr(), out[1].data_ptr(), out[2].data_ptr(), count.data_ptr(),
                                                                 status.data_ptr())
    need = int(lib.mural_simulate_rows_workspace_bytes(n))
    ws = torch.empty(need // 8 + 1, dtype=torch.int64, device=dev)
    L.check(lib.mural_simulate_rows(C.byref(s), ws.data_ptr(), ws.numel() * 8, L.current_stream_ptr(dev)))
    m = int(count.item())
    assert all((x[m:] == fill).all() for x, fill in zip(out, (-7, 9, 9)))      # nothing is written past the count
    return tuple(x[:m].cpu().numpy() for x in out), int(status.item())


def _rows(n, n_class, dtype, seed=0, scale=0.6):
    """(prob, start strictly ascending past 2^32, strand)"""
    rng = np.random.default_rng(seed)
    prob = rng.dirichlet(np.ones(n_class), size=n)
    prob[:, 1:] *= scale
    start = (np.cumsum(rng.integers(1, 4, size=n)) + (1 << 32) - n).astype(np.int64)      # the starts cross 2^32: both counter words
    return prob.astype(dtype), start, rng.integers(0, 2, size=n).astype(np.uint8)


def _all_pairs(ends):
    """Every [a, b) of the sorted positions as a piece of its own group: the pieces nest and overlap in every way."""
    pairs = list(itertools.combinations(sorted(set(int(e) for e in ends)), 2))
    return (np.array([a for a, _ in pairs], np.int64), np.array([b for _, b in pairs], np.int64), np.arange(len(pairs), dtype=np.int32)), len(pairs)


def _pieces_for(start):
    """Pieces around the first row, the wave boundaries, the chunk boundary and the last row; one covers everything, several are empty
    (before the first row, past the last, between two rows)."""
    n, T = len(start), _chunk()
    at = sorted({i for i in (0, 1, 63, 64, 65, 128, T - 1, T, n - 1) if 0 <= i < n})
    ends = [0, int(start[0]) - 5, int(start[-1]) + 1, int(start[-1]) + 9] + [int(start[i]) + d for i in at for d in (0, 1)]
    return _all_pairs(ends)


# ---- 1. the annotation table against the twin ---------------------------------------------------------------------------------------------
def test_the_exported_bounds():
    lib = _lib().lib()
    assert _chunk() == 1024 and int(lib.mural_simulate_grid_waves()) == 8192 and int(lib.mural_simulate_scan_threads()) == 1024
    assert int(lib.mural_simulate_max_replicates()) == 1 << 20 == _S().SIMULATE_MAX_REPLICATES
    assert int(lib.mural_simulate_annot_workspace_bytes(0)) == 0 and int(lib.mural_simulate_rows_workspace_bytes(0)) == 0
    assert 24 * 1000 <= int(lib.mural_simulate_annot_workspace_bytes(1000)) <= 24 * 1000 + 3 * 256 + 8
    assert 8 * 17 <= int(lib.mural_simulate_rows_workspace_bytes(1025)) <= 8 * 18 + 256


CONFIGS = [(2, np.float32, 3, "mixed", 3), (4, np.float64, 0, None, 5), (8, np.float32, 1, "mixed", 67), (4, np.float32, 0, "mixed", 4),
           (2, np.float64, 0, None, 1)]


@pytest.mark.parametrize("n_class,dtype,pad,strand_kind,n_rep", CONFIGS)
@pytest.mark.parametrize("which", range(7))
def test_table_equals_the_twin(which, n_class, dtype, pad, strand_kind, n_rep):
    n = [1, 63, 64, 65, 129, _chunk() - 1, _chunk() + 1][which]
    prob, start, strand = _rows(n, n_class, dtype, seed=which)
    strand = strand if strand_kind == "mixed" else None
    pieces, n_groups = _pieces_for(start)
    got, status = _annot(prob, start, strand, n_class, pieces, n_groups, n_rep, pad=pad)
    want, want_status = _twin(prob, start, strand, n_class, pieces, n_groups, n_rep)
    assert status == 0 == want_status and (want.sum() > 0 or n * n_rep < 8)      # (one row in one replicate may well draw 0)
    assert np.array_equal(_host(got, n_groups, n_class, n_rep), want)
    everything = [g for g, (a, b) in enumerate(zip(*pieces[:2])) if a == 0 and b == int(start[-1]) + 9][0]
    labels = _S().simulate_rows_host(prob, start, strand, n_class, KEY, SEED, np.arange(n_rep))
    assert want[everything].tolist() == [[int((labels[:, r] == c).sum()) for r in range(n_rep)] for c in range(1, n_class)]
    empty = [g for g, (a, b) in enumerate(zip(*pieces[:2])) if b <= int(start[0]) or a > int(start[-1])]
    assert empty and not want[empty].any()


@pytest.mark.parametrize("n_class", [2, 8])
def test_table_equals_the_twin_with_the_fewest_and_the_most_classes_over_two_replicate_blocks(n_class):
    """The field beside the last class's is no bin: a draw of class 0 and a lane without a row count nowhere, at 2 classes (one bound, six
    that do not exist) and at 8 (seven bounds, the last field of the word), in a full block of replicates and a block of one."""
    n, n_rep = 300, 65
    prob, start, strand = _rows(n, n_class, np.float32, seed=40 + n_class)
    ends = [0, int(start[0]), int(start[70]), int(start[200]) + 1, int(start[-1]) + 9]
    pieces, n_groups = _all_pairs(ends)
    got, status = _annot(prob, start, strand, n_class, pieces, n_groups, n_rep)
    want, want_status = _twin(prob, start, strand, n_class, pieces, n_groups, n_rep)
    assert status == 0 == want_status and want[..., 64].sum() > 0 and want.sum() < n * n_rep * n_groups      # (class 0 is drawn as well)
    assert got.cpu().numpy().tobytes() == want.astype(np.uint32).tobytes()


def test_300_nested_pieces_on_500_rows():
    prob, start, strand = _rows(500, 4, np.float32, seed=30)
    lo, hi = int(start[0]), int(start[-1]) + 1
    b0 = lo + np.arange(300, dtype=np.int64)                   # piece j lies inside piece j - 1
    b1 = hi - np.arange(300, dtype=np.int64)
    pieces = (b0, b1, (np.arange(300) % 7).astype(np.int32))   # and 7 names share them
    got, status = _annot(prob, start, strand, 4, pieces, 7, 5)
    want, _ = _twin(prob, start, strand, 4, pieces, 7, 5)
    assert status == 0 and np.array_equal(_host(got, 7, 4, 5), want) and want.min() > 0


def test_past_the_chunk_length_the_grid_and_the_scan_threads():
    """The three loop bounds of the entry.  A piece over 3 * chunk + 7 rows is cut into 4 chunks (mural_simulate_chunk_rows).  Then
    4 200 pieces of at least one row with 67 replicates -- two blocks of 64 --: 8 400 units and more, past the
    mural_simulate_grid_waves() = 8 192 waves of the draw grid, so waves take a second unit; and more pieces than the
    mural_simulate_scan_threads() = 1 024 threads of the scan, so a thread owns a run of pieces."""
    T = _chunk()
    prob, start, strand = _rows(3 * T + 7, 4, np.float32, seed=40)
    pieces = (np.array([0, int(start[5]), int(start[T])]), np.array([int(start[-1]) + 1, int(start[2 * T + 1]), int(start[T]) + 1]),
              np.array([0, 1, 2], np.int32))
    got, status = _annot(prob, start, strand, 4, pieces, 3, 6)
    want, _ = _twin(prob, start, strand, 4, pieces, 3, 6)
    assert status == 0 and np.array_equal(_host(got, 3, 4, 6), want)
    lib = _lib().lib()
    P = 4200
    assert P * 2 > int(lib.mural_simulate_grid_waves()) and P > int(lib.mural_simulate_scan_threads())
    prob, start, strand = _rows(300, 2, np.float64, seed=41, scale=0.5)
    i0 = np.arange(P) % 290
    pieces = (start[i0], start[i0 + 1 + np.arange(P) % 9] + 1, (np.arange(P) % 11).astype(np.int32))
    got, status = _annot(prob, start, strand, 2, pieces, 11, 67)
    want, _ = _twin(prob, start, strand, 2, pieces, 11, 67)
    assert status == 0 and np.array_equal(_host(got, 11, 2, 67), want) and want.min() > 0


def test_calls_accumulate_and_parts_give_the_one_call_table():
    n = 5 * 64 + 11
    prob, start, strand = _rows(n, 4, np.float32, seed=2)
    pieces, n_groups = _all_pairs(np.random.default_rng(3).choice(np.arange(start[0] - 3, start[-1] + 5), size=16, replace=False).tolist())
    want, _ = _twin(prob, start, strand, 4, pieces, n_groups, 9)
    for parts in (1, 2, 7):
        table = None
        for rows in np.array_split(np.arange(n), parts):
            table, status = _annot(prob[rows], start[rows], strand[rows], 4, pieces, n_groups, 9, into=table)
            assert status == 0
        assert np.array_equal(_host(table, n_groups, 4, 9), want), parts
    table, _ = _annot(prob, start, strand, 4, pieces, n_groups, 9, into=table)      # the same rows again: the table doubles
    assert np.array_equal(_host(table, n_groups, 4, 9), 2 * want)


@pytest.mark.parametrize("what,bit", [("nan", 8), ("negative", 8), ("inf", 8), ("order", 4), ("start", 1)])
def test_bad_rows_draw_zero_and_set_status(what, bit):
    n = 2 * 64 + 9
    prob, start, strand = _rows(n, 4, np.float32, seed=4)
    at = 64 + 2
    prob[:, 1:] = 0.3                                          # every good row draws a class >= 1 (cum reaches 0.9 .. and is hit often)
    prob[:, 3] = 0.4
    if what in ("nan", "negative", "inf"):
        prob[at, 2] = {"nan": np.nan, "negative": -0.5, "inf": np.inf}[what]
    elif what == "order":
        start[at], start[at - 1] = start[at - 1], start[at]
    else:
        start = start - start[0] - 1                           # the first start is -1
        at = 0
    pieces = (np.array([-5]), np.array([int(start.max()) + 1]), np.array([0], np.int32))
    got, status = _annot(prob, start, strand, 4, pieces, 1, 8)
    assert status == bit
    if what != "order":
        want, want_status = _twin(prob, start, strand, 4, pieces, 1, 8)
        assert want_status == bit and np.array_equal(_host(got, 1, 4, 8), want)
        assert (want.sum(axis=1) == n - 1).all()                # the bad row alone draws 0; every other row draws a class >= 1
        (_, _, label), status = _list(prob, start, strand, 4, 3)
        assert status == bit and len(label) == n - 1


def test_no_rows_no_pieces_and_a_short_workspace():
    L = _lib()
    prob, start, strand = _rows(10, 2, np.float32)
    table = torch.full((3 * 1 * 4,), 7, dtype=torch.int32, device=_dev())
    none = (np.zeros(0, np.int64), np.zeros(0, np.int64), np.zeros(0, np.int32))
    _, status = _annot(prob, start, strand, 2, none, 3, 4, into=table)
    assert status == 0 and (table == 7).all()
    _, status = _annot(prob[:0], start[:0], strand[:0], 2, (np.array([0]), np.array([5]), np.array([1])), 3, 4, into=table)
    assert status == 0 and (table == 7).all()
    # a workspace one byte short is refused before anything is launched
    lib, dev = L.lib(), _dev()
    prob_d, start_d = _up(prob), _up(start)
    b0, b1, grp = _up(np.array([0], np.int64)), _up(np.array([1 << 40], np.int64)), _up(np.array([0], np.int32))
    status = torch.zeros(1, dtype=torch.int32, device=dev)
    s = L.MuralSimulateAnnotRows()
    _fill_rows(s, prob_d, start_d, None, 2)
    s.n_rep, s.piece_b0, s.piece_b1, s.piece_group, s.n_pieces = 4, b0.data_ptr(), b1.data_ptr(), grp.data_ptr(), 1
    s.n_groups, s.table, s.status = 3, table.data_ptr(), status.data_ptr()
    need = int(lib.mural_simulate_annot_workspace_bytes(1))
    ws = torch.empty(need // 8 + 1, dtype=torch.int64, device=dev)
    assert lib.mural_simulate_annot_rows(C.byref(s), ws.data_ptr(), need - 1, L.current_stream_ptr(dev)) == 3      # MURAL_E_WORKSPACE
    m = L.MuralSimulateRows()
    _fill_rows(m, prob_d, start_d, None, 2)
    out = torch.zeros(10, dtype=torch.int64, device=dev)
    m.replicate, m.out_start, m.out_strand, m.out_label, m.count, m.status = 0, out.data_ptr(), out.data_ptr(), out.data_ptr(), out.data_ptr(), status.data_ptr()
    need = int(lib.mural_simulate_rows_workspace_bytes(10))
    assert lib.mural_simulate_rows(C.byref(m), ws.data_ptr(), need - 1, L.current_stream_ptr(dev)) == 3
    torch.cuda.synchronize()
    assert (table == 7).all() and int(status.item()) == 0 and not out.any()
    m.n = 0                                                    # n == 0 launches nothing, whatever the workspace
    assert lib.mural_simulate_rows(C.byref(m), None, 0, L.current_stream_ptr(dev)) == 0


# ---- 2. the mutation list -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n_class,dtype,pad,strand_kind,rep", [(2, np.float32, 2, "mixed", 0), (4, np.float64, 0, None, 5), (8, np.float32, 0, "mixed", 66)])
@pytest.mark.parametrize("which", range(7))
def test_list_equals_the_twin_s_non_zero_labels_in_order(which, n_class, dtype, pad, strand_kind, rep):
    n = [1, 63, 64, 65, 129, _chunk() - 1, _chunk() + 1][which]
    prob, start, strand = _rows(n, n_class, dtype, seed=10 + which)
    if n == 1:
        prob[0, 1] = 1.0
    strand = strand if strand_kind == "mixed" else None
    (got_start, got_strand, got_label), status = _list(prob, start, strand, n_class, rep, pad=pad)
    label = _S().simulate_rows_host(prob, start, strand, n_class, KEY, SEED, [rep])[:, 0]
    hit = label > 0
    assert status == 0 and hit.any()
    assert np.array_equal(got_start, start[hit]) and np.array_equal(got_label, label[hit])
    assert np.array_equal(got_strand, np.zeros(hit.sum(), np.uint8) if strand is None else strand[hit])


def test_a_part_without_a_hit_and_a_part_where_every_row_hits():
    n = 3 * 64 + 5
    prob, start, strand = _rows(n, 3, np.float32, seed=20)
    prob[:, 1:] = 0.0
    (got_start, _, _), status = _list(prob, start, strand, 3, 2)
    assert status == 0 and len(got_start) == 0
    prob[:, 1] = 1.0                                           # p_1 = 1: cum_1 = 2^32 > every u
    (got_start, got_strand, got_label), status = _list(prob, start, strand, 3, 2)
    assert status == 0 and np.array_equal(got_start, start) and np.array_equal(got_strand, strand) and (got_label == 1).all()


# ---- 3. the sink's routes -------------------------------------------------------------------------------------------------------------------
ANNOT = {"chrA": [(0, 1000, "a"), (500, 3000, "b"), (600, 700, "a"), (2400, 2500, "c"), (2500, 2950, "gap"), (4000, 6000, "tail")],
         "chrL": [(100, 5000, "b"), (3000, 9800, "long"), (0, 100, "before")], "chr10": [(0, 400, "c")], "chrNone": [(0, 10, "never")]}


class _HostCopy:
    """Hands every shard to `inner` as host arrays: the sink's host-part route."""
    takes_aligned_blocks = True

    def __init__(self, inner):
        self.inner = inner

    def __call__(self, shard):
        self.inner({k: (v.cpu().numpy() if isinstance(v, torch.Tensor) else v) for k, v in shard.items()})

    def close(self):
        self.inner.close()


def _regions_run(snv_model, fa, d, tag, part_rows, monkeypatch, listed, host=False, mutations=None, **kw):
    from mural_amd import predict as P
    monkeypatch.setattr(P, "_ALIGNED_PART_ROWS", part_rows)
    sink = P.SummarySink(d / tag, annotations=ANNOT, **kw)
    n = P.predict_regions_sharded(_forward(snv_model, fa), REGIONS, "A", sink=_HostCopy(sink) if host else sink, collect=False,
                                  mutations=listed.write(d / "sim_m.bed") if mutations is None else mutations)
    return sink, n


def test_shard_invariance_and_the_round_trip(files, snv_model, monkeypatch):
    """A labelled regions run with simulate=5, simulate_seed=7 at two part sizes and through the host-part route: byte-identical
    .annotation.sim.tsv and mutation lists; the list of replicate 0 fed back as `mutations=` gives number_of_mut per name equal to
    replicate 0's counts."""
    d, fa = files
    listed = Listed(REGIONS, "A")
    kw = dict(simulate=5, simulate_seed=7, simulate_write=(0, 3))
    runs = [_regions_run(snv_model, fa, d, "sim_a", 700, monkeypatch, listed, **kw), _regions_run(snv_model, fa, d, "sim_b", 4096, monkeypatch, listed, **kw),
            _regions_run(snv_model, fa, d, "sim_h", 1500, monkeypatch, listed, host=True, **kw)]
    texts = [[(d / f"{tag}{suffix}").read_bytes() for suffix in (".annotation.sim.tsv", ".sim0.mutations.bed", ".sim3.mutations.bed")]
             for tag in ("sim_a", "sim_b", "sim_h")]
    assert texts[0] == texts[1] == texts[2] and all(len(t) > 0 for t in texts[0])
    counts = runs[0][0].simulation_counts()
    assert all(np.array_equal(counts, sink.simulation_counts()) for sink, _ in runs[1:])
    names, got_counts, observed, expected = runs[0][0].result()["simulation"]
    assert names == ["a", "b", "c", "gap", "tail", "long", "before", "never"] and counts.shape == (8, 3, 5)
    assert counts[names.index("b")].min() > 0 and not counts[names.index("never")].any() and not counts[names.index("gap")].any()
    lines = [ln.split("\t") for ln in texts[0][0].decode().splitlines()]
    g = names.index("b")
    row = lines[1 + 3 * g]
    assert row[:2] == ["b", "1"] and int(row[2]) == int(observed[g, 0]) > 0 and float(row[3]) == float(expected[g, 0])
    assert float(row[4]) == counts[g, 0].mean() and int(row[7]) == int((counts[g, 0] >= observed[g, 0]).sum())
    # the round trip: replicate 0 as the observed side of a second run
    back, n = _regions_run(snv_model, fa, d, "sim_back", 4096, monkeypatch, listed, mutations=str(d / "sim_a.sim0.mutations.bed"))
    table = back.result()["annotations"][2]
    assert n == runs[0][1] and np.array_equal(table[:, 2:5].astype(np.int64), counts[:, :, 0].astype(np.int64))


def test_table_route_equals_the_in_flight_sink(tmp_path):
    """Device shards with dyadic probabilities (multiples of 1/16: exact at the table's four digits) written by TsvSink and reduced in
    flight; ``tables.simulate_table`` on the file through the same entries: equal counts, equal lists."""
    from mural_amd import tables
    from mural_amd.predict import SummarySink, TsvSink
    rng = np.random.default_rng(8)
    annot = tables.read_annotations({"chrA": [(0, 1500, "x"), (1000, 5000, "y"), (1200, 1300, "x")], "chrB": [(0, 10 ** 6, "y"), (50, 60, "z")]})
    out = str(tmp_path / "t.tsv")
    tsv = TsvSink(out)
    sink = SummarySink(str(tmp_path / "s"), annotations=annot, simulate=6, simulate_seed=99, simulate_write=(4,))
    for chrom, n in (("chrA", 1500), ("chrB", 700)):
        prob = np.zeros((n, 4), np.float32)
        prob[:, 1:] = rng.integers(0, 5, size=(n, 3)) / 16.0
        prob[:, 0] = 1.0 - prob[:, 1:].sum(axis=1)
        start = np.cumsum(rng.integers(1, 5, size=n)).astype(np.int64)
        for rows in np.array_split(np.arange(n), 2):
            shard = {"chrom": chrom, "start": _up(start[rows]), "end": _up(start[rows] + 1), "strand": _up(rng.integers(0, 2, size=len(rows)).astype(np.uint8)),
                     "label": _up(rng.integers(0, 4, size=len(rows)).astype(np.float32)), "prob": _up(prob[rows]), "n_class": 4, "calibrated": False,
                     "aligned": True}
            tsv(dict(shard))
            sink(dict(shard))
    tsv.close()
    sink.close()
    names, counts, observed, expected = tables.simulate_table(out, annot, 6, 99, 4, write=(4,), out_prefix=str(tmp_path / "t"), chunk_bytes=16 << 10)
    want_names, want_counts, want_observed, want_expected = sink.result()["simulation"]
    assert names == want_names and np.array_equal(counts, want_counts) and counts.sum() > 1000
    assert np.array_equal(observed, want_observed) and np.array_equal(expected, want_expected)
    assert (tmp_path / "t.sim4.mutations.bed").read_text() == (tmp_path / "s.sim4.mutations.bed").read_text()

    class Args:
        pred_file, annotations, n_class, out_prefix, simulate, seed, write_simulated = out, annot, 4, str(tmp_path / "calc"), 6, 99, None
    tables.run_simulate_calc(Args)
    assert (tmp_path / "calc.annotation.sim.tsv").read_text() == (tmp_path / "s.annotation.sim.tsv").read_text()
