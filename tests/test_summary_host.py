"""CPU tests of the genome summaries in flight (mural_amd.predict.SummarySink / TeeSink): the numpy path against a plain-Python loop, the
multi-rank merge under gloo with a host forward, the tee's error handling and the command line's argument errors."""
import importlib.util
import os
import socket

import numpy as np
import pytest
import torch.distributed as dist
import torch.multiprocessing as mp

from tests import _summary_data as D

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _host_shard(name, prob, start, end, label, k, rows=slice(None), aligned=True):
    shard = {"chrom": name, "start": start[rows], "end": end[rows], "strand": np.zeros(len(start[rows]), np.uint8), "label": label[rows],
             "prob": prob[rows], "n_class": k, "calibrated": False}
    if aligned:
        shard["aligned"] = True
    return shard


@pytest.mark.parametrize("n_class", [2, 4])
@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_numpy_path_equals_a_python_loop(dtype, n_class):
    from mural_amd.predict import SummarySink
    regions = [(0, 500), (200, 900), (250, 300), (10 ** 7, 10 ** 7 + 5)]
    for n, layout in [(n, "mixed") for n in D.SIZES] + [(3 * D.CHUNK + 17, "long")]:
        prob, start, end, label = D.rows(n, n_class, dtype, layout)
        want, total, n_sites = D.brute_force(prob, start, end, label, n_class, D.WINDOWS, regions)
        cuts = sorted({0, n // 3, n})
        perm = np.random.default_rng(n).permutation(n)
        for gathered in (False, True):
            sink = SummarySink(windows=D.WINDOWS, benchmark_regions={"chrH": ([r[0] for r in regions], [r[1] for r in regions])})
            if gathered:
                sink(_host_shard("chrH", prob[perm], start[perm], end[perm], label[perm], n_class, aligned=False))
            else:
                for a, b in zip(cuts[:-1], cuts[1:]):
                    sink(_host_shard("chrH", prob, start, end, label, n_class, slice(a, b)))
            sink.close()
            res = sink.result()
            assert res["n_sites"] == n_sites and abs(res["prob_sum"] - total) <= 1e-12 * max(total, 1e-300)
            for W in D.WINDOWS:
                keys, table = res["windows"][W]
                assert keys == [("chrH", b * W + W) for b in sorted(want[W])]
                ref = np.array([want[W][b] for b in sorted(want[W])])
                assert np.array_equal(table[:, :1 + n_class], ref[:, :1 + n_class])
                assert (np.abs(table[:, 1 + n_class:] - ref[:, 1 + n_class:]) <= 1e-12 * ref[:, 1 + n_class:]).all()


def test_host_status_and_calibration(tmp_path):
    from mural_amd.data.ingest import poisson_calibrate
    from mural_amd.predict import SummarySink, summary_rows_host
    prob, start, end, label = D.rows(200, 4, np.float64)
    for what, msg in (("label", "mut_type outside"), ("start", "negative start")):
        lab, st = label.copy(), start.copy()
        if what == "label":
            lab[5] = 4
        else:
            st[0] = -1
        sink = SummarySink(tmp_path / "s", windows=(64,))
        sink(_host_shard("c", prob, st, end, lab, 4))
        with pytest.raises(ValueError, match=msg):
            sink.close()
        sink.abort()
        assert os.listdir(tmp_path) == []
    with pytest.raises(ValueError, match="calibrated already"):
        SummarySink(poisson=True)(dict(_host_shard("c", prob, start, end, label, 4), calibrated=True))
    sink = SummarySink(windows=(64,), poisson=True)
    sink(_host_shard("c", prob, start, end, label, 4))
    sink.close()
    want = summary_rows_host(poisson_calibrate(prob[:, :4]), start, end, label, 4, (64,))
    assert abs(sink.result()["prob_sum"] - want[1]) <= 1e-12 * want[1]
    with pytest.raises(ValueError):
        SummarySink(windows=(0,))


# ---- ranks ---------------------------------------------------------------------------------------------------------------------------------
def _free_port():
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        return s.getsockname()[1]


def _run(bed, prefix, parts, set_attr=setattr):
    from mural_amd import predict as P
    from mural_amd.data import ingest as I
    from tests.test_dist_gloo import _ordered_forward
    set_attr(I, "PIECE_ROWS", 53)
    set_attr(P, "_ALIGNED_PART_ROWS", 37)      # a rank's block goes through in several parts
    sink = P.SummarySink(prefix, windows=(1000, 64), parts=parts)
    n = P.predict_bed_sharded(_ordered_forward(), bed, segment_center=700, sink=sink, collect=False)
    res = sink.result()
    return n, res["n_sites"], res["prob_sum"]


def _rank_worker(rank, world, port, bed, prefix, q):
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
    dist.init_process_group("gloo", rank=rank, world_size=world)
    try:
        q.put((rank,) + _run(bed, prefix, True))
    finally:
        dist.destroy_process_group()


@pytest.mark.parametrize("world", [2, 3])
def test_ranks_write_the_files_of_one_process(tmp_path, world, monkeypatch):
    """A host forward under gloo: aligned chromosomes in parts (chrB has fewer rows than ranks), chrD out of order (gathered, every rank
    takes its slice of the sorted rows).  The counts are those of world 1 exactly; the rates are printed as float32 and the totals agree
    within the float64 bound of a sum in another order."""
    from mural_amd.tables import regional_output_names
    from tests.test_dist_gloo import _ordered_bed
    bed = str(tmp_path / "o.bed")
    rows = _ordered_bed(bed)
    n1, sites1, sum1 = _run(bed, str(tmp_path / "w1"), False, monkeypatch.setattr)
    assert n1 == sites1 == len(rows)
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    port = _free_port()
    procs = [ctx.Process(target=_rank_worker, args=(r, world, port, bed, str(tmp_path / "wN"), q)) for r in range(world)]
    for p in procs:
        p.start()
    res = sorted(q.get(timeout=120) for _ in procs)
    for p in procs:
        p.join(timeout=60)
        assert p.exitcode == 0
    for _, n, sites, total in res:                         # every rank holds the merged result
        assert n == sites == len(rows) and abs(total - sum1) <= 1e-12 * sum1
    for W in (1000, 64):
        for a, b in zip(regional_output_names(str(tmp_path / "w1"), W)[:2], regional_output_names(str(tmp_path / "wN"), W)[:2]):
            assert open(a).read() == open(b).read() and len(open(a).readlines()) > 1, (W, a)


# ---- tee -----------------------------------------------------------------------------------------------------------------------------------
class _Sink:
    takes_aligned_blocks = True
    parts = False

    def __init__(self, fail_at=None):
        self.fail_at, self.seen, self.closed, self.aborted = fail_at, 0, False, 0

    def __call__(self, shard):
        self.seen += 1
        if self.fail_at == self.seen:
            raise OSError("disk full")

    def close(self):
        if self.fail_at == "close":
            raise ValueError("bad rows")
        self.closed = True

    def abort(self):
        self.aborted += 1


def test_tee_forwards_and_aborts_the_siblings_of_a_failing_sink():
    from mural_amd.predict import TeeSink
    a, b, c = _Sink(), _Sink(fail_at=2), _Sink()
    tee = TeeSink(a, b, c)
    assert tee.takes_aligned_blocks and not tee.parts
    tee({"x": 1})
    assert (a.seen, b.seen, c.seen) == (1, 1, 1)
    with pytest.raises(OSError, match="disk full"):
        tee({"x": 2})
    assert (a.aborted, b.aborted, c.aborted) == (1, 0, 1) and c.seen == 1
    a, b = _Sink(), _Sink(fail_at="close")
    with pytest.raises(ValueError, match="bad rows"):
        TeeSink(a, b).close()
    assert a.closed and a.aborted == 1
    a, b = _Sink(), _Sink()
    tee = TeeSink(a, b)
    tee.close()
    assert a.closed and b.closed and not a.aborted
    tee.abort()
    assert (a.aborted, b.aborted) == (1, 1)
    b.parts = True
    plain = type("Plain", (), {"__call__": lambda self, shard: None})()
    assert not TeeSink(a, b).parts and not TeeSink(a, plain).takes_aligned_blocks
    a.parts = True
    assert TeeSink(a, b).parts
    with pytest.raises(ValueError):
        TeeSink()


# ---- command line ----------------------------------------------------------------------------------------------------------------------------
def test_command_line_argument_errors():
    spec = importlib.util.spec_from_file_location("predict_files", os.path.join(ROOT, "tools", "predict_files.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    with pytest.raises(SystemExit, match="--no-table"):
        mod.main(["model", "g.fa", "sites.bed", "out.tsv", "--summary", "p", "--window_size", "1000", "--no-table"])
    with pytest.raises(SystemExit, match="--no-table"):
        mod.main(["model", "g.fa", "out.tsv", "--regions", "chr1", "--summary", "p", "--window_size", "1000", "--no-table"])
    with pytest.raises(SystemExit, match="--window_size needs --summary"):
        mod.main(["model", "g.fa", "sites.bed", "out.tsv", "--window_size", "1000"])
    with pytest.raises(SystemExit, match="--window_size needs --summary"):
        mod.main(["model", "g.fa", "out.tsv", "--regions", "chr1", "--window_size=1000"])
    with pytest.raises(SystemExit, match="--m_proportion"):
        mod.main(["model", "g.fa", "sites.bed", "out.tsv", "--genomewide_mu", "1e-8"])
    with pytest.raises(SystemExit, match="nothing to do"):
        mod.main(["model", "g.fa", "sites.bed", "--no-table"])
