"""world_size-2 and -3 gloo tests (CPU) of the simulated counts' merge across ranks: every rank draws for its rows of each shard, close()
exchanges the integer tables in the sink's single all_gather_object, and rank 0's counts, table file and mutation list are the
single-process ones byte for byte."""
import os

import pytest
import torch.distributed as dist
import torch.multiprocessing as mp

from tests import _annot_data as D
from tests.test_dist_gloo import _free_port
from tests.test_simulate_host import brute_force, per_chrom_rows


def _reduce(parts, prefix):
    import numpy as np
    from mural_amd.predict import SummarySink
    sink = SummarySink(prefix, annotations=D.intervals_dict(), parts=parts, simulate=5, simulate_seed=7, simulate_write=(2,))
    for chrom, (prob, start, strand) in per_chrom_rows().items():
        perm = np.random.default_rng(len(start)).permutation(len(start))      # a gathered shard: any order, every rank sees all of it
        sink({"chrom": chrom, "start": start[perm], "end": start[perm] + 1, "strand": strand[perm],
              "label": (np.arange(len(start)) % 4).astype(np.float32)[perm], "prob": prob[perm], "n_class": 4, "calibrated": False})
    sink.close()
    return sink.simulation_counts().tobytes(), sink.rows


def _worker(rank, world, port, prefix, q):
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
    dist.init_process_group("gloo", rank=rank, world_size=world)
    try:
        q.put((rank,) + _reduce(True, prefix))
    finally:
        dist.destroy_process_group()


@pytest.mark.parametrize("world", [2, 3])
def test_ranked_sinks_merge_to_the_single_process_counts(tmp_path, world):
    import numpy as np
    want = _reduce(False, str(tmp_path / "one"))
    assert np.frombuffer(want[0], np.uint32).reshape(12, 3, 5).tolist() == brute_force(per_chrom_rows(), 4, D.NAMES, 7, 5)
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    port = _free_port()
    procs = [ctx.Process(target=_worker, args=(r, world, port, str(tmp_path / "p"), q)) for r in range(world)]
    for p in procs:
        p.start()
    res = sorted(q.get(timeout=120) for _ in procs)
    for p in procs:
        p.join(timeout=60)
        assert p.exitcode == 0
    for rank, counts, rows in res:
        assert counts == want[0] and rows == want[1]
    for suffix in (".annotation.sim.tsv", ".sim2.mutations.bed"):
        assert (tmp_path / ("p" + suffix)).read_bytes() == (tmp_path / ("one" + suffix)).read_bytes() and (tmp_path / ("p" + suffix)).stat().st_size > 0
    assert sorted(f for f in os.listdir(tmp_path) if f.startswith("p.")) == ["p.annotation.corr.txt", "p.annotation.mut_rates.tsv",
                                                                             "p.annotation.sim.tsv", "p.sim2.mutations.bed"]
