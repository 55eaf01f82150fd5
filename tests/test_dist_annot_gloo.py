"""world_size-2 and -3 gloo tests (CPU) of the annotation table's merge across ranks: every rank reduces its rows of each shard, close()
exchanges the integer tables in the sink's single all_gather_object, and rank 0's sums are the single-process ones bit for bit."""
import os

import pytest
import torch.distributed as dist
import torch.multiprocessing as mp

from tests import _annot_data as D
from tests.test_dist_gloo import _free_port


def _per_chrom():
    return {"chrA": D.rows(300, 4, 0), "chrB": D.rows(40, 4, 1, lo=0, hi=70, hole=(62, 64))}


def _reduce(parts, order, prefix=None):
    import numpy as np
    from mural_amd.predict import SummarySink
    sink = SummarySink(prefix, annotations=D.intervals_dict(), parts=parts)
    per_chrom = _per_chrom()
    for chrom in order:
        prob, start, label = per_chrom[chrom]
        perm = np.random.default_rng(len(start)).permutation(len(start))      # a gathered shard: any order, every rank sees all of it
        sink({"chrom": chrom, "start": start[perm], "end": start[perm] + 1, "strand": np.zeros(len(start), np.uint8), "label": label[perm],
              "prob": prob[perm], "n_class": 4, "calibrated": False})
    sink.close()
    names, meta, table = sink.result()["annotations"]
    return sink.annotation_sums().tobytes(), (names, meta.tolist(), table.tobytes()), sink.rows


def _worker(rank, world, port, prefix, q):
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
    dist.init_process_group("gloo", rank=rank, world_size=world)
    try:
        q.put((rank,) + _reduce(True, ["chrA", "chrB"][::1 if rank == 0 else -1], prefix))      # the ranks meet the chromosomes in different orders
    finally:
        dist.destroy_process_group()


@pytest.mark.parametrize("world", [2, 3])
def test_ranked_sinks_merge_to_the_single_process_sums(tmp_path, world):
    want = _reduce(False, ["chrA", "chrB"])
    assert D.as_integers(__import__("numpy").frombuffer(want[0], "u8").reshape(12, 3, 4)) == D.oracle(_per_chrom(), 4, D.NAMES)
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
    for rank, sums, result, rows in res:
        assert sums == want[0] and result == want[1] and rows == want[2]
    assert sorted(os.listdir(tmp_path)) == ["p.annotation.corr.txt", "p.annotation.mut_rates.tsv"]          # rank 0 alone writes
