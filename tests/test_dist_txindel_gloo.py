"""World-size 2 and 3 gloo tests (CPU) of the INDEL structure table's merge across ranks: every rank reduces its rows of each shard on
the host route, close() exchanges the integer tables in the sink's single all_gather_object, and every rank's sums are the
single-process ones bit for bit, whatever the parts; rank 0 alone writes."""
import io
import os

import pytest
import torch.distributed as dist
import torch.multiprocessing as mp

from tests import _txindel_data as I
from tests.test_dist_gloo import _free_port


def _reduce(parts, pieces, prefix=None):
    import numpy as np
    from mural_amd.predict import SummarySink
    seq, text, names = I.build()
    prob, start, label = I.rows(seq, 8, dtype=np.float32)
    sink = SummarySink(prefix, indel_transcripts=io.StringIO(text), indel_kind="deletion_end", genome=lambda name: seq, parts=parts)
    for rows in np.array_split(np.arange(len(start)), pieces):
        perm = rows[np.random.default_rng(len(rows)).permutation(len(rows))]      # a gathered shard: any order, every rank sees all of it
        sink({"chrom": "chr1", "start": start[perm], "end": start[perm] + 1, "strand": np.zeros(len(perm), np.uint8), "label": label[perm],
              "prob": prob[perm], "n_class": 8, "calibrated": False})
    sink.close()
    table, counters = sink.indel_structure_sums()
    return table.tobytes(), counters.tobytes(), sink.rows


def _worker(rank, world, port, prefix, q):
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
    dist.init_process_group("gloo", rank=rank, world_size=world)
    try:
        q.put((rank,) + _reduce(True, 2 + world, prefix))
    finally:
        dist.destroy_process_group()


@pytest.mark.parametrize("world", [2, 3])
def test_ranked_sinks_merge_to_the_single_process_sums(tmp_path, world):
    import numpy as np
    want = _reduce(False, 1)
    seq, text, names = I.build()
    table = np.frombuffer(want[0], "u8").reshape(len(names), 10, 3)
    prob, start, label = I.rows(seq, 8, dtype=np.float32)
    assert I.as_integers(table, np.frombuffer(want[1], "u8").reshape(-1, 2)) == I.oracle(text, prob, start, label, 8, 2, 1, I.pairs(None, 8), len(seq))
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
    for rank, *got in res:
        assert tuple(got) == want
    assert sorted(os.listdir(tmp_path)) == ["p.indel_structure.tsv"]          # rank 0 alone writes
