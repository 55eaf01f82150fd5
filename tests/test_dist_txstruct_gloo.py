"""A world_size-2 gloo test (CPU) of the structure table's merge across ranks: every rank reduces its rows of each shard on the host
route, close() exchanges the integer tables in the sink's single all_gather_object, and every rank's sums are the single-process ones bit
for bit; rank 0 alone writes."""
import io
import os

import torch.distributed as dist
import torch.multiprocessing as mp

from tests import _txstruct_data as S
from tests.test_dist_gloo import _free_port


def _reduce(parts, pieces, prefix=None):
    import numpy as np
    from mural_amd.predict import SummarySink
    seq, text, names = S.build()
    prob, start, strand, label = S.rows(seq, dtype=np.float32)
    sink = SummarySink(prefix, transcripts=io.StringIO(text), genome=lambda name: seq, parts=parts, transcript_structure=True)
    for rows in np.array_split(np.arange(len(start)), pieces):
        perm = rows[np.random.default_rng(len(rows)).permutation(len(rows))]      # a gathered shard: any order, every rank sees all of it
        sink({"chrom": "chr1", "start": start[perm], "end": start[perm] + 1, "strand": strand[perm], "label": label[perm], "prob": prob[perm],
              "n_class": 4, "calibrated": False})
    sink.close()
    table, counters = sink.structure_sums()
    return table.tobytes(), counters.tobytes(), sink.consequence_sums()[0].tobytes(), sink.rows


def _worker(rank, world, port, prefix, q):
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
    dist.init_process_group("gloo", rank=rank, world_size=world)
    try:
        q.put((rank,) + _reduce(True, 3, prefix))
    finally:
        dist.destroy_process_group()


def test_ranked_sinks_merge_to_the_single_process_sums(tmp_path):
    import numpy as np
    world = 2
    want = _reduce(False, 1)
    seq, text, names = S.build()
    table = np.frombuffer(want[0], "u8").reshape(len(names), 9, 3)
    assert S.as_integers(table, np.frombuffer(want[1], "u8").reshape(-1, 2)) == S.oracle(seq, text, *S.rows(seq, dtype=np.float32))
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
    assert sorted(os.listdir(tmp_path)) == ["p.consequence.mut_rates.tsv", "p.consequence.structure.tsv"]          # rank 0 alone writes
