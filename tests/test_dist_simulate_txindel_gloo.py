"""World-size 2 and 3 gloo tests (CPU) of the INDEL structure simulation's merge across ranks: every rank draws over its rows of each
shard on the host route, close() adds the ranks' uint32 tables in the sink's single all_gather_object, and every rank's table is the
single-process one byte for byte, whatever the parts; rank 0 alone writes."""
import io
import os

import pytest
import torch.distributed as dist
import torch.multiprocessing as mp

from tests import _txindel_sim_data as X
from tests.test_dist_gloo import _free_port

R = 9


def _reduce(parts, pieces, prefix=None):
    import numpy as np
    from mural_amd.predict import SummarySink
    text = X.toy_text() + X.random_text(seed=2)
    prob, start, strand, label = X.rows(1000, 8, dtype=np.float32)
    sink = SummarySink(prefix, indel_transcripts=io.StringIO(text), indel_kind="insertion", parts=parts, simulate=R, simulate_seed=X.SEED,
                       simulate_indel_structure=True)
    for rows in np.array_split(np.arange(len(start)), pieces):
        perm = rows[np.random.default_rng(len(rows)).permutation(len(rows))]      # a gathered shard: any order, every rank sees all of it
        sink({"chrom": "chr1", "start": start[perm], "end": start[perm] + 1, "strand": strand[perm], "label": label[perm],
              "prob": prob[perm], "n_class": 8, "calibrated": False})
    sink.close()
    res = sink.result()["indel_structure_simulation"]
    return sink.indel_structure_simulation_counts().tobytes(), res[2].tobytes(), res[3].tobytes(), sink.rows


def _worker(rank, world, port, prefix, q):
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
    dist.init_process_group("gloo", rank=rank, world_size=world)
    try:
        q.put((rank,) + _reduce(True, 2 + world, prefix))
    finally:
        dist.destroy_process_group()


@pytest.mark.parametrize("world", [2, 3])
def test_ranked_sinks_merge_to_the_single_process_table(tmp_path, world):
    import numpy as np
    from mural_amd.summaries import simulate_chrom_key, simulate_txindel_host
    want = _reduce(False, 1)
    text = X.toy_text() + X.random_text(seed=2)
    names, segments, features = X.read(text)
    prob, start, strand, _ = X.rows(1000, 8, dtype=np.float32)
    twin, status = simulate_txindel_host(prob, start, strand, 8, segments, features, len(names), 0, simulate_chrom_key("chr1"), X.SEED, R)
    assert status == 0 and want[0] == twin.tobytes() and twin.any()
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
    assert sorted(os.listdir(tmp_path)) == ["p.indel_structure.sim.tsv", "p.indel_structure.tsv"]          # rank 0 alone writes
