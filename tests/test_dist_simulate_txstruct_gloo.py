"""world_size-2 gloo test (CPU) of the structure simulation's merge across ranks: every rank draws for its rows of each shard, close()
exchanges the integer tables in the sink's single all_gather_object, and rank 0's counts and table files are the single-process ones
byte for byte."""
import os

import torch.distributed as dist
import torch.multiprocessing as mp

from tests import _txstruct_data as S
from tests.test_dist_gloo import _free_port

FILES = ["consequence.mut_rates.tsv", "consequence.sim.tsv", "consequence.structure.sim.tsv", "consequence.structure.tsv"]


def _reduce(parts, prefix, bed):
    import numpy as np
    from mural_amd.predict import SummarySink
    seq, _, _ = S.build()
    prob, start, strand, label = S.rows(seq, seed=5, dtype=np.float32)
    sink = SummarySink(prefix, transcripts=bed, genome=lambda name: seq, parts=parts, simulate=5, simulate_seed=7, simulate_transcripts=True,
                       transcript_structure=True, simulate_structure=True)
    for rows in np.array_split(np.random.default_rng(2).permutation(len(start)), 3):      # gathered shards: any order, every rank sees all
        sink({"chrom": "chr1", "start": start[rows], "end": start[rows] + 1, "strand": strand[rows], "label": label[rows].astype(np.float32),
              "prob": prob[rows], "n_class": 4, "calibrated": False})
    sink.close()
    return sink.structure_simulation_counts().tobytes(), sink.result()["structure_simulation"][2].tobytes(), sink.rows


def _worker(rank, world, port, prefix, bed, q):
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
    dist.init_process_group("gloo", rank=rank, world_size=world)
    try:
        q.put((rank,) + _reduce(True, prefix, bed))
    finally:
        dist.destroy_process_group()


def test_ranked_sinks_merge_to_the_single_process_counts(tmp_path):
    import numpy as np
    from mural_amd.summaries import simulate_chrom_key, simulate_txstruct_host
    from mural_amd.tables import read_transcript_structure
    world = 2
    seq, text, names = S.build()
    bed = str(tmp_path / "tx.bed")
    open(bed, "w").write(text)
    want = _reduce(False, str(tmp_path / "one"), bed)
    prob, start, strand, _ = S.rows(seq, seed=5, dtype=np.float32)
    tx = read_transcript_structure(bed)
    twin, _ = simulate_txstruct_host(seq, prob, start, strand, tx[2]["chr1"], tx[3]["chr1"], len(names), simulate_chrom_key("chr1"), 7, 5)
    assert want[0] == twin.tobytes() and twin.any()
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    port = _free_port()
    procs = [ctx.Process(target=_worker, args=(r, world, port, str(tmp_path / "p"), bed, q)) for r in range(world)]
    for p in procs:
        p.start()
    res = sorted(q.get(timeout=120) for _ in procs)
    for p in procs:
        p.join(timeout=60)
        assert p.exitcode == 0
    for rank, counts, lof, rows in res:
        assert counts == want[0] and lof == want[1] and rows == want[2]
    for tail in FILES:
        assert (tmp_path / f"p.{tail}").read_bytes() == (tmp_path / f"one.{tail}").read_bytes() and (tmp_path / f"p.{tail}").stat().st_size > 0
    assert sorted(f for f in os.listdir(tmp_path) if f.startswith("p.")) == [f"p.{tail}" for tail in FILES]
