"""world_size-2 gloo test (CPU) of the motif tables' merge across ranks: every rank reduces its rows of each shard, close() exchanges the
integer tables in the sink's single all_gather_object, and the result is the single-process one bit for bit."""
import os

import numpy as np
import torch.distributed as dist
import torch.multiprocessing as mp

from tests import _motif_data as D
from tests.test_dist_gloo import _free_port

MOTIFS = (3, 5)


def _shards(order):
    c = D.case("snv")
    for chrom in order:
        prob, start, end, label = c["rows"][chrom]
        perm = np.random.default_rng(len(start)).permutation(len(start))      # a gathered shard: any order, every rank sees all of it
        yield {"chrom": chrom, "start": start[perm], "end": end[perm], "strand": np.zeros(len(start), np.uint8), "label": label[perm],
               "prob": prob[perm], "n_class": 4, "calibrated": False}


def _reduce(parts, order, prefix=None):
    from mural_amd.predict import SummarySink
    sink = SummarySink(prefix, motifs=MOTIFS, kmers=(3,), windows=(1000,), genome=lambda name: D.SEQS[name], parts=parts)
    for shard in _shards(order):
        sink(shard)
    sink.close()
    return ({m: (t.tobytes(), f.tobytes()) for m, (t, f) in sink.motif_sums().items()},
            {m: (names, tab.tobytes()) for m, (names, tab) in sink.result()["motifs"].items()}, sink.rows)


def _worker(rank, world, port, prefix, q):
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
    dist.init_process_group("gloo", rank=rank, world_size=world)
    try:
        # the ranks meet the chromosomes in different orders: their ordinals are reconciled by name in the merge
        q.put((rank,) + _reduce(True, [n for n, _ in D.CHROMS][::1 if rank == 0 else -1], prefix))
    finally:
        dist.destroy_process_group()


def test_ranked_sinks_merge_to_the_single_process_result(tmp_path):
    want = _reduce(False, [n for n, _ in D.CHROMS])
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    port = _free_port()
    procs = [ctx.Process(target=_worker, args=(r, 2, port, str(tmp_path / "p"), q)) for r in range(2)]
    for p in procs:
        p.start()
    res = sorted(q.get(timeout=120) for _ in procs)
    for p in procs:
        p.join(timeout=60)
        assert p.exitcode == 0
    for rank, sums, result, rows in res:
        assert sums == want[0] and result == want[1] and rows == want[2]
    kinds = [f"{m}-motif" for m in MOTIFS] + ["1Kb", "3-mer"]          # rank 0 alone writes
    assert sorted(os.listdir(tmp_path)) == sorted(f"p.{kind}.{ext}" for kind in kinds for ext in ("corr.txt", "mut_rates.tsv"))


def test_merge_reconciles_the_ordinals_by_name():
    """``_kmer_merge`` on two states whose chromosome lists differ: tables added, words renumbered to the merged list and min-merged."""
    from mural_amd.predict import _MOTIF_ORD_SHIFT, _kmer_collapse, _kmer_fold, _kmer_merge, summary_motif_host
    c = D.case("snv")
    per = {}
    for chrom, (prob, start, end, label) in c["rows"].items():
        per[chrom], _ = summary_motif_host(D.SEQS[chrom], prob, start, end, label, 4, (5,))
    states = [_kmer_collapse({5: per[ch][5][0]}, {ch: {5: per[ch][5][1]}}, _MOTIF_ORD_SHIFT) for ch in ("chrM2", "chr10s")]
    assert [s[0] for s in states] == [["chrM2"], ["chr10s"]]      # each is ordinal 0 of its own list
    names, merged = _kmer_merge(states, _MOTIF_ORD_SHIFT)
    _, whole = _kmer_collapse({5: _kmer_fold(per["chrM2"][5][0] + per["chr10s"][5][0])}, {ch: {5: per[ch][5][1]} for ch in per}, _MOTIF_ORD_SHIFT)
    assert names == ["chr10s", "chrM2"]
    assert np.array_equal(merged[5][0], whole[5][0]) and np.array_equal(merged[5][1], whole[5][1])
    seen = merged[5][1] != np.uint64(2 ** 64 - 1)
    assert set((merged[5][1][seen] >> np.uint64(_MOTIF_ORD_SHIFT)).tolist()) == {0, 1}
