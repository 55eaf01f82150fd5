"""gloo tests (CPU, worlds of 2 and 3) of the calibration metrics' merge across ranks: every rank reduces its rows of each host shard,
close() exchanges the integer tables in the sink's single all_gather_object, and every rank holds the single-process tables bit for
bit; rank 0 alone writes.  The calibrator fit across ranks -- its row terms all_reduced, the oracle's ``fit_row_terms`` standing in for
the device kernel as in tests/test_analytics.py::test_oracle_and_host_fit -- reaches the single-process weights within 1e-8."""
import os

import numpy as np
import pytest
import torch.distributed as dist
import torch.multiprocessing as mp

from tests import _util as U
from tests.test_dist_gloo import _free_port


def _row_terms(prob, label, w, need_hessian):
    """sums over the given rows, from the oracle's means"""
    from oracle import eval_ref
    live = label != 255
    loss, g, h = eval_ref.fit_row_terms(eval_ref.fit_features(prob[live]), label[live].astype(np.int64), w, need_hessian)
    n = int(live.sum())
    return loss * n, g * n, h * n


def _shards(order):
    fx = U.load("analytics.npz")
    prob, label = fx["snv_prob"], fx["snv_label"]
    cuts = {"chrB": (0, 2500), "chrA": (2500, 4100), "chrC": (4100, len(label))}
    for chrom in order:
        a, b = cuts[chrom]
        perm = np.random.default_rng(b).permutation(b - a)      # a gathered shard: any order, every rank sees all of it
        yield {"chrom": chrom, "start": (np.arange(a, b) * 3)[perm], "end": (np.arange(a, b) * 3 + 1)[perm], "strand": np.zeros(b - a, np.uint8),
               "label": label[a:b][perm].astype(np.float32), "prob": prob[a:b][perm], "n_class": 4, "calibrated": False}


def _reduce(parts, order, prefix=None, fit=True):
    from mural_amd.predict import SummarySink
    sink = SummarySink(prefix, calibration=True, calibration_bins=15, parts=parts, windows=(1000,),
                       **(dict(fit_calibrator="FullDiri", fit_row_terms=_row_terms) if fit else {}))
    for shard in _shards(order):
        sink(shard)
    sink.close()
    sums, res = sink.calibration_sums(), sink.result()["calibration"]
    return ({"all": sums["all"].tobytes(), "after": sums["after"].tobytes() if fit else None,
             "per": {k: v.tobytes() for k, v in sums["per_chromosome"].items()}},
            {k: v for k, v in res.items() if k not in ("weights", "after", "fit_loss")}, res.get("weights"), res.get("after"), sink.rows)


def _worker(rank, world, port, prefix, q):
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
    dist.init_process_group("gloo", rank=rank, world_size=world)
    try:
        order = ["chrB", "chrA", "chrC"]
        q.put((rank,) + _reduce(True, order[::1 if rank == 0 else -1], prefix))
    finally:
        dist.destroy_process_group()


@pytest.mark.parametrize("world", [2, 3])
def test_ranked_sinks_merge_to_the_single_process_result(tmp_path, world):
    want = _reduce(False, ["chrB", "chrA", "chrC"])
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    port = _free_port()
    procs = [ctx.Process(target=_worker, args=(r, world, port, str(tmp_path / "p"), q)) for r in range(world)]
    for p in procs:
        p.start()
    res = sorted((q.get(timeout=180) for _ in procs), key=lambda r: r[0])
    for p in procs:
        p.join(timeout=60)
        assert p.exitcode == 0
    assert want[1]["rows"] == 6000 and list(want[1]["per_chromosome"]) == ["chrA", "chrB", "chrC"]
    for rank, sums, result, weights, after, rows in res:
        assert sums["all"] == want[0]["all"] and sums["per"] == want[0]["per"] and result == want[1], rank
        print("rank", rank, "weights differ by", np.abs(weights - want[2]).max())
        assert np.abs(weights - want[2]).max() < 1e-8
        assert after["rows"] == 6000 and abs(after["nll"] - want[3]["nll"]) < 1e-8 and after["nll"] <= result["nll"] + 1e-9
    assert sum(r[5] for r in res) == 6000 * world          # every rank saw every gathered shard and took its own rows of it
    assert sorted(os.listdir(tmp_path)) == sorted(["p.1Kb.corr.txt", "p.1Kb.mut_rates.tsv", "p.calibration.txt", "p.fdiri_cal.pkl"])
    fx = U.load("analytics.npz")
    assert np.abs(want[2] - fx["snv_fit_w"]).max() < 1e-8      # (the single-process fit is the fixture's)
