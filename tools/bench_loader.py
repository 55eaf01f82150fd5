"""GPU box: the file-level training loaders at BASELINE config 3's shape (r = 10, R = 1000, batch 4096) on a synthetic FASTA + BED.

  (a) loader only, rows/s:  ``EpochLoader.epoch`` consumed to its end (one ``mural_train_batch_encode`` launch per batch)
  (b) loader only, rows/s:  ``train_batches_from_files`` on the same files and seed (dense one-hot segments, group-wise index-select)
  (c) steps/s of ``train_epoch`` fed by each, and of the step alone on one resident batch (the loop of tools/bench_train_sym.py)
  (d) peak device memory of each leg (torch's allocator: ``max_memory_allocated``)

Every leg: `--warmup` untimed passes, `--repeats` timed ones, a device synchronise inside the timed window; median, min and max are
printed, and one JSON line at the end.  ``--routes old --root <tree>`` times the old route alone with the package of another checkout
(the parent commit) on the same inputs."""
import argparse
import json
import os
import sys
import tempfile
import time

import numpy as np
import torch

R_LOCAL, ORDER, R_DISTAL, BATCH = 10, 3, 1000, 4096


def write_inputs(tmp, chroms, chrom_len, rows_per_chrom, seed=7):
    """A seeded synthetic genome (1.2 % N) and a BED of A/T sites on their own strand, class labels 0..3."""
    rng = np.random.default_rng(seed)
    fa, bed = os.path.join(tmp, "g.fa"), os.path.join(tmp, "s.bed")
    with open(fa, "wb") as f, open(bed, "w") as b:
        for c in range(chroms):
            seq = rng.choice(np.frombuffer(b"ACGTN", np.uint8), size=chrom_len, p=[.247, .247, .247, .247, .012])
            f.write(b">chr%d\n" % (c + 1))
            lines = seq[:chrom_len - chrom_len % 80].reshape(-1, 80)
            f.write(b"\n".join(r.tobytes() for r in lines) + b"\n")
            if chrom_len % 80:
                f.write(seq[chrom_len - chrom_len % 80:].tobytes() + b"\n")
            at = np.nonzero((seq == ord("A")) | (seq == ord("T")))[0]
            pos = np.sort(rng.choice(at, size=rows_per_chrom, replace=False))
            lab = rng.choice(4, size=rows_per_chrom, p=[0.955, 0.015, 0.015, 0.015])
            b.write("".join("chr%d\t%d\t%d\t.\t%d\t%s\n" % (c + 1, p, p + 1, v, "+" if seq[p] == ord("A") else "-") for p, v in zip(pos, lab)))
    return fa, bed


def timed(fn, warmup, repeats):
    """[seconds] of `repeats` calls of fn() after `warmup` untimed ones; fn synchronises itself.  Also the peak allocation of the timed calls."""
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    out = []
    for _ in range(repeats):
        t0 = time.perf_counter()
        fn()
        out.append(time.perf_counter() - t0)
    return out, torch.cuda.max_memory_allocated()


def rate(units, secs):
    r = sorted(units / s for s in secs)
    return dict(median=float(np.median(r)), min=r[0], max=r[-1], n=len(r))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--root", default=os.path.dirname(os.path.dirname(os.path.abspath(__file__))), help="checkout whose mural_amd is measured")
    ap.add_argument("--routes", default="new,old", help="new, old or both")
    ap.add_argument("--chroms", type=int, default=2)
    ap.add_argument("--chrom-len", type=int, default=3_000_000)
    ap.add_argument("--rows-per-chrom", type=int, default=40960)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--train-repeats", type=int, default=3)
    ap.add_argument("--no-train", action="store_true")
    args = ap.parse_args()
    sys.path.insert(0, args.root)
    if not torch.cuda.is_available():
        raise SystemExit("bench_loader: no HIP device (a loader rate is a GPU measurement; there is no CPU stand-in)")
    import bench
    from mural_amd import train as TR
    from mural_amd.data import ingest
    routes = args.routes.split(",")
    dev = torch.device("cuda", 0)
    res = dict(shape=dict(local_radius=R_LOCAL, distal_radius=R_DISTAL, batch=BATCH, rows=args.chroms * args.rows_per_chrom), root=args.root)
    with tempfile.TemporaryDirectory() as tmp:
        fa, bed = write_inputs(tmp, args.chroms, args.chrom_len, args.rows_per_chrom)
        n_rows = args.chroms * args.rows_per_chrom
        feeds = {}
        if "new" in routes:
            from mural_amd.data import EpochLoader
            t0 = time.perf_counter()
            loader = EpochLoader(fa, bed, BATCH, R_LOCAL, ORDER, R_DISTAL, device=dev)
            torch.cuda.synchronize()
            res["new_construct_s"] = time.perf_counter() - t0
            feeds["new"] = lambda: loader.epoch(shuffle=True, generator=torch.Generator().manual_seed(3))
            res["batches"] = loader.n_batches
        if "old" in routes:
            # (the old route reads and packs the files on every call: that is part of what an epoch costs through it)
            feeds["old"] = lambda: ingest.train_batches_from_files(fa, bed, BATCH, R_LOCAL, ORDER, R_DISTAL, shuffle=True,
                                                                   generator=torch.Generator().manual_seed(3), device=dev)

        def consume(feed):
            n = 0
            for batch in feed():
                n += batch[0].shape[0]
            torch.cuda.synchronize()
            assert n == n_rows
        for name, feed in feeds.items():
            secs, peak = timed(lambda: consume(feed), args.warmup, args.repeats)
            res[f"{name}_loader_rows_per_s"] = rate(n_rows, secs)
            res[f"{name}_loader_peak_bytes"] = peak
            print(name, "loader only: rows/s", res[f"{name}_loader_rows_per_s"], "peak MiB %.1f" % (peak / 2 ** 20), flush=True)
        if not args.no_train:
            config = dict(lr_scheduler="StepLR", min_lr=1e-9, restart_lr=1e-4)
            model = bench.build_model(dev).train()
            opt = TR.Adam(model.parameters(), lr=1e-3)
            sch = torch.optim.lr_scheduler.StepLR(opt, step_size=10 ** 6, gamma=0.9)
            crit = TR.CrossEntropySum()
            steps = {}

            def epoch(feed, name):
                k = 0

                def counted():
                    nonlocal k
                    for batch in feed():
                        k += batch[0].shape[0] > 1
                        yield batch
                TR.train_epoch(model, counted(), crit, opt, sch, config, dev)
                torch.cuda.synchronize()
                steps[name] = k
            # the step alone on one resident symbol batch, through the same train_epoch loop (its loss.item() per batch included)
            order = list(feeds)
            first = next(iter(feeds[order[0]]()))
            resident = [tuple(first)] * 20
            legs = [("step_only", lambda: resident)] + [(n, feeds[n]) for n in order]
            secs = {n: [] for n, _ in legs}
            peaks = {}
            for n, f in legs:      # warm every leg, then alternate them
                epoch(f, n)
            for _ in range(args.train_repeats):
                for n, f in legs:
                    torch.cuda.synchronize()
                    torch.cuda.reset_peak_memory_stats()
                    t0 = time.perf_counter()
                    epoch(f, n)
                    secs[n].append(time.perf_counter() - t0)
                    peaks[n] = max(peaks.get(n, 0), torch.cuda.max_memory_allocated())
            for n, _ in legs:
                res[f"{n}_train_steps_per_s"] = rate(steps[n], secs[n])
                res[f"{n}_train_peak_bytes"] = peaks[n]
                print(n, "train_epoch: steps/s", res[f"{n}_train_steps_per_s"], "steps", steps[n], "peak MiB %.1f" % (peaks[n] / 2 ** 20), flush=True)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
