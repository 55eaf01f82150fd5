"""GPU box: what a whole epoch of ``mural_amd.train_run.fit`` costs over the bare training epoch, on the synthetic FASTA + BED of
tools/bench_train_epoch.py (2 chromosomes of 3 Mb, 81920 rows, r = 10, R = 1000, the SNV flagship model; ``--model indel``: a UNet_Small on
symbol windows).

The BED is split by segment (``EpochLoader.split``, --valid-ratio 0.1).  One untimed run of ``fit`` warms everything (graph capture, the
folded eval copy, lazy kernel loads); then `--repeats` runs of ONE epoch of ``fit`` are timed with its ``timings=`` dict -- seconds of
train / validate / report / save, a device synchronise at each boundary -- alternating with the same epoch's training part alone
(``train_epoch_device`` over the same view and seed on a twin model).  Printed per batch size: the medians (min, max), the overhead of the
run over the bare epoch (fit's total / bare - 1), which of validate / report is the larger, and one JSON line at the end."""
import argparse
import json
import os
import shutil
import sys
import tempfile
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from bench_loader import ORDER, R_DISTAL, R_LOCAL, write_inputs  # noqa: E402


def stat(secs):
    s = sorted(secs)
    return dict(median=float(np.median(s)), min=s[0], max=s[-1], n=len(s))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batches", default="128,4096")
    ap.add_argument("--chroms", type=int, default=2)
    ap.add_argument("--chrom-len", type=int, default=3_000_000)
    ap.add_argument("--rows-per-chrom", type=int, default=40960)
    ap.add_argument("--segment-center", type=int, default=300000)
    ap.add_argument("--valid-ratio", type=float, default=0.1)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--model", default="snv", choices=["snv", "indel"])
    args = ap.parse_args()
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    if not torch.cuda.is_available():
        raise SystemExit("bench_train_run: no HIP device (an epoch time is a GPU measurement; there is no CPU stand-in)")
    from mural_amd import train as TR
    from mural_amd import train_run as R
    from mural_amd.data import EpochLoader
    dev = torch.device("cuda", 0)
    indel = args.model == "indel"
    res = dict(shape=dict(local_radius=R_LOCAL, distal_radius=R_DISTAL, rows=args.chroms * args.rows_per_chrom), model=args.model, legs={})
    quiet = lambda *a: None      # noqa: E731
    with tempfile.TemporaryDirectory() as tmp:
        fa, bed = write_inputs(tmp, args.chroms, args.chrom_len, args.rows_per_chrom)
        for B in [int(b) for b in args.batches.split(",")]:
            cfg = dict(local_radius=R_LOCAL, local_order=ORDER, distal_radius=R_DISTAL, n_class=4, lr_scheduler="StepLR", batch_size=B,
                       LR_gamma=0.5, min_lr=1e-9, restart_lr=1e-4, learning_rate=1e-3, weight_decay=0.0, optim="Adam",
                       segment_center=args.segment_center, sampled_segments=10)
            if indel:
                cfg.update(model_no=0, CNN_kernel_size=3, CNN_out_channels=8, down_list=[2, 2, 2, 5, 5, 5], use_reverse=True)
            else:
                cfg.update(model_no=2, local_hidden1_size=150, local_hidden2_size=75, emb_dropout=0.1, local_dropout=0.1, CNN_kernel_size=3,
                           CNN_out_channels=32, distal_fc_dropout=0.25)
            loader = EpochLoader(fa, bed, B, R_LOCAL, ORDER, R_DISTAL, segment_center=args.segment_center, device=dev,
                                 **(dict(model_type="indel", symbols=True) if indel else {}))
            train, valid = loader.split(args.valid_ratio, 1)
            torch.manual_seed(0)
            model = R.prepare_model(cfg, dev, model_type=args.model)
            torch.manual_seed(0)
            twin = R.prepare_model(dict(cfg), dev, model_type=args.model)
            crit = TR.CrossEntropySum()
            opt = TR.make_optimizer(cfg, model.parameters(), device_state=TR.DeviceStepState(dev, cfg["learning_rate"]))
            opt_t = TR.make_optimizer(cfg, twin.parameters(), device_state=TR.DeviceStepState(dev, cfg["learning_rate"]))
            trial = os.path.join(tmp, f"trial_{B}")

            def run(timings=None):
                shutil.rmtree(trial, ignore_errors=True)
                return R.fit(model, cfg, train, valid, epochs=1, trial_dir=trial, grace_period=5, device=dev, model_type=args.model,
                             split_generator_seed=3, printer=quiet, criterion=crit, optimizer=opt, timings=timings)

            def bare():
                gen = torch.Generator().manual_seed(3)
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                TR.train_epoch_device(twin, train.epoch(shuffle=True, generator=gen), crit, opt_t, cfg, dev, train_size=len(train),
                                      model_type=args.model)
                torch.cuda.synchronize()
                return time.perf_counter() - t0

            run()
            bare()
            timings, alone, whole = {}, [], []
            for _ in range(args.repeats):
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                history, _ = run(timings)
                torch.cuda.synchronize()
                whole.append(time.perf_counter() - t0)
                alone.append(bare())
            out = dict(train_rows=len(train), valid_rows=len(valid), train_batches=train.n_batches, valid_batches=valid.n_batches,
                       fit_epoch=stat(whole), bare_epoch=stat(alone), **{k: stat(v) for k, v in timings.items()},
                       valid_loss=history[0]["loss"])
            out["overhead"] = out["fit_epoch"]["median"] / out["bare_epoch"]["median"] - 1.0
            out["dominant"] = max(("validate", "report"), key=lambda k: out[k]["median"])
            res["legs"][str(B)] = out
            print(f"batch {B}: fit epoch {out['fit_epoch']['median']:.3f} s = train {out['train']['median']:.3f} + validate "
                  f"{out['validate']['median']:.3f} + report {out['report']['median']:.3f} + save {out['save']['median']:.3f}; bare epoch "
                  f"{out['bare_epoch']['median']:.3f} s; overhead {100 * out['overhead']:.1f} %; larger of validate / report: {out['dominant']}",
                  flush=True)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
