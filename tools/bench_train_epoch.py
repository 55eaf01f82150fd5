"""GPU box: one epoch of ``train_epoch`` (host scheduler, ``loss.item()`` every step) against one of ``train_epoch_device`` (graph replays on
the device step state, one read-back per epoch) at batch 128 -- the reference's default, host-bound -- and at batch 4096, fed by
``EpochLoader`` over the synthetic FASTA + BED of tools/bench_loader.py, with 'StepLR' as the reference's defaults have it and the optimiser
``--optim`` names ('Adam', the default, 'AdamW', 'AdamW2', 'SGD': ``make_optimizer``).  ``--model indel`` runs a ``UNet_Small`` (8 channels,
kernel 3, down_list 2,2,2,5,5,5) from ``EpochLoader(model_type="indel", symbols=True)`` instead of the SNV flagship model.

Per batch size: both loops are warmed with one untimed epoch each (the device loop captures its graph there), then `--repeats` timed epochs
alternate between them; a device synchronise sits inside every timed window.  rows/s and steps/s (median, min, max) of both, the share
of the device loop's steps that were graph replays, and both loops' loss of the last epoch are printed, and one JSON line at the end.
``--root <tree>`` takes ``train_epoch`` from another checkout (the parent commit); where that checkout has no device loop for the model
or the optimiser asked for, that leg is skipped."""
import argparse
import inspect
import json
import os
import sys
import tempfile
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from bench_loader import ORDER, R_DISTAL, R_LOCAL, rate, write_inputs  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--root", default=os.path.dirname(os.path.dirname(os.path.abspath(__file__))), help="checkout whose mural_amd is measured")
    ap.add_argument("--batches", default="128,4096")
    ap.add_argument("--chroms", type=int, default=2)
    ap.add_argument("--chrom-len", type=int, default=3_000_000)
    ap.add_argument("--rows-per-chrom", type=int, default=40960)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--optim", default="Adam", choices=["Adam", "AdamW", "AdamW2", "SGD"])
    ap.add_argument("--model", default="snv", choices=["snv", "indel"])
    args = ap.parse_args()
    sys.path.insert(0, args.root)
    if not torch.cuda.is_available():
        raise SystemExit("bench_train_epoch: no HIP device (an epoch rate is a GPU measurement; there is no CPU stand-in)")
    import bench
    from mural_amd import train as TR
    from mural_amd.data import EpochLoader
    dev = torch.device("cuda", 0)
    have_device_loop = hasattr(TR, "train_epoch_device")
    indel = args.model == "indel"
    if indel and have_device_loop and "model_type" not in inspect.signature(TR.train_epoch_device).parameters:
        have_device_loop = False
    kw = dict(model_type="indel") if indel else {}

    def build_model():
        if not indel:
            return bench.build_model(dev).train()
        from mural_amd.model import model_choice, weights_init
        cfg = dict(local_radius=R_LOCAL, local_order=ORDER, distal_radius=R_DISTAL, CNN_kernel_size=3, CNN_out_channels=8,
                   down_list=[2, 2, 2, 5, 5, 5], use_reverse=True, n_class=4, model_no=0)
        m = model_choice(0, cfg, dict(n_class=4), "indel")
        m.apply(weights_init)
        return m.to(dev).train()

    n_rows = args.chroms * args.rows_per_chrom
    res = dict(shape=dict(local_radius=R_LOCAL, distal_radius=R_DISTAL, rows=n_rows), root=args.root, optim=args.optim, model=args.model, legs={})
    with tempfile.TemporaryDirectory() as tmp:
        fa, bed = write_inputs(tmp, args.chroms, args.chrom_len, args.rows_per_chrom)
        for B in [int(b) for b in args.batches.split(",")]:
            config = dict(lr_scheduler="StepLR", batch_size=B, LR_gamma=0.5, min_lr=1e-9, restart_lr=1e-4, learning_rate=1e-3, weight_decay=0.0,
                          optim=args.optim)
            loader = EpochLoader(fa, bed, B, R_LOCAL, ORDER, R_DISTAL, device=dev, **(dict(model_type="indel", symbols=True) if indel else {}))
            crit = TR.CrossEntropySum()
            feed = lambda: loader.epoch(shuffle=True, generator=torch.Generator().manual_seed(3))      # noqa: E731
            counts = {}

            def counted(name):
                k = n = g = 0
                for batch in feed():
                    rows = batch[0].shape[0]
                    k, n, g = k + (rows > 1), n + (rows if rows > 1 else 0), g + (rows == B)
                    yield batch
                counts[name] = (k, n, g)

            torch.manual_seed(0)
            model_h = build_model()
            opt_h = TR.make_optimizer(config, model_h.parameters())
            sch_h = TR.make_scheduler(config, opt_h)
            loss = {}

            def host_epoch():
                loss["host"] = TR.train_epoch(model_h, counted("host"), crit, opt_h, sch_h, config, dev, **kw)
                torch.cuda.synchronize()
            legs = [("host", host_epoch)]
            device_leg = have_device_loop
            if device_leg:
                torch.manual_seed(0)
                model_d = build_model()
                try:
                    opt_d = TR.make_optimizer(config, model_d.parameters(), device_state=TR.DeviceStepState(dev, config["learning_rate"]))
                except ValueError as e:            # (a checkout whose device state serves 'Adam' only)
                    print(f"batch {B}: no device leg: {e}", flush=True)
                    device_leg = False
            if device_leg:

                def device_epoch():
                    loss["device"] = TR.train_epoch_device(model_d, counted("device"), crit, opt_d, config, dev, **kw)
                    torch.cuda.synchronize()
                legs.append(("device", device_epoch))
            for _, fn in legs:
                fn()
            secs = {n: [] for n, _ in legs}
            for _ in range(args.repeats):
                for n, fn in legs:
                    torch.cuda.synchronize()
                    t0 = time.perf_counter()
                    fn()
                    secs[n].append(time.perf_counter() - t0)
            out = dict(batches=loader.n_batches)
            for n, _ in legs:
                k, rows, g = counts[n]
                out[n] = dict(steps=k, rows=rows, full_batches=g, steps_per_s=rate(k, secs[n]), rows_per_s=rate(rows, secs[n]), loss=loss[n])
                print(f"batch {B} {n}: steps/s", out[n]["steps_per_s"], "rows/s", out[n]["rows_per_s"], "steps", k, "of them full", g,
                      "loss %.6g" % loss[n], flush=True)
            if device_leg:
                out["speedup_steps_per_s"] = out["device"]["steps_per_s"]["median"] / out["host"]["steps_per_s"]["median"]
                out["graphs_captured"] = len(model_d._device_epoch_steps)
            res["legs"][str(B)] = out
    print(json.dumps(res))


if __name__ == "__main__":
    main()
