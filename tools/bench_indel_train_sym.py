"""GPU box: the INDEL (UNet_Small) training step from the dense window against the step from SymbolWindows, at the configuration of
tools/bench_indel_train.py (L = 8000, 8 classes, 8 channels, k = 7, down_list 1 4 5 5 5 2, use_reverse, batch 128, fused Adam).

  (a) steps/s of the dense step and of the symbol step over one resident batch, alternating in one process
  (b) peak device memory of each (torch's allocator: ``max_memory_allocated``)
  (c) steps/s of ``train_epoch`` fed by ``EpochLoader(model_type="indel")`` dense against ``symbols=True`` on a synthetic FASTA + BED

Every leg: `--warmup` untimed rounds, `--repeats` timed ones with a device synchronise inside the timed window; median, min and max
are printed, and one JSON line at the end.  ``--legs dense --root <tree>`` times the dense step alone with the package of another
checkout (the parent commit) -- ``--parent <tree>`` does that in a child process of the same call and adds its figures."""
import argparse
import ctypes as C
import json
import os
import subprocess
import sys
import tempfile
import time

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
CFG = dict(CNN_out_channels=8, CNN_kernel_size=7, down_list=[1, 4, 5, 5, 5, 2], use_reverse=True)
L, N_CLASS, R_LOCAL, ORDER = 8000, 8, 10, 3


def rate(units, secs):
    r = sorted(units / s for s in secs)
    return dict(median=float(np.median(r)), min=r[0], max=r[-1], n=len(r))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--root", default=os.path.dirname(HERE), help="checkout whose mural_amd is measured")
    ap.add_argument("--parent", default=None, help="another checkout: its dense step is timed in a child process of this call")
    ap.add_argument("--legs", default="dense,symbols")
    ap.add_argument("--batch", type=int, default=128)
    ap.add_argument("--steps", type=int, default=20, help="steps per timed round")
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--rows", type=int, default=1024, help="BED rows of the loader-fed epochs")
    ap.add_argument("--no-epoch", action="store_true")
    args = ap.parse_args()
    sys.path.insert(0, args.root)
    if not torch.cuda.is_available():
        raise SystemExit("bench_indel_train_sym: no HIP device")
    from mural_amd import _lib
    from mural_amd import train as TR
    from mural_amd.model import model_choice, weights_init
    legs = args.legs.split(",")
    B = args.batch
    res = dict(root=args.root, batch=B, length=L, steps=args.steps)
    torch.manual_seed(0)
    crit = torch.nn.CrossEntropyLoss(reduction="sum")
    codes = torch.randint(0, 4, (B, L), device="cuda")
    y = torch.randint(0, N_CLASS, (B,), device="cuda")
    inputs = {}
    if "dense" in legs:
        inputs["dense"] = torch.nn.functional.one_hot(codes, 4).permute(0, 2, 1).float().contiguous()
    if "symbols" in legs:
        from mural_amd.data import SymbolWindows
        inputs["symbols"] = SymbolWindows(codes.to(torch.uint8))
    del codes

    def fresh():
        torch.manual_seed(0)
        m = model_choice(0, CFG, dict(n_class=N_CLASS), "indel")
        m.apply(weights_init)
        m = m.cuda().train()
        return m, torch.optim.Adam(m.parameters(), lr=1e-3, fused=True)

    models = {n: fresh() for n in inputs}

    def run(name):
        model, opt = models[name]
        x = inputs[name]
        for _ in range(args.steps):
            loss = crit(model(x), y)
            opt.zero_grad()
            loss.backward()
            TR.clip_grad_norm_(model, 10)
            opt.step()
        torch.cuda.synchronize()
        return float(loss.item())

    TR.freeze_host_heap()
    secs, peaks, last = {n: [] for n in inputs}, {}, {}
    for _ in range(args.warmup):
        for n in inputs:
            run(n)
    for _ in range(args.repeats):      # the legs alternate: drift of the machine lands on both
        for n in inputs:
            torch.cuda.synchronize()
            torch.cuda.reset_peak_memory_stats()
            t0 = time.perf_counter()
            last[n] = run(n)
            secs[n].append(time.perf_counter() - t0)
            peaks[n] = max(peaks.get(n, 0), torch.cuda.max_memory_allocated())
    for n in inputs:
        res[f"{n}_steps_per_s"] = rate(args.steps, secs[n])
        res[f"{n}_peak_bytes"] = peaks[n]
        res[f"{n}_last_loss"] = last[n]
        print(n, "step: steps/s", res[f"{n}_steps_per_s"], "peak MiB %.1f" % (peaks[n] / 2 ** 20), "loss %.4f" % last[n], flush=True)
    shape = _lib.MuralIndelShape(N_CLASS, 8, 7, (C.c_int32 * 6)(1, 4, 5, 5, 5, 2), 1, L, 1e-5)
    res["dense_workspace_bytes"] = int(_lib.lib().mural_indel_train_workspace_bytes(C.byref(shape), B))
    if hasattr(_lib.lib(), "mural_indel_train_symbols_workspace_bytes"):
        res["symbols_workspace_bytes"] = int(_lib.lib().mural_indel_train_symbols_workspace_bytes(C.byref(shape), B))
    if args.parent:
        args.parent = os.path.abspath(args.parent)
        env = {k: v for k, v in os.environ.items() if k != "PYTHONPATH"}
        out = subprocess.run([sys.executable, os.path.abspath(__file__), "--root", args.parent, "--legs", "dense", "--batch", str(B), "--steps",
                              str(args.steps), "--warmup", str(args.warmup), "--repeats", str(args.repeats), "--no-epoch"],
                             capture_output=True, text=True, env=env, cwd=args.parent, timeout=900)
        if out.returncode != 0:
            raise SystemExit("parent leg failed:\n" + out.stdout[-2000:] + out.stderr[-4000:])
        parent = json.loads(out.stdout.strip().splitlines()[-1])
        res["parent_dense_steps_per_s"], res["parent_dense_peak_bytes"] = parent["dense_steps_per_s"], parent["dense_peak_bytes"]
        print("parent dense step: steps/s", res["parent_dense_steps_per_s"], "peak MiB %.1f" % (parent["dense_peak_bytes"] / 2 ** 20), flush=True)
    if not args.no_epoch and "symbols" in legs and "dense" in legs:
        from mural_amd.data import EpochLoader
        sys.path.insert(0, HERE)
        from bench_loader import write_inputs
        config = dict(lr_scheduler="StepLR", min_lr=1e-9, restart_lr=1e-4)
        with tempfile.TemporaryDirectory() as tmp:
            fa, bed = write_inputs(tmp, 2, 400_000, args.rows // 2)
            loaders = {"dense": EpochLoader(fa, bed, B, R_LOCAL, ORDER, L // 2, model_type="indel"),
                       "symbols": EpochLoader(fa, bed, B, R_LOCAL, ORDER, L // 2, model_type="indel", symbols=True)}
            nb = loaders["dense"].n_batches

            def epoch(name):
                model, opt = models[name]
                sch = torch.optim.lr_scheduler.StepLR(opt, step_size=10 ** 6, gamma=0.9)
                TR.train_epoch(model, loaders[name].epoch(shuffle=True, generator=torch.Generator().manual_seed(3)), crit, opt, sch, config,
                               "cuda", model_type="indel")
                torch.cuda.synchronize()

            esecs, epeaks = {n: [] for n in loaders}, {}
            for n in loaders:
                epoch(n)
            for _ in range(max(args.repeats, 3)):
                for n in loaders:
                    torch.cuda.synchronize()
                    torch.cuda.reset_peak_memory_stats()
                    t0 = time.perf_counter()
                    epoch(n)
                    esecs[n].append(time.perf_counter() - t0)
                    epeaks[n] = max(epeaks.get(n, 0), torch.cuda.max_memory_allocated())
            for n in loaders:
                res[f"{n}_epoch_steps_per_s"] = rate(nb, esecs[n])
                res[f"{n}_epoch_peak_bytes"] = epeaks[n]
                print(n, "loader-fed train_epoch: steps/s", res[f"{n}_epoch_steps_per_s"], "batches", nb, "peak MiB %.1f" % (epeaks[n] / 2 ** 20),
                      flush=True)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
