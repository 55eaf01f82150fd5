"""GPU box: saturation mutagenesis on the S configuration (r = 10, R = 1000, 4 classes) beside the forward alone.

  python tools/bench_mutagenesis.py        (environment: SITES = 64, STEPS = 5)

Prints sites/s and windows/s of ``saturation_mutagenesis`` (SITES sites = SITES * 2001 * 3 windows), the time of ``forward_symbols``
alone on the same number of resident windows in the same chunks (the capability the map is built on, and what to compare with), the
ratio of the two, and the split of the map's device time between enumerate + encode, forward and reduce from HIP events; one JSON line
at the end.

  python tools/bench_mutagenesis.py --model_type indel      (environment: SITES = 4, STEPS = 3)

The same for UNet_Small in the shipped insertion geometry (R = 4000, L = 8000, 8 classes, use_reverse; SITES * 8000 * 3 windows) beside
``forward_symbols`` alone on the same resident rows, and ``forward_symbols`` beside ``model(SymbolWindows(..))``, the dense detour it
replaces (bytes expanded to 16 B per column and classified back)."""
import json
import os
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import bench  # noqa: E402
from mural_amd.data import PackedGenome  # noqa: E402
from mural_amd.mutagenesis import mutagenesis_rows, saturation_mutagenesis  # noqa: E402

R, r, ORDER = 1000, 10, 3
CHUNK = 1 << 17


def timed(fn, steps):
    fn()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(steps):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / steps


def main_indel():
    from mural_amd.data.genome import SymbolWindows
    dev = torch.device("cuda", 0)
    sites, steps = int(os.environ.get("SITES", 4)), int(os.environ.get("STEPS", 3))
    R_I, chunk = 4000, 24_576
    codes = bench.synthetic_genome(1_000_000)
    packed, mask = bench.pack2(codes)
    genome = PackedGenome(packed, mask, len(codes), dev)
    model, weights = bench.indel_model_and_weights(dev)
    model.eval()
    idx = torch.arange(sites, device=dev, dtype=torch.int64)
    pos, strand = 50_000 + idx * 9973, (idx & 1).to(torch.uint8)
    windows = sites * 2 * R_I * 3
    with torch.no_grad():
        t_map = timed(lambda: saturation_mutagenesis(model, genome, pos, strand, chunk_windows=chunk, distal_radius=R_I), steps)
        chunks = []
        for first in range(0, windows, chunk):
            rows = mutagenesis_rows(genome, pos, strand, R_I, first, min(chunk, windows - first), "indel")
            chunks.append(genome.encode_subst_windows(*rows, R_I, model_type="indel")[0])
        t_fwd = timed(lambda: [model.forward_symbols(sym) for sym in chunks], steps)
        t_dense = timed(lambda: [model(SymbolWindows(sym)) for sym in chunks], steps)
        del chunks
        split = {}
        for _ in range(steps):
            saturation_mutagenesis(model, genome, pos, strand, chunk_windows=chunk, distal_radius=R_I, timings=split)
    split = {k: v / steps for k, v in split.items()}
    device_ms = sum(split.values())
    line = dict(config="indel", weights=weights, distal_radius=R_I, n_class=8, sites=sites, windows=windows, chunk_windows=chunk, steps=steps,
                map_ms=t_map * 1e3, sites_per_s=sites / t_map, windows_per_s=windows / t_map, forward_alone_ms=t_fwd * 1e3,
                forward_alone_windows_per_s=windows / t_fwd, map_over_forward=t_map / t_fwd, dense_detour_ms=t_dense * 1e3,
                dense_detour_over_forward_symbols=t_dense / t_fwd, split_ms=split, split_share={k: v / device_ms for k, v in split.items()})
    print(f"saturation_mutagenesis (INDEL) {sites} sites = {windows} windows: {t_map * 1e3:8.2f} ms  {sites / t_map:8.2f} sites/s  "
          f"{windows / t_map / 1e3:8.1f} k windows/s")
    print(f"forward_symbols alone on {windows} resident windows: {t_fwd * 1e3:8.2f} ms  (map / forward = {t_map / t_fwd:.3f})")
    print(f"model(SymbolWindows) on the same windows: {t_dense * 1e3:8.2f} ms  (dense detour / forward_symbols = {t_dense / t_fwd:.3f})")
    print("device time per map (HIP events): " + ", ".join(f"{k} {v:.2f} ms ({v / device_ms:.1%})" for k, v in split.items()))
    print(json.dumps(line))


def main():
    if "--model_type" in sys.argv[1:]:
        kind = sys.argv[sys.argv.index("--model_type") + 1:][:1]
        if kind == ["indel"]:
            return main_indel()
        if kind != ["snv"]:
            raise SystemExit("--model_type must be snv or indel")
    dev = torch.device("cuda", 0)
    sites = int(os.environ.get("SITES", 64))
    steps = int(os.environ.get("STEPS", 5))
    if sites < 64:
        raise SystemExit("SITES must be at least 64")
    codes = bench.synthetic_genome(1_000_000)
    packed, mask = bench.pack2(codes)
    genome = PackedGenome(packed, mask, len(codes), dev)
    model = bench.build_model(dev)
    idx = torch.arange(sites, device=dev, dtype=torch.int64)
    pos, strand = 5000 + idx * 9973, (idx & 1).to(torch.uint8)
    W = 2 * R + 1
    windows = sites * W * 3

    with torch.no_grad():
        t_map = timed(lambda: saturation_mutagenesis(model, genome, pos, strand, r, ORDER, chunk_windows=CHUNK), steps)
        # the forward alone: the same windows, resident, in the same chunks
        chunks = []
        for first in range(0, windows, CHUNK):
            rows = mutagenesis_rows(genome, pos, strand, R, first, min(CHUNK, windows - first))
            chunks.append(genome.encode_subst_windows(*rows, R, r, ORDER))
        t_fwd = timed(lambda: [model.forward_symbols(cat, sym) for sym, cat in chunks], steps)
        del chunks
        split = {}
        for _ in range(steps):
            saturation_mutagenesis(model, genome, pos, strand, r, ORDER, chunk_windows=CHUNK, timings=split)
    split = {k: v / steps for k, v in split.items()}
    device_ms = sum(split.values())
    line = dict(config="S", local_radius=r, distal_radius=R, n_class=4, sites=sites, windows=windows, chunk_windows=CHUNK, steps=steps,
                map_ms=t_map * 1e3, sites_per_s=sites / t_map, windows_per_s=windows / t_map, forward_alone_ms=t_fwd * 1e3,
                forward_alone_windows_per_s=windows / t_fwd, map_over_forward=t_map / t_fwd,
                split_ms=split, split_share={k: v / device_ms for k, v in split.items()})
    print(f"saturation_mutagenesis {sites} sites = {windows} windows: {t_map * 1e3:8.2f} ms  {sites / t_map:8.1f} sites/s  "
          f"{windows / t_map / 1e6:6.2f} M windows/s")
    print(f"forward_symbols alone on {windows} resident windows: {t_fwd * 1e3:8.2f} ms  {windows / t_fwd / 1e6:6.2f} M windows/s  "
          f"(map / forward = {t_map / t_fwd:.3f})")
    print("device time per map (HIP events): " + ", ".join(f"{k} {v:.2f} ms ({v / device_ms:.1%})" for k, v in split.items()))
    print(json.dumps(line))


if __name__ == "__main__":
    main()
