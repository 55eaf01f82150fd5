"""GPU box: saturation mutagenesis on the S configuration (r = 10, R = 1000, 4 classes) beside the forward alone.

  python tools/bench_mutagenesis.py        (environment: SITES = 64, STEPS = 5)

Prints sites/s and windows/s of ``saturation_mutagenesis`` (SITES sites = SITES * 2001 * 3 windows), the time of ``forward_symbols``
alone on the same number of resident windows in the same chunks (the capability the map is built on, and what to compare with), the
ratio of the two, and the split of the map's device time between enumerate + encode, forward and reduce from HIP events; one JSON line
at the end.

  python tools/bench_mutagenesis.py --model_type indel      (environment: SITES = 4, STEPS = 3)

The same for UNet_Small in the shipped insertion geometry (R = 4000, L = 8000, 8 classes, use_reverse; SITES * 8000 * 3 windows) beside
``forward_symbols`` alone on the same resident rows, and ``forward_symbols`` beside ``model(SymbolWindows(..))``, the dense detour it
replaces (bytes expanded to 16 B per column and classified back).

  python tools/bench_mutagenesis.py --profile      (environment also: SHORT_SITES = 65536)

After the map leg, ``mutagenesis_profile`` on the same sites and chunks: its wall time and HIP-event split beside
the map's, and the ratio of the two.  Then the short-window leg, where a chunk holds thousands of sites per table cell: the model
rebuilt at R = 6 (W = 13), SHORT_SITES sites, map and profile with their splits, and the profile entry alone on one resident chunk
through its two add paths (summed per block in LDS, as a call of a whole chunk does; and as calls of 8191 ids, which add to memory
directly)."""
import json
import os
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import bench  # noqa: E402
from mural_amd.data import PackedGenome  # noqa: E402
from mural_amd.mutagenesis import MutagenesisProfile, mutagenesis_profile, mutagenesis_profile_window, mutagenesis_rows, saturation_mutagenesis  # noqa: E402

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


def profile_leg(model, genome, pos, strand, steps, t_map, split_map):
    """``mutagenesis_profile`` beside a map leg already measured on the same sites and chunks: the keys of the JSON line."""
    with torch.no_grad():
        t_prof = timed(lambda: mutagenesis_profile(model, genome, pos, strand, local_radius=r, local_order=ORDER, chunk_windows=CHUNK), steps)
        split = {}
        for _ in range(steps):
            mutagenesis_profile(model, genome, pos, strand, local_radius=r, local_order=ORDER, chunk_windows=CHUNK, timings=split)
    split = {k: v / steps for k, v in split.items()}
    device_ms, map_ms = sum(split.values()), sum(split_map.values())
    print(f"mutagenesis_profile on the same sites: {t_prof * 1e3:8.2f} ms  (profile / map = {t_prof / t_map:.3f})")
    print("device time per profile (HIP events): " + ", ".join(f"{k} {v:.3f} ms ({v / device_ms:.2%})" for k, v in split.items())
          + f";  the map's reduce: {split_map['reduce_ms']:.3f} ms ({split_map['reduce_ms'] / map_ms:.2%})")
    return dict(profile_ms=t_prof * 1e3, profile_over_map=t_prof / t_map, profile_split_ms=split,
                profile_split_share={k: v / device_ms for k, v in split.items()})


def short_window_leg(dev, genome, steps):
    """R = 6: the contended shape.  The whole loop if the model serves that window, and the entry alone on one resident chunk."""
    sites = int(os.environ.get("SHORT_SITES", 65536))
    R6, W = 6, 13
    idx = torch.arange(sites, device=dev, dtype=torch.int64)
    pos, strand = 5000 + idx * 13, (idx & 1).to(torch.uint8)
    out = dict(distal_radius=R6, sites=sites, windows=sites * W * 3, chunk_windows=CHUNK)
    try:
        model = bench.build_model(dev, R6)
        with torch.no_grad():
            t_map = timed(lambda: saturation_mutagenesis(model, genome, pos, strand, r, ORDER, chunk_windows=CHUNK), steps)
            split_map = {}
            saturation_mutagenesis(model, genome, pos, strand, r, ORDER, chunk_windows=CHUNK, timings=split_map)
        print(f"R = 6: saturation_mutagenesis {sites} sites = {sites * W * 3} windows: {t_map * 1e3:8.2f} ms")
        out.update(map_ms=t_map * 1e3, split_ms=split_map, **profile_leg(model, genome, pos, strand, steps, t_map, split_map))
    except RuntimeError as e:
        print(f"R = 6: the model does not serve this window ({e}); the entry alone follows")
        out["model_refused"] = str(e)
    # the entry alone: one chunk of resident log-probabilities, whole (LDS path) and in calls below the LDS threshold (memory path)
    n = CHUNK // (W * 3) + 1
    gen = torch.Generator(device=dev).manual_seed(6)
    ref_logp = torch.log_softmax(torch.randn((n, 4), device=dev, generator=gen), dim=1)
    var_logp = (ref_logp.repeat_interleave(W * 3, dim=0) + 0.5 * torch.randn((n * W * 3, 4), device=dev, generator=gen))[:CHUNK].contiguous()
    ref_symbols = torch.randint(0, 4, (n, W), device=dev, generator=gen).to(torch.uint8)
    prof = MutagenesisProfile.zeros(R6, "snv", 4, 1, dev)
    pieces = [(f, var_logp[f:f + 8191].contiguous()) for f in range(0, CHUNK, 8191)]

    def events(fn, reps=20):
        fn()
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(reps):
            fn()
        b.record()
        torch.cuda.synchronize()
        return a.elapsed_time(b) / reps

    t_lds = events(lambda: mutagenesis_profile_window(ref_logp, var_logp, ref_symbols, None, 0, prof.table, prof.status))
    t_mem = events(lambda: [mutagenesis_profile_window(ref_logp, v, ref_symbols, None, f, prof.table, prof.status) for f, v in pieces])
    print(f"R = 6: the entry alone on one chunk of {CHUNK} ids: {t_lds * 1e3:.1f} us summed per block in LDS, {t_mem * 1e3:.1f} us in "
          f"{len(pieces)} calls that add to memory directly")
    out.update(entry_chunk_lds_us=t_lds * 1e3, entry_chunk_memory_us=t_mem * 1e3, entry_memory_calls=len(pieces))
    return out


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
    if "--profile" in sys.argv[1:]:
        line.update(profile_leg(model, genome, pos, strand, steps, t_map, split))
        line["short_window"] = short_window_leg(dev, genome, steps)
    print(json.dumps(line))


if __name__ == "__main__":
    main()
