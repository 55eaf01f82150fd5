"""GPU box: allele footprints (insertions, deletions, multi-base alleles) beside the forward alone.

  python tools/bench_alleles.py                         (environment: ALLELES = 128, STEPS = 5)

S configuration (r = 10, R = 1000, 4 classes): ``allele_footprint`` of a fixed set of ALLELES alleles (ALLELES * 2000 rows, each
predicted on both haplotypes), the time of ``forward_symbols`` alone on the same resident rows of both haplotypes in the same chunks,
the ratio of the two, and the split of the footprint's device time between enumerate + encode and forward from HIP events; one JSON
line at the end.

  python tools/bench_alleles.py --model_type indel      (environment: ALLELES = 4, STEPS = 3)

The same for UNet_Small in the shipped insertion geometry (R = 4000, L = 8000, 8 classes; ALLELES * 7999 rows); its forward includes the
log-softmax of the scores on both sides of the ratio."""
import json
import os
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import bench  # noqa: E402
from mural_amd.data import PackedGenome  # noqa: E402
from mural_amd.mutagenesis import Alleles, allele_footprint, allele_rows, scores_log_softmax  # noqa: E402

R, r, ORDER = 1000, 10, 3
KINDS = [(0, "A"), (0, "CGT"), (0, "ACGTTGCAAGCTTCGATCGGATCCATGCAGTA"), (1, ""), (5, ""), (2, "ACGTA"), (4, "G"), (3, "TGA")]


def timed(fn, steps):
    fn()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(steps):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / steps


def fixed_alleles(n, first, stride, dev):
    """n alleles cycling through KINDS (three insertions, two deletions, two of unequal lengths, one 3-for-3), `stride` apart"""
    kinds = [KINDS[i % len(KINDS)] for i in range(n)]
    table = Alleles.from_host([first + i * stride for i in range(n)], [d for d, _ in kinds], [a for _, a in kinds], dev)
    return table, (torch.arange(n, device=dev) & 1).to(torch.uint8)


def main():
    indel = False
    if "--model_type" in sys.argv[1:]:
        kind = sys.argv[sys.argv.index("--model_type") + 1:][:1]
        if kind not in (["snv"], ["indel"]):
            raise SystemExit("--model_type must be snv or indel")
        indel = kind == ["indel"]
    dev = torch.device("cuda", 0)
    n = int(os.environ.get("ALLELES", 4 if indel else 128))
    steps = int(os.environ.get("STEPS", 3 if indel else 5))
    codes = bench.synthetic_genome(1_000_000)
    packed, mask = bench.pack2(codes)
    genome = PackedGenome(packed, mask, len(codes), dev)
    if indel:
        radius, chunk, model_type = 4000, 24_576, "indel"
        model, weights = bench.indel_model_and_weights(dev)
        model.eval()
        kw = dict(distal_radius=radius, chunk_windows=chunk)
        slots = 2 * radius - 1
    else:
        radius, chunk, model_type, weights = R, 1 << 17, "snv", "synthetic"
        model = bench.build_model(dev)
        kw = dict(local_radius=r, local_order=ORDER, chunk_windows=chunk)
        slots = 2 * radius
    table, strand = fixed_alleles(n, 50_000, 9973, dev)
    rows = n * slots

    def forward(sym, cat):
        return scores_log_softmax(model.forward_symbols(sym)) if indel else model.forward_symbols(cat, sym)

    with torch.no_grad():
        t_fp = timed(lambda: allele_footprint(model, genome, table, strand, **kw), steps)
        # the forward alone: the same rows of both haplotypes, resident, in the same chunks
        chunks = []
        for first in range(0, rows, chunk):
            ref_pos, alt_pos, row_strand, row_allele = allele_rows(genome, table, strand, radius, first, min(chunk, rows - first), model_type)
            chunks.append(genome.encode_allele_windows(alt_pos, row_strand, row_allele, table, radius, r, ORDER, model_type))
            chunks.append(genome.encode_allele_windows(ref_pos, row_strand, torch.full_like(row_allele, -1), table, radius, r, ORDER, model_type))
        t_fwd = timed(lambda: [forward(sym, cat) for sym, cat in chunks], steps)
        del chunks
        split = {}
        for _ in range(steps):
            allele_footprint(model, genome, table, strand, timings=split, **kw)
    split = {k: v / steps for k, v in split.items()}
    device_ms = sum(split.values())
    line = dict(config="indel" if indel else "S", weights=weights, distal_radius=radius, alleles=n, rows=rows, forward_rows=2 * rows,
                chunk_windows=chunk, steps=steps, footprint_ms=t_fp * 1e3, alleles_per_s=n / t_fp, forward_alone_ms=t_fwd * 1e3,
                footprint_over_forward=t_fp / t_fwd, split_ms=split, split_share={k: v / device_ms for k, v in split.items()})
    print(f"allele_footprint ({model_type}) {n} alleles = {rows} rows on two haplotypes: {t_fp * 1e3:8.2f} ms  {n / t_fp:8.1f} alleles/s")
    print(f"forward_symbols alone on the {2 * rows} resident windows: {t_fwd * 1e3:8.2f} ms  (footprint / forward = {t_fp / t_fwd:.3f})")
    print("device time per footprint (HIP events): " + ", ".join(f"{k} {v:.2f} ms ({v / device_ms:.1%})" for k, v in split.items()))
    print(json.dumps(line))


if __name__ == "__main__":
    main()
