"""Rows/s of the prediction-table tools (mural_amd.tables) end to end, file to file.

Writes a seeded SNV table (default 50 M rows on two synthetic chromosomes, '%.4g' probabilities, plain and .gz) with the project's
row formatter, then times scale, calc_scaling_factor, k-mer (k = 7) and regional (100 kb) on each and prints one JSON line per run
with the split the reader reports: read / inflate (worker thread, overlapped), waiting for it, device parse, the rest (consumer
kernels, format / deflate / write, host merges).  Kernel times: run this under `rocprofv3 --kernel-trace --stats -- python
tools/bench_tables.py ...` in a run of its own.

--reference N: the reference scripts (through the stand-ins of tools/make_tables_golden.py) on the first N rows of the plain
table -- a HOST figure, taken on whatever machine runs it; it needs the reference tree.

    python tools/bench_tables.py --rows 50000000 --dir /tmp/tb
"""
import argparse
import json
import os
import sys
import tempfile
import time
import types

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def write_inputs(d, rows, seed=5):
    import gzip
    from mural_amd.predict import format_rows_host
    os.makedirs(d, exist_ok=True)
    table, fasta = os.path.join(d, "bench.tsv"), os.path.join(d, "bench.fa")
    if os.path.exists(table) and os.path.exists(table + ".gz") and os.path.exists(fasta):
        return table, fasta
    rng = np.random.default_rng(seed)
    half = rows // 2
    lens = [half + 10, rows - half + 10]
    with open(fasta, "w") as fh:
        for i, n in enumerate(lens):
            seq = np.frombuffer(b"ACGT", np.uint8)[rng.integers(0, 4, size=n)].tobytes().decode()
            fh.write(f">chr{i + 1}\n" + "\n".join(seq[j:j + 60] for j in range(0, n, 60)) + "\n")
    head = ("\t".join(["chrom", "start", "end", "strand", "mut_type"] + [f"prob{i}" for i in range(4)]) + "\n").encode()
    with open(table, "wb") as fh, gzip.open(table + ".gz", "wb", compresslevel=1) as gz:
        fh.write(head)
        gz.write(head)
        step = 4_000_000
        for c, n in enumerate([half, rows - half]):
            for s0 in range(0, n, step):
                m = min(step, n - s0)
                start = np.arange(s0, s0 + m, dtype=np.int64) + 5
                p = 10.0 ** rng.uniform(-9, -2, size=(m, 3))
                prob = np.concatenate([1 - p.sum(axis=1, keepdims=True), p], axis=1)
                txt = format_rows_host([f"chr{c + 1}"], None, start, start + 1, rng.integers(0, 2, size=m).astype(np.uint8),
                                       rng.integers(0, 4, size=m).astype(np.float32), prob)
                fh.write(txt)
                gz.write(txt)
    return table, fasta


def run(tool, table, fasta, d, chunk_bytes):
    import torch
    from mural_amd import tables
    timing = {}
    t0 = time.perf_counter()
    if tool == "scale":
        tables._scale_file(table, 0.5, 4, os.path.join(d, "out.tsv" + (".gz" if table.endswith(".gz") else "")), chunk_bytes, timing)
    elif tool == "calc_scaling_factor":
        tables.prob_sum_file(table, 4, None, chunk_bytes)
    elif tool == "kmer7":
        args = types.SimpleNamespace(pred_file=table, ref_genome=fasta, out_prefix=os.path.join(d, "k"), kmer_length=7, n_class=4)
        tables.run_kmer_corr_calc(args, "snv", chunk_bytes=chunk_bytes)
    elif tool == "regional100k":
        args = types.SimpleNamespace(pred_file=table, window_size=100000, ratio_cutoff=0.2, n_class=4, out_prefix=os.path.join(d, "r"))
        tables.run_regional_corr_calc(args, chunk_bytes=chunk_bytes)
    torch.cuda.synchronize()
    return time.perf_counter() - t0, timing


def reference_rate(table, fasta, d, n):
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import make_tables_golden as G
    scaling, kmer, regional = G._load_reference()
    sl = os.path.join(d, "slice.tsv")
    with open(table) as src, open(sl, "w") as dst:
        for i, line in enumerate(src):
            if i > n:
                break
            dst.write(line)
    out = {}
    t = time.perf_counter()
    scaling.apply_scaling(sl, 0.5, 4, os.path.join(d, "ref_scaled.tsv"))
    out["scale"] = n / (time.perf_counter() - t)
    t = time.perf_counter()
    kmer.run_kmer_corr_calc(types.SimpleNamespace(pred_file=sl, ref_genome=fasta, out_prefix=os.path.join(d, "rk"), kmer_length=7,
                                                  n_class=4), "snv")
    out["kmer7"] = n / (time.perf_counter() - t)
    t = time.perf_counter()
    regional.run_regional_corr_calc(types.SimpleNamespace(pred_file=sl, window_size=100000, ratio_cutoff=0.2, n_class=4,
                                                          out_prefix=os.path.join(d, "rr")))
    out["regional100k"] = n / (time.perf_counter() - t)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=50_000_000)
    ap.add_argument("--dir", default=os.path.join(tempfile.gettempdir(), "mural_bench_tables"))
    ap.add_argument("--chunk-bytes", type=int, default=64 << 20)
    ap.add_argument("--tools", default="scale,calc_scaling_factor,kmer7,regional100k")
    ap.add_argument("--inputs", default="plain,gz")
    ap.add_argument("--reference", type=int, default=0, help="rows of the reference scripts' host run (0: skip)")
    a = ap.parse_args()
    t = time.perf_counter()
    table, fasta = write_inputs(a.dir, a.rows)
    print(json.dumps({"inputs_s": round(time.perf_counter() - t, 1), "rows": a.rows, "plain_bytes": os.path.getsize(table),
                      "gz_bytes": os.path.getsize(table + ".gz")}), flush=True)
    if a.reference:
        print(json.dumps({"reference_host_rows_per_s": reference_rate(table, fasta, a.dir, a.reference), "rows": a.reference}), flush=True)
        return
    for kind in a.inputs.split(","):
        path = table + (".gz" if kind == "gz" else "")
        for tool in a.tools.split(","):
            sec, timing = run(tool, path, fasta, a.dir, a.chunk_bytes)
            rec = {"tool": tool, "input": kind, "seconds": round(sec, 3), "rows_per_s": round(a.rows / sec)}
            rec.update({k: (round(v, 3) if isinstance(v, float) else v) for k, v in timing.items()})
            print(json.dumps(rec), flush=True)


if __name__ == "__main__":
    main()
