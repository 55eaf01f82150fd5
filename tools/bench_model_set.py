"""One regions run with one model per site class against three single-class runs, file to file:
  python tools/bench_model_set.py [--bases N] [--repeats K]

One synthetic chromosome (i.i.d. uniform ACGT, 50 Mbp by default: the one of tools/bench_regions.py), the three shipped
Homo_sapiens/SNV checkpoints (AT, nonCpG, CpG), reuse=False so that the tables can be compared byte for byte.  The legs alternate,
--repeats timed rounds after one warm-up round:
  (a) three single-class runs one after the other (focal A; focal C nonCpG; focal C CpG), each with its own forward: three packs and
      uploads of the chromosome, three tables;
  (b) one ModelSetForward run, focal "SET": one pack and upload, one table of every A/C/G/T base;
  (c) leg (a) followed by the host merge of its three tables by `start` (GNU `sort -m` in the C locale on the tab-separated text: the
      tables are already sorted, so this is a pure merge, the fastest text tool there is for it).  Its seconds are the round's (a)
      seconds plus the merge's.
Tables (b) and (c) must be byte-identical.  Prints one JSON line."""
import json
import os
import shutil
import statistics
import subprocess
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch  # noqa: E402

from bench import shipped_snv_model  # noqa: E402
from mural_amd.predict import HipShardForward, ModelSetForward, TsvSink, predict_regions_sharded  # noqa: E402

CLASSES = {"A": ("A", "all", "snv_pretrained_human_AT.npz"), "nonCpG": ("C", "nonCpG", "snv_pretrained_human_nonCpG.npz"),
           "CpG": ("C", "CpG", "snv_pretrained_human_CpG.npz")}


def write_fasta(work, device, bases, name="chr1", seed=7):
    fa = os.path.join(work, "genome.fa")
    gen = torch.Generator(device=device).manual_seed(seed)
    seq = torch.tensor(list(b"ACGT"), dtype=torch.uint8, device=device)[torch.randint(0, 4, (bases,), device=device, generator=gen)]
    whole = bases // 60 * 60
    lines = torch.cat([seq[:whole].view(-1, 60), torch.full((whole // 60, 1), 10, dtype=torch.uint8, device=device)], dim=1)
    with open(fa, "wb") as f:
        f.write(b">" + name.encode() + b"\n" + lines.cpu().numpy().tobytes())
        if whole < bases:
            f.write(seq[whole:].cpu().numpy().tobytes() + b"\n")
    return fa


def merge_tables(paths, out):
    """Header + the rows of the sorted tables merged by their second column."""
    script = "{ head -n 1 \"$1\"; LC_ALL=C sort -m -t \"$(printf '\\t')\" -k2,2n <(tail -n +2 \"$1\") <(tail -n +2 \"$2\") <(tail -n +2 \"$3\"); } > \"$4\""
    subprocess.run(["bash", "-c", script, "merge"] + list(paths) + [out], check=True)


def same_bytes(a, b):
    if os.path.getsize(a) != os.path.getsize(b):
        return False
    with open(a, "rb") as fa, open(b, "rb") as fb:
        return all(x == y for x, y in zip(iter(lambda: fa.read(1 << 24), b""), iter(lambda: fb.read(1 << 24), b"")))


def spread(xs):
    return {"median": statistics.median(xs), "min": min(xs), "max": max(xs), "all": xs}


def main(argv):
    bases = int(argv[argv.index("--bases") + 1]) if "--bases" in argv else 50_000_000
    repeats = int(argv[argv.index("--repeats") + 1]) if "--repeats" in argv else 3
    if not torch.cuda.is_available():
        raise SystemExit("bench_model_set needs a HIP device")
    device = torch.device("cuda", 0)
    models = {k: shipped_snv_model(device, name) for k, (_, _, name) in CLASSES.items()}
    shm = "/dev/shm" if os.path.isdir("/dev/shm") and os.access("/dev/shm", os.W_OK) and shutil.disk_usage("/dev/shm").free > 400 * bases else None
    with tempfile.TemporaryDirectory(prefix="mural_model_set_", dir=shm) as work:
        fa = write_fasta(work, device, bases)
        torch.cuda.empty_cache()
        single = {k: os.path.join(work, f"single_{k}.tsv") for k in CLASSES}
        set_out, merged = os.path.join(work, "set.tsv"), os.path.join(work, "merged.tsv")

        def member(k, fasta):
            model, r, order, _ = models[k]
            return HipShardForward(model, fasta, r, order, device=device, reuse=False)

        def run_singles():
            rows, seconds, splits = {}, {}, {}
            for k, (focal, context, _) in CLASSES.items():
                split = {}
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                fwd = member(k, fa)
                rows[k] = predict_regions_sharded(fwd, "chr1", focal, context, sink=TsvSink(single[k]), collect=False, timings=split)
                torch.cuda.synchronize()
                seconds[k] = time.perf_counter() - t0
                splits[k] = dict({key: v for key, v in split.items() if isinstance(v, float)}, pack=fwd.seconds["pack"],
                                 pack_wait=fwd.seconds["pack_wait"])
            return rows, seconds, splits

        def run_set():
            split = {}
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            fwd = ModelSetForward({k: member(k, None) for k in CLASSES}, fasta_path=fa)
            n = predict_regions_sharded(fwd, "chr1", "SET", sink=TsvSink(set_out), collect=False, timings=split)
            torch.cuda.synchronize()
            dt = time.perf_counter() - t0
            return n, dt, dict({key: v for key, v in split.items() if isinstance(v, float)}, pack=fwd.seconds["pack"],
                               pack_wait=fwd.seconds["pack_wait"])

        a_s, b_s, merge_s, per_class, splits = [], [], [], {k: [] for k in CLASSES}, {}
        rows = rows_set = None
        for i in range(repeats + 1):
            rows, seconds, split_a = run_singles()
            rows_set, dt_set, split_b = run_set()
            t0 = time.perf_counter()
            merge_tables([single[k] for k in CLASSES], merged)
            dt_merge = time.perf_counter() - t0
            print("round %d: singles %.2f s, set %.2f s, merge %.2f s" % (i, sum(seconds.values()), dt_set, dt_merge), file=sys.stderr, flush=True)
            if i:                                          # (round 0 warms kernels, allocator pools and the page cache)
                a_s.append(sum(seconds.values()))
                b_s.append(dt_set)
                merge_s.append(dt_merge)
                for k in CLASSES:
                    per_class[k].append(seconds[k])
                splits = {"single": split_a, "set": split_b}
        total = sum(rows.values())
        identical = rows_set == total and same_bytes(set_out, merged)
        sizes = {"fasta_bytes": os.path.getsize(fa), "set_table_bytes": os.path.getsize(set_out),
                 "single_table_bytes": {k: os.path.getsize(single[k]) for k in CLASSES}}
    c_s = [a + m for a, m in zip(a_s, merge_s)]
    rate = {"a": spread([total / s for s in a_s]), "b": spread([total / s for s in b_s]), "c": spread([total / s for s in c_s])}
    single_rate = {k: statistics.median(rows[k] / s for s in per_class[k]) for k in CLASSES}
    res = {"workload": "one chromosome of %d bases, every A/C/G/T base, Homo_sapiens/SNV AT + nonCpG + CpG weights, reuse off, file to file" % bases,
           "rows": total, "rows_per_class": rows, **sizes, "repeats": repeats, "tables_identical": identical,
           "a_three_single_runs_rows_per_s": rate["a"], "b_model_set_rows_per_s": rate["b"], "c_singles_plus_merge_rows_per_s": rate["c"],
           "single_rows_per_s": single_rate,      # ((a)'s rate is their row-weighted mean: all rows over the three runs' seconds)
           "b_over_a": rate["b"]["median"] / rate["a"]["median"], "b_over_c": rate["b"]["median"] / rate["c"]["median"],
           "a_seconds": a_s, "b_seconds": b_s, "merge_seconds": merge_s, "c_seconds": c_s, "single_seconds": per_class,
           "split_seconds": splits, "files_in": "/dev/shm" if shm else "the temp directory"}
    print(json.dumps(res))
    if not identical:
        raise SystemExit("the model-set table differs from the merge of the three single-class tables")


if __name__ == "__main__":
    main(sys.argv[1:])
