"""Prediction over a region against prediction from a BED file of the same sites, file to file, and the site enumeration alone
(DESIGN.md section 3.7):  python tools/bench_regions.py [--bases N] [--repeats K]

One synthetic chromosome (i.i.d. uniform ACGT, 50 Mbp by default), the shipped Homo_sapiens/SNV/AT weights, focal A (every A a '+'
site, every T a '-' site).  The BED is written from the device enumeration (one row per site, label 0) and stays in the page cache:
it is written, and read once by the warm-up run, right before the timed runs.  The two paths alternate, --repeats timed runs each
after one warm-up run each; the two tables must be byte-identical.  A third leg in the same rounds is the regions run with observed
mutations: a synthetic list with every 100th site (1 % of the rows, classes 1 .. 3, a BED in the same directory,
read by every run), whose table must carry exactly those labels.  Prints one JSON line."""
import ctypes as C
import json
import os
import shutil
import statistics
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch  # noqa: E402

from bench import shipped_snv_model  # noqa: E402
from mural_amd import _lib  # noqa: E402
from mural_amd.data import PackedGenome, pack_fasta_record, scan_fasta  # noqa: E402
from mural_amd.predict import HipShardForward, TsvSink, _name_table, _tsv_struct, predict_bed_sharded, predict_regions_sharded  # noqa: E402


def write_inputs(work, device, bases, name="chr1", seed=7):
    """FASTA of one random chromosome; BED6 of its A/T sites from the device enumeration (text by the library's row formatter)."""
    fa, bed = os.path.join(work, "genome.fa"), os.path.join(work, "sites.bed")
    gen = torch.Generator(device=device).manual_seed(seed)
    seq = torch.tensor(list(b"ACGT"), dtype=torch.uint8, device=device)[torch.randint(0, 4, (bases,), device=device, generator=gen)]
    whole = bases // 60 * 60
    lines = torch.cat([seq[:whole].view(-1, 60), torch.full((whole // 60, 1), 10, dtype=torch.uint8, device=device)], dim=1)
    with open(fa, "wb") as f:
        f.write(b">" + name.encode() + b"\n" + lines.cpu().numpy().tobytes())
        if whole < bases:
            f.write(seq[whole:].cpu().numpy().tobytes() + b"\n")
    del seq, lines
    packed, mask, n, amb = pack_fasta_record(fa, scan_fasta(fa)[0])
    genome = PackedGenome(packed, mask, n, device, amb)
    pos, strand = genome.enumerate_sites(0, n, "A")
    end, label = pos + 1, torch.zeros(pos.shape[0], dtype=torch.float32, device=device)
    lib = _lib.lib()
    t = _tsv_struct(_name_table([name]), 1, None, 0, 0, 0, 0, None, False, 0, 0, None, 0)
    t.layout = 1                                           # BED6: chrom start end . label strand
    piece = 1 << 21
    text = torch.empty(piece * int(lib.mural_tsv_row_bound(C.byref(t))), dtype=torch.uint8, device=device)
    count = torch.zeros(1, dtype=torch.int64, device=device)
    ws = torch.empty(int(lib.mural_tsv_format_workspace_bytes(piece)) + 256, dtype=torch.uint8, device=device)
    with open(bed, "wb") as b:
        for r0 in range(0, pos.shape[0], piece):
            t.start, t.end, t.strand, t.label = pos[r0:].data_ptr(), end[r0:].data_ptr(), strand[r0:].data_ptr(), label[r0:].data_ptr()
            t.n = min(piece, pos.shape[0] - r0)
            _lib.check(lib.mural_tsv_format_device(C.byref(t), text.data_ptr(), text.numel(), count.data_ptr(), ws.data_ptr(), ws.numel(),
                                                  _lib.current_stream_ptr(device)))
            b.write(text[:int(count.item())].cpu().numpy().tobytes())
    # the observed side of the labelled leg: every 100th site, its own strand, classes 1 .. 3
    mut = os.path.join(work, "mutations.bed")
    m_pos, m_strand = pos[::100].cpu().numpy(), strand[::100].cpu().numpy()
    with open(mut, "w") as f:
        f.write("".join(f"{name}\t{p}\t{p + 1}\t.\t{1 + i % 3}\t{'+-'[st]}\n" for i, (p, st) in enumerate(zip(m_pos.tolist(), m_strand.tolist()))))
    return fa, bed, mut, len(m_pos), genome, int(pos.shape[0])


def time_enumeration(genome, repeats):
    """Milliseconds (device events) of the counting pass and of count + emit over the whole record, per repeat."""
    count_ms, both_ms = [], []
    for i in range(repeats + 1):
        ev = [torch.cuda.Event(enable_timing=True) for _ in range(3)]
        ev[0].record()
        scan = genome.scan_sites(0, genome.length, "A")
        ev[1].record()
        total = scan.total                                 # (the read-back every caller needs to size the outputs)
        genome.emit_sites(scan, 0, total)
        ev[2].record()
        torch.cuda.synchronize()
        if i:                                              # (the first round is the warm-up)
            count_ms.append(ev[0].elapsed_time(ev[1]))
            both_ms.append(ev[0].elapsed_time(ev[2]))
    return count_ms, both_ms


def spread(xs):
    return {"median": statistics.median(xs), "min": min(xs), "max": max(xs), "all": xs}


def main(argv):
    bases = int(argv[argv.index("--bases") + 1]) if "--bases" in argv else 50_000_000
    repeats = int(argv[argv.index("--repeats") + 1]) if "--repeats" in argv else 3
    if not torch.cuda.is_available():
        raise SystemExit("bench_regions needs a HIP device")
    device = torch.device("cuda", 0)
    model, r, order, _ = shipped_snv_model(device)
    shm = "/dev/shm" if os.path.isdir("/dev/shm") and os.access("/dev/shm", os.W_OK) and shutil.disk_usage("/dev/shm").free > 100 * bases else None
    with tempfile.TemporaryDirectory(prefix="mural_regions_", dir=shm) as work:
        fa, bed, mut, listed, genome, rows = write_inputs(work, device, bases)
        count_ms, both_ms = time_enumeration(genome, max(repeats, 5))
        del genome
        torch.cuda.empty_cache()
        out = {"regions": os.path.join(work, "regions.tsv"), "bed": os.path.join(work, "bed.tsv"), "labelled": os.path.join(work, "labelled.tsv")}

        def run(path):
            split = {}
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            fwd = HipShardForward(model, fa, r, order, device=device, reuse=True)
            if path == "regions":
                n = predict_regions_sharded(fwd, "chr1", "A", sink=TsvSink(out[path]), collect=False, timings=split)
            elif path == "labelled":
                n = predict_regions_sharded(fwd, "chr1", "A", sink=TsvSink(out[path]), collect=False, timings=split, mutations=mut,
                                            strict_mutations=True)
                assert split["mutations"] == {"in_regions": listed, "matched": listed, "unmatched": 0}, split["mutations"]
            else:
                n = predict_bed_sharded(fwd, bed, sink=TsvSink(out[path]), collect=False, timings=split)
            torch.cuda.synchronize()
            dt = time.perf_counter() - t0
            assert n == rows, (path, n, rows)
            return dt, {k: v for k, v in split.items() if isinstance(v, float)}

        seconds, splits = {"regions": [], "bed": [], "labelled": []}, {}
        for i in range(repeats + 1):
            for path in ("bed", "regions", "labelled"):
                dt, split = run(path)
                if i:                                      # (round 0 warms kernels, allocator pools and the page cache of the inputs)
                    seconds[path].append(dt)
                    splits[path] = split
        with open(out["regions"], "rb") as a, open(out["bed"], "rb") as b:
            identical = all(x == y for x, y in zip(iter(lambda: a.read(1 << 24), b""), iter(lambda: b.read(1 << 24), b""))) \
                and os.path.getsize(out["regions"]) == os.path.getsize(out["bed"])
        # the labelled table: the same rows, the list's labels per class (the table tools' device parser counts them)
        from mural_amd.tables import regional_table
        counts = regional_table(out["labelled"], 100_000, 4)[1][:, :5].sum(axis=0).astype(int).tolist()
        want = [rows, rows - listed] + [len(range(c, listed, 3)) for c in range(3)]
        identical = identical and counts == want and os.path.getsize(out["labelled"]) == os.path.getsize(out["regions"])
        sizes = {"fasta_bytes": os.path.getsize(fa), "bed_bytes": os.path.getsize(bed), "table_bytes": os.path.getsize(out["bed"])}
    rate = {p: spread([rows / s for s in seconds[p]]) for p in seconds}
    res = {"workload": "one chromosome of %d bases, focal A, Homo_sapiens/SNV/AT weights, file to file" % bases, "rows": rows, **sizes,
           "repeats": repeats, "tables_identical": identical, "labelled_table_counts": counts,
           "enumeration_ms_per_100Mbp": {"count": spread([m * 1e8 / bases for m in count_ms]),
                                         "count_readback_emit": spread([m * 1e8 / bases for m in both_ms])},
           "regions_rows_per_s": rate["regions"], "bed_rows_per_s": rate["bed"],
           "regions_over_bed": rate["regions"]["median"] / rate["bed"]["median"],
           "labelled_rows_per_s": rate["labelled"], "listed_mutations": listed,
           "labelled_over_regions": rate["labelled"]["median"] / rate["regions"]["median"],
           "regions_seconds": seconds["regions"], "bed_seconds": seconds["bed"], "labelled_seconds": seconds["labelled"],
           "split_seconds": splits,
           "files_in": "/dev/shm" if shm else "the temp directory"}
    print(json.dumps(res))
    if not identical:
        raise SystemExit("the region table differs from the BED table, or the labelled table does not carry the list's labels")


if __name__ == "__main__":
    main(sys.argv[1:])
