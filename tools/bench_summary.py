"""Genome summaries in flight against the table route to the same numbers:
  python tools/bench_summary.py [--bases N] [--indel_bases N] [--repeats K] [--legs a,b,..]

One synthetic chromosome (i.i.d. uniform ACGT, 50 Mbp by default), the shipped Homo_sapiens/SNV/AT weights, focal A, sites enumerated on
the device (predict_regions_sharded), files in /dev/shm.  Twenty-five legs (--legs picks some by name; the agreement checks need their legs),
alternating, --repeats timed runs each after one warm-up run each:
  a  table     TsvSink alone: the '%.4g' table, nothing else
  b  summary   SummarySink alone, 100 kb + 1 kb windows and the scaling totals: no text
  c  tee       TeeSink of both
  d  tools     the route to b's numbers without this sink: leg a's table, then prob_sum_file + regional_table (100 kb, 1 kb) on it
  e  kmers       leg b with kmers=(3, 5, 7) as well: the k-mer tables reduced from the resident chromosome
  f  kmer_tools  the route to e's k-mer tables without the sink: leg a's table, then tables.kmer_table x 3 on it (the FASTA packed again)
  g  motifs      leg b with motifs=(3, 5, 7) as well: the motif tables reduced from the resident chromosome
  h  motif_tools the route to g's motif tables without the sink: leg a's table, then tables.motif_table x 3 on it
  i  calib       leg b with calibration=True as well: loss and calibration metrics reduced in flight; the
                 comparison is leg b, the same run without it
  j  calib_fit   leg b with fit_calibrator="FullDiri" and a synthetic mutation list (every 100th site, classes 1 .. 3 in turn) so that
                 every class occurs: the rows retained on the device, the fit and the metrics after it at close(); reports close()
                 seconds, the retained bytes and the leg's peak device memory
  k  annot       leg b with annotations= as well: expected and observed mutations per name of a synthetic
                 annotation file -- 20 000 names x 10 intervals of 150 bp spread over the chromosome, 5 % of the names overlapping a
                 neighbour --; the comparison is leg b, the same run without it
  l  annot_tools the route to k's table without the sink: leg a's table, then tables.annotation_table on it
  m  sim100      leg k with simulate=100, simulate_seed=1 as well: the counts of 100 mutation sets drawn from the
                 rates per name; the comparison is leg k, the same run without it
  n  sim1000     leg k with simulate=1000 (a table of 240 MB, below the sink's cap)
  o  conseq       leg b with transcripts= as well: expected and observed mutations per transcript by consequence,
                  leg k's 200 000 pieces regrouped into 20 000 ten-exon transcripts on alternating strands; the comparisons are leg b, the
                  same run without it, and leg k
  p  conseq_tools the route to o's table without the sink: leg a's table, then tables.consequence_table on it (the FASTA packed again)
  q  conseq_sim100  leg o with simulate=100, simulate_seed=1, simulate_transcripts=True as well: the counts of 100
                  mutation sets per transcript and consequence; the comparison is leg o, the same run without it
  r  conseq_sim1000 leg o with simulate=1000 (a table of 400 MB, below the sink's cap)
  s  conseq_struct  leg o with transcript_structure=True as well: the structure table of the same transcripts --
                  their exons and the coding introns between them --; the comparison is leg o, the same run without it
  t  struct_sim100  leg s with simulate=100, simulate_seed=1, simulate_transcripts=True, simulate_structure=True as well (DESIGN.md section
                  3.24): the counts of 100 mutation sets per transcript, structure bin and LoF; the comparisons are leg s and leg q
  u  struct_sim1000 leg s with simulate=1000 (tables of 720 MB and 400 MB, each below the sink's cap)
  v  indel         an INDEL-row run: a second synthetic chromosome of --indel_bases bases (5 Mbp by default),
                  the shipped Homo_sapiens/INDEL/deletion_start weights (tests/golden), every A/C/G/T position a row of 8 classes,
                  SummarySink with the 100 kb + 1 kb windows alone
  w  indel_struct  leg v with indel_transcripts= as well: ten-exon transcripts of 2 500 bases each on alternating strands (exons of 150
                  bases, introns of 100), indel_kind="deletion_start"; the comparison is leg v, the same run without it: the difference
                  of the medians beside leg v's own repeat spread.  With leg w the entry alone, mural_summary_txindel_rows over the
                  whole chromosome's rows in one call, is timed under HIP events for each of the three kinds (the rows' probabilities
                  uniform random: the entry's work does not depend on them)
  x  indel_struct_sim100   leg w with simulate=100, simulate_seed=, simulate_indel_structure=True
  y  indel_struct_sim1000  the same at 1000 replicates; with leg w, mural_simulate_txindel_rows alone on leg w's part under HIP events,
                  each of the three kinds at 100 and 1000 replicates; close() alone is timed in every INDEL leg
Prints one JSON line; the summary of leg b must agree with leg d's, leg e's k-mer tables with leg f's, leg g's motif tables with leg
h's, leg k's annotation table with leg l's and leg o's consequence table with leg p's, within the table's four digits (names, order and
counts exactly)."""
import json
import os
import shutil
import statistics
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import torch  # noqa: E402

from bench import shipped_snv_model  # noqa: E402
from bench_regions import spread, write_inputs  # noqa: E402
from mural_amd import tables  # noqa: E402
from mural_amd.predict import HipShardForward, SummarySink, TeeSink, TsvSink, predict_regions_sharded  # noqa: E402

WINDOWS = (100_000, 1000)
KMERS = (3, 5, 7)
MOTIFS = (3, 5, 7)
LEGS = ("table", "summary", "tee", "tools", "kmers", "kmer_tools", "motifs", "motif_tools", "calib", "calib_fit", "annot", "annot_tools", "sim100", "sim1000",
        "conseq", "conseq_tools", "conseq_sim100", "conseq_sim1000", "conseq_struct", "struct_sim100", "struct_sim1000", "indel", "indel_struct",
        "indel_struct_sim100", "indel_struct_sim1000")
INDEL_LEGS = ("indel", "indel_struct", "indel_struct_sim100", "indel_struct_sim1000")
INDEL_SIM_REPLICATES = {"indel_struct_sim100": 100, "indel_struct_sim1000": 1000}      # leg w's run with simulate_indel_structure=True
INDEL_TX_SPAN = 2500
SIM_REPLICATES = {"sim100": 100, "sim1000": 1000}
CONSEQ_SIM_REPLICATES = {"conseq_sim100": 100, "conseq_sim1000": 1000}
STRUCT_SIM_REPLICATES = {"struct_sim100": 100, "struct_sim1000": 1000}
ANNOT_NAMES, ANNOT_INTERVALS, ANNOT_BP, ANNOT_OVERLAP = 20_000, 10, 150, 0.05


def synthetic_annotations(bases, chrom="chr1"):
    """``tables.read_annotations``' result for ANNOT_NAMES names of ANNOT_INTERVALS intervals of ANNOT_BP bases each, a name per equal
    span of the chromosome; every 20th name is moved half a span up, into its neighbour's intervals."""
    span = bases // ANNOT_NAMES
    step = max(span // ANNOT_INTERVALS, 1)
    every = int(round(1 / ANNOT_OVERLAP))
    rows = []
    for g in range(ANNOT_NAMES):
        at = g * span + (span // 2 if g % every == every - 1 else 0)
        rows += [(at + j * step, at + j * step + ANNOT_BP, "set%05d" % g) for j in range(ANNOT_INTERVALS)]
    return tables.read_annotations({chrom: rows})


def synthetic_transcripts(bases, chrom="chr1", structure=False, names=ANNOT_NAMES):
    """``tables.read_transcripts``' result (`structure`: ``tables.read_transcript_structure``'s) for the intervals of ``synthetic_annotations`` as ANNOT_NAMES transcripts of ANNOT_INTERVALS
    exons each, all of it CDS, on alternating strands."""
    import io
    span = bases // names
    step = max(span // ANNOT_INTERVALS, 1)
    every = int(round(1 / ANNOT_OVERLAP))
    lines = []
    for g in range(names):
        at = g * span + (span // 2 if g % every == every - 1 else 0)
        end = at + (ANNOT_INTERVALS - 1) * step + ANNOT_BP
        lines.append("\t".join([chrom, str(at), str(end), "tx%05d" % g, "0", "+-"[g & 1], str(at), str(end), "0", str(ANNOT_INTERVALS),
                                ",".join([str(ANNOT_BP)] * ANNOT_INTERVALS), ",".join(str(j * step) for j in range(ANNOT_INTERVALS))]))
    return (tables.read_transcript_structure if structure else tables.read_transcripts)(io.StringIO("\n".join(lines) + "\n"))


def shipped_indel_model(device, name="indel_pretrained_human_deletion_start.npz"):
    """UNet_Small with the shipped Homo_sapiens/INDEL/deletion_start weights (they travel inside the parity fixture tests/golden/<name>);
    (model, distal_radius, n_class)."""
    from mural_amd.model import model_choice
    from tests import _util as U
    fx = U.load(name)
    R, C, k, n_class, rev = [int(v) for v in fx["hp"]]
    model = model_choice(0, dict(CNN_out_channels=C, CNN_kernel_size=k, down_list=[int(d) for d in fx["down"]], use_reverse=bool(rev)),
                         dict(n_class=n_class), "indel")
    model.load_state_dict(U.indel_state_for(fx, U.indel_oracle_from_hp(fx["hp"], fx["down"])), strict=True)
    return model.to(device).eval(), R, n_class


def indel_legs(legs, device, bases, repeats, shm):
    """Legs v and w, alternating, and the entry alone under HIP events: the "indel_structure" block of the result."""
    import numpy as np
    from mural_amd.summaries import simulate_txindel_rows_device, txindel_rows_device
    model, R, n_class = shipped_indel_model(device)
    with tempfile.TemporaryDirectory(prefix="mural_summary_indel_", dir=shm) as work:
        fa = write_inputs(work, device, bases)[0]
        torch.cuda.empty_cache()
        tx = synthetic_transcripts(bases, structure=True, names=max(bases // INDEL_TX_SPAN, 1))
        seconds, kept, rows, close_seconds = {leg: [] for leg in legs}, {}, None, {}

        def run(leg):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            fwd = HipShardForward(model, fa, 5, 3, distal_radius=R, model_type="indel", device=device, poisson=False)
            extra = dict(indel_transcripts=tx, indel_kind="deletion_start", genome=fwd.genome, transcript_labels=False) if leg != "indel" else {}
            if leg in INDEL_SIM_REPLICATES:
                extra.update(simulate=INDEL_SIM_REPLICATES[leg], simulate_seed=7, simulate_indel_structure=True)
            summary = SummarySink(windows=WINDOWS, **extra)
            plain_close = summary.close

            def close_timed():      # close() alone, of every run: the read-back and the host's share
                torch.cuda.synchronize()
                t1 = time.perf_counter()
                plain_close()
                torch.cuda.synchronize()
                close_seconds.setdefault(leg, []).append(time.perf_counter() - t1)
            summary.close = close_timed
            n = predict_regions_sharded(fwd, "chr1", "ANY", model_type="indel", sink=summary, collect=False)
            torch.cuda.synchronize()
            kept[leg] = summary.result()
            return time.perf_counter() - t0, n

        for i in range(repeats + 1):
            for leg in legs:
                dt, rows = run(leg)
                if i:
                    seconds[leg].append(dt)
    out = {"bases": bases, "rows": rows, "classes": n_class, "transcripts": len(tx[0]), "repeats": repeats, "seconds": seconds,
           "rows_per_s": {leg: spread([rows / v for v in seconds[leg]]) for leg in legs},
           "close_seconds": {leg: spread(v[1:]) for leg, v in close_seconds.items() if len(v) > 1}}
    if {"indel", "indel_struct"} <= set(legs):
        plain, with_it = seconds["indel"], seconds["indel_struct"]
        out["indel_struct_minus_indel_seconds"] = statistics.median(with_it) - statistics.median(plain)
        out["indel_repeat_spread_seconds"] = max(plain) - min(plain)
        out["indel_struct_over_indel"] = statistics.median(plain) / statistics.median(with_it)
    if "indel_struct" in legs:
        table, counters = kept["indel_struct"]["indel_structure"][1:]
        out["rows_counted"], out["expected_by_bin"] = int(counters[:, 0].sum()), (table[:, :, 1].sum(axis=0) / float(1 << 31)).tolist()
        # the entry alone: every position of the chromosome a row, one call, HIP events around it
        k, n_tx, features, segments = n_class, len(tx[0]), tx[3]["chr1"], tx[2]["chr1"]
        links, class_len = tables.structure_links(features), tables.check_indel_lengths(None, k)
        gen = torch.Generator(device=device).manual_seed(3)
        prob = torch.rand((bases, k), device=device, generator=gen) / k
        start, label = torch.arange(bases, dtype=torch.int64, device=device), torch.zeros(bases, dtype=torch.int32, device=device)
        out["entry_ms"] = {}
        for kind, what in enumerate(tables.INDEL_KINDS):
            acc, ms = tables._indel_structure_acc(n_tx, device), []
            for i in range(repeats + 1):
                a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                a.record()
                txindel_rows_device(acc, "chr1", segments, features, links, n_tx, kind, 1, class_len, bases, device, prob=prob.data_ptr(),
                                    prob_f64=0, prob_stride=k, start=start.data_ptr(), label=label.data_ptr(), label_kind=1, n=bases, n_class=k)
                b.record()
                b.synchronize()
                if i:
                    ms.append(a.elapsed_time(b))
            assert int(acc["status"].item()) == 0
            out["entry_ms"][what] = spread(ms)
        out["entry_rows"] = bases
        # the simulation's entry alone on the same part, each kind at 100 and 1000 replicates
        out["simulate_entry_ms"] = {}
        strand, status = torch.zeros(bases, dtype=torch.uint8, device=device), torch.zeros(1, dtype=torch.int32, device=device)
        for n_rep in sorted(set(INDEL_SIM_REPLICATES.values())):
            sim = torch.zeros(n_tx * 10 * n_rep, dtype=torch.int32, device=device)
            for kind, what in enumerate(tables.INDEL_KINDS):
                ms = []
                for i in range(repeats + 1):
                    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                    a.record()
                    simulate_txindel_rows_device(sim, status, acc, "chr1", n_tx, kind, 1, class_len, bases, device, n_rep, 7, prob=prob.data_ptr(),
                                                 prob_f64=0, prob_stride=k, start=start.data_ptr(), strand=strand.data_ptr(), n=bases, n_class=k)
                    b.record()
                    b.synchronize()
                    if i:
                        ms.append(a.elapsed_time(b))
                out["simulate_entry_ms"][f"{what}_R{n_rep}"] = spread(ms)
        assert int(status.item()) == 0
    return out


def main(argv):
    indel_bases = int(argv[argv.index("--indel_bases") + 1]) if "--indel_bases" in argv else 5_000_000
    bases = int(argv[argv.index("--bases") + 1]) if "--bases" in argv else 50_000_000
    repeats = int(argv[argv.index("--repeats") + 1]) if "--repeats" in argv else 3
    legs = tuple(argv[argv.index("--legs") + 1].split(",")) if "--legs" in argv else LEGS
    if set(legs) - set(LEGS):
        raise SystemExit(f"--legs: one of {LEGS}")
    if not torch.cuda.is_available():
        raise SystemExit("bench_summary needs a HIP device")
    device = torch.device("cuda", 0)
    indel = [leg for leg in legs if leg in INDEL_LEGS]
    legs = tuple(leg for leg in legs if leg not in INDEL_LEGS)
    shm_ok = os.path.isdir("/dev/shm") and os.access("/dev/shm", os.W_OK)
    indel_result = indel_legs(indel, device, indel_bases, repeats, "/dev/shm" if shm_ok else None) if indel else None
    if not legs:
        print(json.dumps({"indel_structure": indel_result}))
        return
    model, r, order, _ = shipped_snv_model(device)
    n_class = model.n_class
    shm = "/dev/shm" if os.path.isdir("/dev/shm") and os.access("/dev/shm", os.W_OK) and shutil.disk_usage("/dev/shm").free > 100 * bases else None
    with tempfile.TemporaryDirectory(prefix="mural_summary_", dir=shm) as work:
        fa, _, mutations, _, genome, rows = write_inputs(work, device, bases)      # (its mutation list: every 100th site, classes 1 .. 3)
        del genome
        torch.cuda.empty_cache()
        out = os.path.join(work, "table.tsv")
        kept, closes = {}, {}
        annot = synthetic_annotations(bases) if {"annot", "annot_tools", "sim100", "sim1000"} & set(legs) else None

        transcripts = synthetic_transcripts(bases) if {"conseq", "conseq_tools", *CONSEQ_SIM_REPLICATES} & set(legs) else None

        structure = synthetic_transcripts(bases, structure=True) if {"conseq_struct", *STRUCT_SIM_REPLICATES} & set(legs) else None

        def run(leg):
            split, extra = {}, {}
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            fwd = HipShardForward(model, fa, r, order, device=device, reuse=True)
            summary = SummarySink(windows=WINDOWS) if leg in ("summary", "tee") else None
            if leg == "kmers":
                summary = SummarySink(windows=WINDOWS, kmers=KMERS, genome=fwd.genome)
            if leg == "motifs":
                summary = SummarySink(windows=WINDOWS, motifs=MOTIFS, genome=fwd.genome)
            if leg == "calib":
                summary = SummarySink(windows=WINDOWS, calibration=True)
            if leg == "annot":
                summary = SummarySink(windows=WINDOWS, annotations=annot)
            if leg in SIM_REPLICATES:
                summary = SummarySink(windows=WINDOWS, annotations=annot, simulate=SIM_REPLICATES[leg], simulate_seed=1, simulate_labels=False)
            if leg == "conseq":
                summary = SummarySink(windows=WINDOWS, transcripts=transcripts, genome=fwd.genome, transcript_labels=False)
            if leg == "conseq_struct":
                summary = SummarySink(windows=WINDOWS, transcripts=structure, genome=fwd.genome, transcript_labels=False,
                                      transcript_structure=True)
            if leg in STRUCT_SIM_REPLICATES:
                summary = SummarySink(windows=WINDOWS, transcripts=structure, genome=fwd.genome, transcript_labels=False,
                                      transcript_structure=True, simulate=STRUCT_SIM_REPLICATES[leg], simulate_seed=1,
                                      simulate_transcripts=True, simulate_structure=True)
            if leg in CONSEQ_SIM_REPLICATES:
                summary = SummarySink(windows=WINDOWS, transcripts=transcripts, genome=fwd.genome, transcript_labels=False,
                                      simulate=CONSEQ_SIM_REPLICATES[leg], simulate_seed=1, simulate_transcripts=True)
            if leg in ("summary", "annot", "sim100", "sim1000", "conseq", "conseq_struct", *CONSEQ_SIM_REPLICATES, *STRUCT_SIM_REPLICATES) and {"annot", "conseq"} & set(legs):      # close() alone, of every run: where leg k's host work would be
                plain_close = summary.close

                def close_timed():
                    torch.cuda.synchronize()
                    t1 = time.perf_counter()
                    plain_close()
                    torch.cuda.synchronize()
                    closes.setdefault(leg, []).append(time.perf_counter() - t1)
                summary.close = close_timed
            if leg == "calib_fit":
                torch.cuda.reset_peak_memory_stats(device)
                summary = SummarySink(windows=WINDOWS, fit_calibrator="FullDiri")
                close = summary.close

                def timed_close():
                    torch.cuda.synchronize()
                    t1 = time.perf_counter()
                    extra["retained_bytes"] = float(sum(p.numel() * p.element_size() + y.numel() for p, y in summary._reducers["calibration"].fit_blocks))
                    close()
                    torch.cuda.synchronize()
                    extra["close"] = time.perf_counter() - t1
                summary.close = timed_close
            sink = {"calib": lambda: summary, "calib_fit": lambda: summary, "table": lambda: TsvSink(out), "tools": lambda: TsvSink(out), "summary": lambda: summary, "kmers": lambda: summary,
                    "tee": lambda: TeeSink(TsvSink(out), summary), "kmer_tools": lambda: TsvSink(out), "motifs": lambda: summary,
                    "motif_tools": lambda: TsvSink(out), "annot": lambda: summary, "annot_tools": lambda: TsvSink(out), "sim100": lambda: summary,
                    "sim1000": lambda: summary, "conseq": lambda: summary, "conseq_tools": lambda: TsvSink(out),
                    "conseq_sim100": lambda: summary, "conseq_sim1000": lambda: summary, "conseq_struct": lambda: summary,
                    "struct_sim100": lambda: summary, "struct_sim1000": lambda: summary}[leg]()
            n = predict_regions_sharded(fwd, "chr1", "A", sink=sink, collect=False, timings=split,
                                        **(dict(mutations=mutations) if leg == "calib_fit" else {}))
            torch.cuda.synchronize()
            extra["predict"] = time.perf_counter() - t0
            if leg == "calib_fit":
                extra["peak_device_bytes"] = float(torch.cuda.max_memory_allocated(device))
            if leg == "tools":
                t1 = time.perf_counter()
                total, n_sites = tables.prob_sum_file(out, n_class)
                extra["prob_sum_file"] = time.perf_counter() - t1
                wins = {}
                for W in WINDOWS:
                    t1 = time.perf_counter()
                    wins[W] = tables.regional_table(out, W, n_class)
                    extra["regional_table_%d" % W] = time.perf_counter() - t1
                kept["tools"] = {"prob_sum": total, "n_sites": n_sites, "windows": wins}
            if leg == "kmer_tools":
                kept["kmer_tools"] = {}
                for k in KMERS:
                    t1 = time.perf_counter()
                    kept["kmer_tools"][k] = tables.kmer_table(out, fa, k, n_class, "snv")
                    extra["kmer_table_%d" % k] = time.perf_counter() - t1
            if leg == "motif_tools":
                kept["motif_tools"] = {}
                for m in MOTIFS:
                    t1 = time.perf_counter()
                    kept["motif_tools"][m] = tables.motif_table(out, fa, m, n_class, "snv")
                    extra["motif_table_%d" % m] = time.perf_counter() - t1
            if leg == "annot_tools":
                t1 = time.perf_counter()
                kept["annot_tools"] = tables.annotation_table(out, annot, n_class)
                extra["annotation_table"] = time.perf_counter() - t1
            if leg == "conseq_tools":
                t1 = time.perf_counter()
                kept["conseq_tools"] = tables.consequence_table(out, transcripts, fa)
                extra["consequence_table"] = time.perf_counter() - t1
            dt = time.perf_counter() - t0
            assert n == rows, (leg, n, rows)
            if summary is not None:
                kept[leg] = summary.result()
            return dt, dict({k: v for k, v in split.items() if isinstance(v, float)}, **extra)

        seconds, splits = {leg: [] for leg in legs}, {}
        for i in range(repeats + 1):
            for leg in legs:
                dt, split = run(leg)
                if i:                                      # (round 0 warms kernels, allocator pools and the page cache)
                    seconds[leg].append(dt)
                    splits[leg] = split
        table_bytes = os.path.getsize(out) if os.path.exists(out) else 0
    agree, k = True, 1 + n_class
    if {"summary", "tools", "tee"} <= set(legs):
        a, d = kept["summary"], kept["tools"]
        agree = a["n_sites"] == d["n_sites"] and abs(a["prob_sum"] - d["prob_sum"]) <= 5e-4 * a["prob_sum"] and kept["tee"]["n_sites"] == a["n_sites"]
        for W in WINDOWS:
            (ka, ta), (kd, td) = a["windows"][W], d["windows"][W]
            agree = agree and ka == kd and (ta[:, :k] == td[:, :k]).all() and bool((abs(ta[:, k:] - td[:, k:]) <= 5e-4 * ta[:, k:]).all())
            agree = agree and bool((kept["tee"]["windows"][W][1] == ta).all())      # bit for bit, with or without the table beside it
    if {"kmers", "kmer_tools"} <= set(legs):
        for kk in KMERS:
            (na, ta), (nd, td) = kept["kmers"]["kmers"][kk], kept["kmer_tools"][kk]
            agree = agree and na == nd and bool((ta[:, :k] == td[:, :k]).all()) and bool((abs(ta[:, k:] - td[:, k:]) <= 5e-4 * ta[:, k:]).all())
    if {"motifs", "motif_tools"} <= set(legs):
        for m in MOTIFS:
            (na, ta), (nd, td) = kept["motifs"]["motifs"][m], kept["motif_tools"][m]
            agree = agree and na == nd and bool((ta[:, :k] == td[:, :k]).all()) and bool((abs(ta[:, k:] - td[:, k:]) <= 5e-4 * ta[:, k:]).all())
    if {"annot", "annot_tools"} <= set(legs):
        (na, ma, ta), (nd, md, td) = kept["annot"]["annotations"], kept["annot_tools"]
        agree = agree and na == nd and bool((ma == md).all()) and bool((ta[:, :k] == td[:, :k]).all())
        agree = agree and bool((abs(ta[:, k:] - td[:, k:]) <= 5e-4 * ta[:, k:]).all()) and bool(ta[:, 0].sum() > 0)
    if {"conseq", "conseq_tools"} <= set(legs):
        (na, _, ta), (nd, _, td) = kept["conseq"]["consequences"], kept["conseq_tools"]
        counts, sums = [0, 1, 2, 4, 6, 8, 10], [3, 5, 7, 9, 11]
        agree = agree and na == nd and bool((ta[:, counts] == td[:, counts]).all()) and bool(ta[:, 0].sum() > 0)
        agree = agree and bool((abs(ta[:, sums] - td[:, sums]) <= 5e-4 * ta[:, sums]).all())
    if {"conseq", "conseq_struct"} <= set(legs):      # the consequence table beside the structure table is leg o's, and bins 7 + 8 are its rows
        (na, _, ta), (ns, _, ts) = kept["conseq"]["consequences"], kept["conseq_struct"]["consequences"]
        struct = kept["conseq_struct"]["transcript_structure"][1]
        agree = agree and na == ns and bool((ta == ts).all()) and bool((struct[:, 7:9, 0].sum(axis=1) == ta[:, [2, 4, 6, 8, 10]].sum(axis=1)).all())
    for leg in STRUCT_SIM_REPLICATES:      # bins 7 + 8 of the structure draws are the five bins of the consequence draws, replicate by replicate
        if leg in kept:
            sim, conseq_sim = kept[leg]["structure_simulation"][1], kept[leg]["consequence_simulation"][1]
            agree = agree and bool((sim[:, 7].astype("int64") + sim[:, 8] == conseq_sim.astype("int64").sum(axis=1)).all()) and bool(sim.any())
    rate = {leg: spread([rows / s for s in seconds[leg]]) for leg in legs}
    med = {leg: rate[leg]["median"] for leg in legs}
    sec = {leg: statistics.median(seconds[leg]) for leg in legs}
    ratio = lambda x, y, of: of[x] / of[y] if x in of and y in of else None      # noqa: E731
    res = {"workload": "one chromosome of %d bases, focal A, Homo_sapiens/SNV/AT weights, sites enumerated on the device" % bases,
           "rows": rows, "table_bytes": table_bytes, "windows": list(WINDOWS), "kmers": list(KMERS), "repeats": repeats,
           "summaries_agree": bool(agree), "rows_per_s": rate, "summary_over_table": ratio("summary", "table", med),
           "tee_over_table": ratio("tee", "table", med), "tools_over_summary_seconds": ratio("tools", "summary", sec),
           "kmers_over_summary": ratio("kmers", "summary", med), "kmer_tools_over_kmers_seconds": ratio("kmer_tools", "kmers", sec),
           "motifs": list(MOTIFS), "motifs_over_summary": ratio("motifs", "summary", med),
           "motif_tools_over_motifs_seconds": ratio("motif_tools", "motifs", sec),
           "calib_over_summary": ratio("calib", "summary", med), "calib_fit_over_summary": ratio("calib_fit", "summary", med),
           "annot_over_summary": ratio("annot", "summary", med), "annot_tools_over_annot_seconds": ratio("annot_tools", "annot", sec),
           "sim100_over_annot": ratio("sim100", "annot", med), "sim1000_over_annot": ratio("sim1000", "annot", med),
           "conseq_over_summary": ratio("conseq", "summary", med), "conseq_over_annot": ratio("conseq", "annot", med),
           "conseq_tools_over_conseq_seconds": ratio("conseq_tools", "conseq", sec),
           "consequences": {"transcripts": ANNOT_NAMES, "exons": ANNOT_INTERVALS, "bp": ANNOT_BP,
                            "rows_in_a_cds": float(kept["conseq"]["consequences"][2][:, 0].sum()) if "conseq" in kept else None,
                            "expected": kept["conseq"]["consequences"][2][:, 3:11:2].sum(axis=0).tolist() if "conseq" in kept else None},
           "conseq_sim100_over_conseq": ratio("conseq_sim100", "conseq", med), "conseq_sim1000_over_conseq": ratio("conseq_sim1000", "conseq", med),
           "conseq_struct_over_conseq": ratio("conseq_struct", "conseq", med),
           "struct_sim100_over_conseq_struct": ratio("struct_sim100", "conseq_struct", med),
           "struct_sim1000_over_conseq_struct": ratio("struct_sim1000", "conseq_struct", med),
           "struct_sim100_over_conseq_sim100": ratio("struct_sim100", "conseq_sim100", med),
           "struct_sim1000_over_conseq_sim1000": ratio("struct_sim1000", "conseq_sim1000", med),
           "simulated_structure_draws": {leg: float(kept[leg]["structure_simulation"][1].sum()) for leg in STRUCT_SIM_REPLICATES if leg in kept},
           "simulated_lof": {leg: float(kept[leg]["structure_simulation"][2].sum()) for leg in STRUCT_SIM_REPLICATES if leg in kept},
           "structure_rows": kept["conseq_struct"]["transcript_structure"][2][:, 0].sum().item() if "conseq_struct" in kept else None,
           "simulated_consequence_draws": {leg: float(kept[leg]["consequence_simulation"][1].sum()) for leg in CONSEQ_SIM_REPLICATES if leg in kept},
           "simulated_draws": {leg: float(kept[leg]["simulation"][1].sum()) for leg in SIM_REPLICATES if leg in kept},
           "annotations": {"names": ANNOT_NAMES, "intervals": ANNOT_INTERVALS, "bp": ANNOT_BP,
                           "close_seconds": {leg: v[1:] for leg, v in closes.items()},      # (without the warm-up round's)
                           "rows_in_a_piece": float(kept["annot"]["annotations"][2][:, 0].sum()) if "annot" in kept else None},
           "calibration": {leg: {key: val for key, val in kept[leg]["calibration"].items() if key not in ("per_chromosome", "weights")}
                           for leg in ("calib", "calib_fit") if leg in kept},
           "indel_structure": indel_result, "seconds": seconds, "split_seconds": splits, "files_in": "/dev/shm" if shm else "the temp directory"}
    print(json.dumps(res))
    if not agree:
        raise SystemExit("the in-flight summary differs from the table tools'")


if __name__ == "__main__":
    main(sys.argv[1:])
