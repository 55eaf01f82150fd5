"""File-to-file prediction with a reference-style model directory (what `mural_snv predict` / scripts/run_predict.py:58-239 does,
minus its CLI): python tools/predict_files.py MODEL FASTA BED OUT.tsv [--indel] [--poisson] [--no-calibration]

Without a BED file -- the sites are enumerated from the FASTA on the device (mural_amd.predict.predict_regions_sharded):
  python tools/predict_files.py MODEL FASTA OUT.tsv --regions SPEC [--regions SPEC ..] [--focal A|C] [--context all|CpG|nonCpG]
SPEC: chr, chr:start-end (1-based, inclusive) or a BED-like file of regions; --focal defaults to A (with --indel every A/C/G/T
position is a site and --focal / --context do not apply).
  --mutations FILE      with --regions: the observed mutations, a BED of the mutated sites only (chrom start end name score strand,
                        score = mut_type, plain or gzip).  A row on a listed position carries that mut_type, every other row 0 -- the
                        table (and every summary) of a BED with one row per site, without writing that BED
  --strict_mutations    fail when a listed mutation inside the regions lies on no enumerated site (by default they are only counted)

One table from one model per site class (mural_amd.predict.ModelSetForward) -- no MODEL argument, every row by the model of its own base:
  python tools/predict_files.py FASTA OUT.tsv --regions SPEC --model_set CLASS=MODEL_PATH [CLASS=MODEL_PATH ..]
                                [--scale_factors CLASS=F ..] [--mutations FILE] [--no-calibration]
CLASS: A, nonCpG, CpG, or C (= nonCpG and CpG by one model).  Each model directory brings its own .config.pkl and, if present, its
.fdiri_cal.pkl; every model is calibrated / scaled behind its own head, so all of them are or none is.  prob1..3 of a row are the
substitutions of that row's own base (the strand column and the genome say which).  Not with --summary, --focal / --context, --indel.

Genome summaries in flight, in both forms (mural_amd.predict.SummarySink; the numbers `calc_scaling_factor` and `evaluate --window_size`
read back from the table, taken from the probabilities before they are rounded):
  --summary PREFIX  --window_size W [--window_size W ..]   PREFIX.{W/1000}Kb.mut_rates.tsv and .corr.txt per window size
  --summary PREFIX  --kmer_length K [--kmer_length K ..]   PREFIX.{K}-mer.mut_rates.tsv and .corr.txt per k-mer length: the files of
                                                             `evaluate --kmer_only`, the flanks read from the resident chromosome
                                                             (with either or both of --window_size / --kmer_length)
  --summary PREFIX  --motif_length M [M ..]                PREFIX.{M}-motif.mut_rates.tsv and .corr.txt per motif length (odd, 3 and
                                                             more): the files of `evaluate --motif_only` -- every window of M bases that
                                                             holds a site, a motif and its reverse complement in one entry
  --summary PREFIX  --calibration_metrics [--n_bins N]     PREFIX.calibration.txt: rows, NLL, ECE, classwise ECE and Brier score of all
                                                             rows and per chromosome, from the rows' labels (a BED's score column, or
                                                             --regions with --mutations FILE; refused for --regions alone, where every
                                                             label is 0); N bins, 50 by default; alone or with the options above
  --fit_calibrator NAME                                      with --calibration_metrics: fit that calibrator (FullDiri, FullDiriODIR,
                                                             FullDiri1, FullDiri2, VectS, TempS) on the raw softmax of the same run,
                                                             write PREFIX.fdiri_cal.pkl and the metrics after it; the run itself is not
                                                             calibrated (not with --scale_factor, --poisson / --indel's Poisson step;
                                                             a MODEL.fdiri_cal.pkl next to the model needs --no-calibration)
  --summary PREFIX  --annotations BED                      PREFIX.annotation.mut_rates.tsv and .corr.txt: per name (column 4 of the
                                                             BED; the exons of a gene share one) the observed mutations and the
                                                             expected ones, the sums of the probabilities over the rows inside the
                                                             name's intervals; alone or with the options above
  --summary PREFIX  --simulate R --seed S [--write_simulated r ..]
                                                             R mutation sets drawn from the run's probabilities (stateless Philox draws
                                                             keyed by the 64-bit seed S, chromosome, start, strand and replicate; there
                                                             is no default seed).  With --annotations: PREFIX.annotation.sim.tsv, per
                                                             name and class the observed and expected counts, the mean, minimum and
                                                             maximum of the R simulated counts, n_ge / n_le and the empirical p-values
                                                             (n + 1) / (R + 1); observed and the p-values are NA where the rows carry no
                                                             labels (--regions without --mutations).  --write_simulated r ..: replicate
                                                             r as PREFIX.sim{r}.mutations.bed, a list that --mutations reads
  --summary PREFIX  --transcripts BED12 [--codon_table STR] [--alt_order SPEC]
                                                             PREFIX.consequence.mut_rates.tsv: per transcript of the BED12 file the
                                                             expected and observed mutations of the SNV rows inside its CDS, split into
                                                             synonymous, missense, stop gained and stop lost (blocks clipped to
                                                             thickStart .. thickEnd; offset 0 is the 5'-most CDS base).  STR: 64 amino
                                                             acids indexed by 16 b0 + 4 b1 + b2 with A0 C1 G2 T3, * a stop (default the
                                                             standard code); SPEC: the alternative base of mut_type 1, 2, 3 per own base
                                                             A, C, G, T (default CGT,AGT,ACT,ACG); observed is NA where the rows carry
                                                             no labels; not with --indel; alone or with the options above
  --summary PREFIX  --transcripts BED12 --simulate R --seed S --simulate_consequences
                                                             PREFIX.consequence.sim.tsv: per transcript and consequence the observed and
                                                             expected counts of the consequence table beside the mean, minimum and
                                                             maximum of the R simulated counts -- the rows inside the CDS whose draw is a
                                                             class whose substitution has that consequence --, n_ge / n_le and the
                                                             empirical p-values (n + 1) / (R + 1); --simulate then needs neither
                                                             --annotations nor --write_simulated
  --summary PREFIX  --transcripts BED12 --transcript_structure
                                                             PREFIX.consequence.structure.tsv as well: per transcript the expected and
                                                             observed mutations of the SNV rows inside chromStart .. chromEnd, split
                                                             into utr5, utr3, noncoding_exon, splice_donor, splice_acceptor (the two
                                                             essential bases at the ends of an intron between CDS bases), splice_utr
                                                             (those of any other intron), intron, start_lost (a change of the amino acid
                                                             of CDS codon 0: BED12 carries no frame, ATG is not demanded) and cds, and
                                                             expected_lof / observed_lof = stop gained + splice donor + splice acceptor
                                                             + start lost
  --summary PREFIX  --transcripts BED12 --transcript_structure --simulate R --seed S --simulate_consequences --simulate_structure
                                                             PREFIX.consequence.structure.sim.tsv as well: per transcript, structure bin
                                                             and lof the observed and expected counts of the structure file beside the
                                                             mean, minimum and maximum of the R simulated counts, n_ge / n_le and the
                                                             empirical p-values (n + 1) / (R + 1); the lof count of a replicate adds the
                                                             stop-gained, splice and start-lost events of the same draw; it needs every
                                                             flag named here; not with --indel
  --indel --summary PREFIX  --indel_transcripts BED12 --indel_kind insertion|deletion_start|deletion_end [--indel_lengths SPEC]
                                  [--breakpoint_offset 0|1]  PREFIX.indel_structure.tsv: per transcript the expected and observed INDEL
                                                             events of the model's kind by what they do to the transcript -- utr5,
                                                             utr3, noncoding_exon, splice (a splice dinucleotide of an intron between
                                                             CDS bases split or deleted), splice_utr (of any other intron), intron,
                                                             start_lost (CDS offsets 0 .. 2), frameshift, inframe and cds_mixed (a
                                                             class whose lengths hold both) --, expected_lof / observed_lof = splice +
                                                             start_lost + frameshift and the _upper pair = that + cds_mixed.  SPEC: the
                                                             lengths of mut_type 1, 2, .. (default 1,2,3,4,5,6,7-20 for 8 classes); the
                                                             event's boundary is start + offset (default 1); alone or with the
                                                             options above
  --indel --summary PREFIX  --indel_transcripts BED12 --indel_kind K --simulate R --seed S --simulate_indel_structure
                                                             PREFIX.indel_structure.sim.tsv as well: per transcript, INDEL structure
                                                             bin, lof and lof_upper the observed and expected counts of the INDEL
                                                             structure file beside the mean, minimum and maximum of the R simulated
                                                             counts, n_ge / n_le and the empirical p-values (n + 1) / (R + 1); the lof
                                                             counts of a replicate add the splice, start-lost and frameshift events (and
                                                             cds_mixed for lof_upper) of the same draw; --simulate then needs neither
                                                             --annotations nor --write_simulated; 2 .. 8 classes
  --strand pos|neg|both                                      with --indel and --kmer_length: the strand(s) the k-mers are counted on
  --benchmark_regions BED                                    count a site once per overlapping region in the scaling totals
  --genomewide_mu X --m_proportion M [--g_proportion G]     print the scaling factor
  --no-table                                                 summaries only: leave OUT.tsv out
  --scale_factor F                                           write the table scaled by F (the second pass of the two)"""
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from mural_amd.calibration import load_dirichlet_weights  # noqa: E402
from mural_amd.data import predict_bed, write_predictions  # noqa: E402
from mural_amd.model.nn_utils import load_model  # noqa: E402

_SUMMARY_OPTIONS = ("--summary", "--window_size", "--kmer_length", "--motif_length", "--annotations", "--strand", "--benchmark_regions", "--genomewide_mu", "--m_proportion", "--g_proportion",
                    "--scale_factor", "--n_bins", "--fit_calibrator", "--simulate", "--seed", "--write_simulated", "--transcripts", "--codon_table",
                    "--alt_order", "--indel_transcripts", "--indel_kind", "--indel_lengths", "--breakpoint_offset")
_PAIR_OPTIONS = ("--model_set", "--scale_factors")      # NAME CLASS=VALUE [CLASS=VALUE ..]
_VALUE_OPTIONS = ("--regions", "--focal", "--context", "--mutations") + _PAIR_OPTIONS + _SUMMARY_OPTIONS


def _split(argv):
    """(flags, positional arguments, {value option: [values]})"""
    flags, args, values = set(), [], {}
    argv = list(argv)
    it = iter(range(len(argv)))
    for at in it:
        a = argv[at]
        name, eq, val = a.partition("=")
        if name in _VALUE_OPTIONS:
            if not eq:
                at = next(it, None)
                if at is None:
                    raise SystemExit(f"{name} needs a value\n\n{__doc__}")
                val = argv[at]
            values.setdefault(name, []).append(val)
            while name in ("--motif_length", "--write_simulated") and at + 1 < len(argv) and argv[at + 1].lstrip("-").isdigit():      # M [M ..]
                at = next(it)
                values[name].append(argv[at])
            while name in _PAIR_OPTIONS and at + 1 < len(argv) and "=" in argv[at + 1] and not argv[at + 1].startswith("--"):
                at = next(it)
                values[name].append(argv[at])
        elif a.startswith("--"):
            flags.add(a)
        else:
            args.append(a)
    return flags, args, values


def main(argv):
    flags, args, values = _split(argv)
    model_type = "indel" if "--indel" in flags else "snv"
    poisson = "--poisson" in flags or model_type == "indel"
    opts = _summary_options(flags, values, model_type)
    if opts["calibration"] and "--regions" in values and "--mutations" not in values:
        raise SystemExit("--calibration_metrics needs labels: --regions alone gives every row the label 0; add --mutations FILE")
    opts["labelled"] = "--regions" not in values or "--mutations" in values      # --regions alone gives every row the label 0
    if opts["simulate"] is not None and ("--model_set" in values or "--scale_factors" in values):
        raise SystemExit("--simulate does not go with --model_set")
    if opts["fit_calibrator"] is not None and poisson:
        raise SystemExit("--fit_calibrator fits the raw softmax: it does not go with the Poisson calibration (--poisson; on by default "
                         "with --indel)")
    if "--model_set" in values or "--scale_factors" in values:
        return _main_model_set(args, values, flags, model_type, poisson, opts)
    if ("--mutations" in values or "--strict_mutations" in flags) and "--regions" not in values:
        raise SystemExit("--mutations / --strict_mutations label the sites that --regions enumerates: a BED run takes its labels from "
                         "the BED's score column")
    n_args = (3 if "--regions" in values else 4) - int(opts["no_table"])
    if opts["no_table"] and len(args) == n_args + 1:
        raise SystemExit(f"--no-table writes no table: leave {args[-1]} out")
    if len(args) != n_args:
        raise SystemExit(__doc__)
    if opts["no_table"]:
        args = args + [None]
    if "--regions" in values:
        if "--strict_mutations" in flags and "--mutations" not in values:
            raise SystemExit("--strict_mutations needs --mutations FILE")
        if len(values.get("--mutations", [])) > 1 or len(values.get("--focal", [])) > 1 or len(values.get("--context", [])) > 1:
            raise SystemExit(__doc__)
        return _main_regions(args, values, flags, model_type, poisson, opts)
    if set(values) - set(_SUMMARY_OPTIONS):
        raise SystemExit(__doc__)
    if opts["any"]:
        return _main_bed_sharded(args, flags, model_type, poisson, opts)
    model_path, fasta, bed, out = args
    model, cfg = load_model(model_path, model_type=model_type)
    res = predict_bed(model, fasta, bed, cfg["local_radius"], cfg.get("local_order", 3), distal_radius=cfg["distal_radius"],
                      segment_center=cfg.get("segment_center", 300000), model_type=model_type)
    cal = model_path + ".fdiri_cal.pkl"
    weights = load_dirichlet_weights(cal) if os.path.exists(cal) and "--no-calibration" not in flags else None
    write_predictions(res, out, poisson=poisson, dirichlet_weights=weights)
    print(f"{len(res['start'])} sites -> {out}")


def _summary_options(flags, values, model_type="snv"):
    """The summary / scaling options, checked before anything is loaded."""
    one = lambda name, kind: None if name not in values else kind(values[name][-1])      # noqa: E731
    opts = {"summary": one("--summary", str), "windows": tuple(int(w) for w in values.get("--window_size", [])),
            "benchmark_regions": one("--benchmark_regions", str), "genomewide_mu": one("--genomewide_mu", float),
            "m_proportion": one("--m_proportion", float), "g_proportion": one("--g_proportion", float),
            "scale_factor": one("--scale_factor", float), "no_table": "--no-table" in flags,
            "kmers": tuple(int(k) for k in values.get("--kmer_length", [])), "strand": one("--strand", str),
            "motifs": tuple(int(m) for m in values.get("--motif_length", [])), "calibration": "--calibration_metrics" in flags,
            "n_bins": one("--n_bins", int), "fit_calibrator": one("--fit_calibrator", str), "annotations": one("--annotations", str),
            "simulate": one("--simulate", int), "seed": one("--seed", lambda v: int(v, 0)),
            "write_simulated": tuple(int(r) for r in values.get("--write_simulated", [])), "transcripts": one("--transcripts", str),
            "codon_table": one("--codon_table", str), "alt_order": one("--alt_order", str),
            "simulate_consequences": "--simulate_consequences" in flags, "transcript_structure": "--transcript_structure" in flags,
            "simulate_structure": "--simulate_structure" in flags, "simulate_indel_structure": "--simulate_indel_structure" in flags,
            "indel_transcripts": one("--indel_transcripts", str),
            "indel_kind": one("--indel_kind", str), "indel_lengths": one("--indel_lengths", str),
            "breakpoint_offset": one("--breakpoint_offset", str)}
    if opts["indel_transcripts"] is not None and model_type != "indel":
        raise SystemExit("--indel_transcripts takes INDEL rows: it goes with --indel")
    if opts["indel_transcripts"] is not None and opts["indel_kind"] is None:
        raise SystemExit("--indel_transcripts needs --indel_kind insertion|deletion_start|deletion_end: the events the model predicts")
    if opts["indel_transcripts"] is None and (opts["indel_kind"] is not None or opts["indel_lengths"] is not None
                                              or opts["breakpoint_offset"] is not None):
        raise SystemExit("--indel_kind / --indel_lengths / --breakpoint_offset go with --indel_transcripts BED12")
    if opts["indel_transcripts"] is not None and opts["summary"] is None:
        raise SystemExit("--indel_transcripts needs --summary PREFIX: the prefix of the file it writes")
    if opts["simulate_indel_structure"] and model_type != "indel":
        raise SystemExit("--simulate_indel_structure takes INDEL rows: it goes with --indel")
    if opts["simulate_indel_structure"] and opts["indel_transcripts"] is None:
        raise SystemExit("--simulate_indel_structure needs --indel_transcripts BED12 --indel_kind K: the transcripts whose INDEL structure counts it simulates")
    if opts["simulate_indel_structure"] and (opts["simulate"] is None or opts["seed"] is None):
        raise SystemExit("--simulate_indel_structure needs --simulate R --seed S: the replicates it counts")
    if opts["simulate_structure"] and model_type == "indel":
        raise SystemExit("--simulate_structure takes SNV rows: it does not go with --indel")
    if opts["simulate_structure"] and opts["transcripts"] is None:
        raise SystemExit("--simulate_structure needs --transcripts BED12: the transcripts whose structure counts it simulates")
    if opts["simulate_structure"] and not opts["transcript_structure"]:
        raise SystemExit("--simulate_structure needs --transcript_structure: the structure table whose counts it simulates")
    if opts["simulate_structure"] and opts["simulate"] is None:
        raise SystemExit("--simulate_structure needs --simulate R --seed S: the replicates it counts")
    if opts["simulate_structure"] and not opts["simulate_consequences"]:
        raise SystemExit("--simulate_structure needs --simulate_consequences: the stop-gained counts of the same draws complete the lof count")
    if opts["transcript_structure"] and opts["transcripts"] is None:
        raise SystemExit("--transcript_structure needs --transcripts BED12: the transcripts whose UTRs, introns and splice sites it bins")
    if opts["transcript_structure"] and model_type == "indel":
        raise SystemExit("--transcript_structure takes SNV rows: it does not go with --indel")
    if opts["simulate_consequences"] and opts["transcripts"] is None:
        raise SystemExit("--simulate_consequences needs --transcripts BED12: the transcripts whose consequence counts it simulates")
    if opts["simulate_consequences"] and opts["simulate"] is None:
        raise SystemExit("--simulate_consequences needs --simulate R --seed S: the replicates it counts")
    if opts["simulate"] is not None and opts["seed"] is None:
        raise SystemExit("--simulate needs --seed S: there is no default randomness")
    if opts["simulate"] is None and (opts["seed"] is not None or opts["write_simulated"]):
        raise SystemExit("--seed / --write_simulated go with --simulate R")
    if opts["simulate"] is not None:
        if opts["summary"] is None:
            raise SystemExit("--simulate needs --summary PREFIX: the prefix of the files it writes")
        if opts["annotations"] is None and not opts["write_simulated"] and not opts["simulate_consequences"] and not opts["simulate_indel_structure"]:
            raise SystemExit("--simulate needs --annotations BED (the counts per name) or --write_simulated r")
        if not 1 <= opts["simulate"] <= 1 << 20 or not 0 <= opts["seed"] < 1 << 64:
            raise SystemExit("--simulate takes 1 .. 2^20 replicates and an unsigned 64-bit --seed")
        if any(not 0 <= r < opts["simulate"] for r in opts["write_simulated"]) or len(set(opts["write_simulated"])) != len(opts["write_simulated"]):
            raise SystemExit("--write_simulated takes distinct replicates below --simulate R")
    if opts["calibration"] and opts["summary"] is None:
        raise SystemExit("--calibration_metrics needs --summary PREFIX: the prefix of the file it writes")
    if (opts["n_bins"] is not None or opts["fit_calibrator"] is not None) and not opts["calibration"]:
        raise SystemExit("--n_bins / --fit_calibrator go with --calibration_metrics")
    if opts["n_bins"] is not None and opts["n_bins"] < 1:
        raise SystemExit("--n_bins must be positive")
    if opts["fit_calibrator"] is not None:
        from mural_amd.evaluation import CALIBRATORS
        if opts["fit_calibrator"] not in CALIBRATORS:
            raise SystemExit(f"--fit_calibrator {opts['fit_calibrator']}: one of {', '.join(sorted(CALIBRATORS))}")
        if opts["scale_factor"] is not None:
            raise SystemExit("--fit_calibrator fits the raw softmax (the reference fits its calibrator before any scaling): it does not go "
                             "with --scale_factor")
    if opts["windows"] and opts["summary"] is None:
        raise SystemExit("--window_size needs --summary PREFIX: the prefix of the files it writes")
    if opts["kmers"] and opts["summary"] is None:
        raise SystemExit("--kmer_length needs --summary PREFIX: the prefix of the files it writes")
    if opts["motifs"] and opts["summary"] is None:
        raise SystemExit("--motif_length needs --summary PREFIX: the prefix of the files it writes")
    if opts["annotations"] is not None and opts["summary"] is None:
        raise SystemExit("--annotations needs --summary PREFIX: the prefix of the files it writes")
    if opts["transcripts"] is not None and opts["summary"] is None:
        raise SystemExit("--transcripts needs --summary PREFIX: the prefix of the file it writes")
    if opts["transcripts"] is None and (opts["codon_table"] is not None or opts["alt_order"] is not None):
        raise SystemExit("--codon_table / --alt_order go with --transcripts BED12")
    if opts["transcripts"] is not None and model_type == "indel":
        raise SystemExit("--transcripts takes SNV rows: it does not go with --indel")
    if (opts["summary"] is not None and not opts["windows"] and not opts["kmers"] and not opts["motifs"] and not opts["calibration"]
            and opts["annotations"] is None and opts["simulate"] is None and opts["transcripts"] is None
            and opts["indel_transcripts"] is None):
        raise SystemExit("--summary PREFIX needs a --window_size, a --kmer_length, a --motif_length, --calibration_metrics, --annotations, "
                         "--simulate or --transcripts")
    if opts["transcripts"] is not None:
        from mural_amd.tables import check_alt_order, read_transcript_structure, read_transcripts
        try:
            opts["transcripts"] = (read_transcript_structure if opts["transcript_structure"] else read_transcripts)(opts["transcripts"],
                                                                                                                   opts["codon_table"])
            opts["alt_order"] = check_alt_order(opts["alt_order"])
        except (OSError, ValueError) as e:
            raise SystemExit(f"--transcripts: {e}") from None
    if opts["indel_transcripts"] is not None:
        from mural_amd.tables import check_breakpoint_offset, check_indel_kind, check_indel_lengths, read_transcript_structure
        try:
            opts["indel_kind"] = check_indel_kind(opts["indel_kind"])
            if opts["indel_lengths"] is not None:
                opts["indel_lengths"] = check_indel_lengths(opts["indel_lengths"])
            offset = opts["breakpoint_offset"]
            opts["breakpoint_offset"] = 1 if offset is None else check_breakpoint_offset(int(offset) if offset.isdigit() else offset)
            opts["indel_transcripts"] = read_transcript_structure(opts["indel_transcripts"])
        except (OSError, ValueError) as e:
            raise SystemExit(f"--indel_transcripts: {e}") from None
    if opts["annotations"] is not None:
        from mural_amd.tables import read_annotations
        try:
            opts["annotations"] = read_annotations(opts["annotations"])
        except (OSError, ValueError) as e:
            raise SystemExit(f"--annotations: {e}") from None
    if opts["motifs"]:
        from mural_amd.tables import check_motif_length
        try:
            for m in opts["motifs"]:
                check_motif_length(m)
        except ValueError as e:
            raise SystemExit(f"--motif_length: {e}") from None
    if opts["kmers"]:
        from mural_amd.tables import check_kmer_length, strand_mode
        try:
            for k in opts["kmers"]:
                check_kmer_length(k)
            if model_type == "indel" or opts["strand"] is not None:
                if model_type != "indel":
                    raise ValueError("--strand goes with --indel")
                strand_mode("indel", opts["strand"])
        except ValueError as e:
            raise SystemExit(f"--kmer_length: {e}") from None
    elif opts["strand"] is not None:
        raise SystemExit("--strand selects the strand of the k-mer tables: it goes with --indel and --kmer_length")
    if (opts["genomewide_mu"] is None) != (opts["m_proportion"] is None):
        raise SystemExit("the scaling factor needs --genomewide_mu and --m_proportion")
    if opts["g_proportion"] is not None and opts["genomewide_mu"] is None:
        raise SystemExit("--g_proportion goes with --genomewide_mu and --m_proportion")
    opts["wants_summary"] = opts["summary"] is not None or opts["genomewide_mu"] is not None
    if opts["benchmark_regions"] is not None and opts["genomewide_mu"] is None:
        raise SystemExit("--benchmark_regions weighs the scaling totals: it goes with --genomewide_mu and --m_proportion")
    if opts["no_table"] and not opts["wants_summary"]:
        raise SystemExit("--no-table leaves nothing to do without --summary or --genomewide_mu")
    opts["any"] = opts["wants_summary"] or opts["no_table"] or opts["scale_factor"] is not None
    return opts


def _forward_and_sink(model_path, fasta, out, flags, model_type, poisson, opts):
    """The forward and the sink(s) of a sharded run.  Without --scale_factor the calibration chain runs in the sinks, as write_predictions
    applies it in the plain BED form; with it the whole chain, the scaling last, runs behind the head and the sinks take what they get."""
    from mural_amd.predict import HipShardForward, SummarySink, TeeSink, TsvSink
    model, cfg = load_model(model_path, model_type=model_type)
    cal = model_path + ".fdiri_cal.pkl"
    weights = load_dirichlet_weights(cal) if os.path.exists(cal) and "--no-calibration" not in flags else None
    if opts["fit_calibrator"] is not None and weights is not None:
        raise SystemExit(f"--fit_calibrator fits the raw softmax, but {cal} would calibrate this run: pass --no-calibration")
    in_forward = opts["scale_factor"] is not None
    chain = dict(poisson=poisson, dirichlet_weights=weights)
    forward = HipShardForward(model, fasta, cfg["local_radius"], cfg.get("local_order", 3), distal_radius=cfg["distal_radius"],
                              model_type=model_type, scale_factor=opts["scale_factor"], **(chain if in_forward else dict(poisson=False)))
    sink_chain = {} if in_forward else chain
    sinks, summary = [], None
    if out is not None:
        sinks.append(TsvSink(out, **sink_chain))
    if opts["wants_summary"]:
        summary = SummarySink(opts["summary"], opts["windows"], opts["benchmark_regions"], kmers=opts["kmers"], genome=forward.genome,
                              kmer_strand=opts["strand"] if model_type == "indel" else None, motifs=opts["motifs"],
                              motif_indel=model_type == "indel", calibration=opts["calibration"],
                              calibration_bins=50 if opts["n_bins"] is None else opts["n_bins"], fit_calibrator=opts["fit_calibrator"],
                              annotations=opts["annotations"], simulate=opts["simulate"], simulate_seed=opts["seed"],
                              simulate_write=opts["write_simulated"], simulate_labels=opts.get("labelled", True), transcripts=opts["transcripts"], alt_order=opts["alt_order"],
                              transcript_labels=opts.get("labelled", True), simulate_transcripts=opts["simulate_consequences"],
                              transcript_structure=opts["transcript_structure"], simulate_structure=opts["simulate_structure"],
                              **(dict(indel_transcripts=opts["indel_transcripts"], indel_kind=opts["indel_kind"],
                                      indel_lengths=opts["indel_lengths"], breakpoint_offset=opts["breakpoint_offset"],
                                      simulate_indel_structure=opts["simulate_indel_structure"])
                                 if opts["indel_transcripts"] is not None else {}), **sink_chain)
        sinks.append(summary)
    return forward, cfg, sinks[0] if len(sinks) == 1 else TeeSink(*sinks), summary


def _report(n, out, summary, opts):
    print(f"{n} sites -> {out}" if out is not None else f"{n} sites")
    if summary is not None and opts["calibration"]:
        res = summary.result()["calibration"]
        for tag, m in (("", res),) + (((" (after %s)" % opts["fit_calibrator"], res["after"]),) if "after" in res else ()):
            print("calibration%s - rows: %d, NLL: %.8f, ECE: %.8f, CwECE: %.8f, Brier: %.8f" % (tag, m["rows"], m["nll"], m["ece"], m["c_ece"],
                                                                                              m["brier"]))
    if summary is not None and opts["genomewide_mu"] is not None:
        summary.scaling_factor(opts["genomewide_mu"], opts["m_proportion"], 1.0 if opts["g_proportion"] is None else opts["g_proportion"])


def _report_mutations(split):
    if "mutations" in split:
        print("mutations inside the regions: {in_regions}, on an enumerated site: {matched}, on none: {unmatched}".format(**split["mutations"]))


def _main_bed_sharded(args, flags, model_type, poisson, opts):
    from mural_amd.predict import predict_bed_sharded
    model_path, fasta, bed, out = args
    forward, cfg, sink, summary = _forward_and_sink(model_path, fasta, out, flags, model_type, poisson, opts)
    n = predict_bed_sharded(forward, bed, segment_center=cfg.get("segment_center", 300000), model_type=model_type, sink=sink, collect=False)
    _report(n, out, summary, opts)


def _main_regions(args, values, flags, model_type, poisson, opts):
    from mural_amd.predict import HipShardForward, TsvSink, predict_regions_sharded, read_regions_arg
    model_path, fasta, out = args
    if model_type == "indel":
        if "--focal" in values or "--context" in values:
            raise SystemExit("--focal / --context select SNV sites; an INDEL model takes every A/C/G/T position")
        focal, context = "ANY", "all"
    else:
        focal, context = values.get("--focal", ["A"])[0], values.get("--context", ["all"])[0]
    regions = read_regions_arg(values["--regions"])
    split = {}
    labels = dict(mutations=values["--mutations"][0], strict_mutations="--strict_mutations" in flags) if "--mutations" in values else {}
    if opts["any"]:
        forward, cfg, sink, summary = _forward_and_sink(model_path, fasta, out, flags, model_type, poisson, opts)
        n = predict_regions_sharded(forward, regions, focal, context, model_type=model_type, sink=sink, collect=False, timings=split,
                                    **labels)
        _report_mutations(split)
        return _report(n, out, summary, opts)
    model, cfg = load_model(model_path, model_type=model_type)
    cal = model_path + ".fdiri_cal.pkl"
    weights = load_dirichlet_weights(cal) if os.path.exists(cal) and "--no-calibration" not in flags else None
    # the calibration chain runs in the sink, as write_predictions applies it in the BED form
    forward = HipShardForward(model, fasta, cfg["local_radius"], cfg.get("local_order", 3), distal_radius=cfg["distal_radius"],
                              model_type=model_type, poisson=False)
    sink = TsvSink(out, poisson=poisson, dirichlet_weights=weights)
    n = predict_regions_sharded(forward, regions, focal, context, model_type=model_type, sink=sink, collect=False, timings=split, **labels)
    _report_mutations(split)
    print(f"{n} sites -> {out}")


_SET_CLASSES = ("A", "C", "nonCpG", "CpG")


def _class_pairs(option, items, kind):
    """{CLASS: kind(VALUE)} of the CLASS=VALUE arguments of `option`."""
    out = {}
    for item in items:
        name, eq, val = item.partition("=")
        if not eq or not val or name not in _SET_CLASSES:
            raise SystemExit(f"{option} {item!r}: expected CLASS=VALUE with CLASS one of {', '.join(_SET_CLASSES)}")
        if name in out:
            raise SystemExit(f"{option}: class {name} is named twice")
        try:
            out[name] = kind(val)
        except ValueError:
            raise SystemExit(f"{option} {item!r}: bad value") from None
    return out


def _main_model_set(args, values, flags, model_type, poisson, opts):
    """--regions with one model per site class: one table, every row by the model of its own base."""
    if "--model_set" not in values:
        raise SystemExit("--scale_factors CLASS=F sets the factors of the models that --model_set names")
    if "--model_path" in flags or len(args) == 3:
        raise SystemExit("--model_set names the models (CLASS=MODEL_PATH): leave the MODEL argument / --model_path out "
                         "(FASTA OUT.tsv --regions SPEC --model_set CLASS=MODEL_PATH ..)")
    if opts["wants_summary"] or opts["no_table"]:
        raise SystemExit("--model_set does not go with --summary / --genomewide_mu / --no-table: a scaling factor belongs to one model, "
                         "and per-class summaries are not written; summarise each model's own run")
    if opts["scale_factor"] is not None:
        raise SystemExit("--model_set takes a factor per class: --scale_factors CLASS=F ..")
    if "--regions" not in values:
        raise SystemExit("--model_set needs --regions: a BED run serves one model (its per-segment focal-base check stands)")
    if model_type == "indel" or "--focal" in values or "--context" in values:
        raise SystemExit("--model_set selects the sites by its classes: it takes neither --indel nor --focal / --context")
    if len(args) != 2:
        raise SystemExit(__doc__)
    if "--strict_mutations" in flags and "--mutations" not in values:
        raise SystemExit("--strict_mutations needs --mutations FILE")
    if len(values.get("--mutations", [])) > 1:
        raise SystemExit(__doc__)
    paths = _class_pairs("--model_set", values["--model_set"], str)
    factors = _class_pairs("--scale_factors", values.get("--scale_factors", []), float)
    if "C" in paths and ("CpG" in paths or "nonCpG" in paths):
        raise SystemExit("--model_set: C serves the CpG and the nonCpG sites: it does not go with a CpG or nonCpG model")
    for name in factors:
        if name not in paths:
            raise SystemExit(f"--scale_factors: class {name} has no model in --model_set")
    from mural_amd.predict import HipShardForward, ModelSetForward, TsvSink, predict_regions_sharded, read_regions_arg
    fasta, out = args
    regions = read_regions_arg(values["--regions"])
    chains = {}
    for name, path in paths.items():
        cal = path + ".fdiri_cal.pkl"
        weights = load_dirichlet_weights(cal) if os.path.exists(cal) and "--no-calibration" not in flags else None
        chains[name] = dict(dirichlet_weights=weights, poisson=poisson, scale_factor=factors.get(name))
    # every member runs its own chain behind its head (the sink could apply one calibrator only), so all of them have one or none has
    has = {name: c["dirichlet_weights"] is not None or bool(c["poisson"]) or bool(c["scale_factor"]) for name, c in chains.items()}
    if len(set(has.values())) > 1:
        raise SystemExit("--model_set: %s would be calibrated or scaled and %s would not, but one table has one number format: give every "
                         "model a calibrator or a --scale_factors entry, or pass --no-calibration"
                         % (", ".join(k for k in has if has[k]), ", ".join(k for k in has if not has[k])))
    members = {}
    for name, path in paths.items():
        model, cfg = load_model(path, model_type="snv")
        members[name] = HipShardForward(model, None, cfg["local_radius"], cfg.get("local_order", 3), distal_radius=cfg["distal_radius"],
                                        model_type="snv", **chains[name])
    try:
        forward = ModelSetForward(members, fasta_path=fasta)
    except ValueError as e:
        raise SystemExit(f"--model_set: {e}") from None
    split = {}
    labels = dict(mutations=values["--mutations"][0], strict_mutations="--strict_mutations" in flags) if "--mutations" in values else {}
    n = predict_regions_sharded(forward, regions, "SET", sink=TsvSink(out), collect=False, timings=split, **labels)
    _report_mutations(split)
    print(f"{n} sites -> {out}")


if __name__ == "__main__":
    main(sys.argv[1:])
