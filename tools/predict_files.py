"""File-to-file prediction with a reference-style model directory (what `mural_snv predict` / scripts/run_predict.py:58-239 does,
minus its CLI): python tools/predict_files.py MODEL FASTA BED OUT.tsv [--indel] [--poisson] [--no-calibration]

Without a BED file -- the sites are enumerated from the FASTA on the device (mural_amd.predict.predict_regions_sharded):
  python tools/predict_files.py MODEL FASTA OUT.tsv --regions SPEC [--regions SPEC ..] [--focal A|C] [--context all|CpG|nonCpG]
SPEC: chr, chr:start-end (1-based, inclusive) or a BED-like file of regions; --focal defaults to A (with --indel every A/C/G/T
position is a site and --focal / --context do not apply)."""
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from mural_amd.calibration import load_dirichlet_weights  # noqa: E402
from mural_amd.data import predict_bed, write_predictions  # noqa: E402
from mural_amd.model.nn_utils import load_model  # noqa: E402

_VALUE_OPTIONS = ("--regions", "--focal", "--context")


def _split(argv):
    """(flags, positional arguments, {value option: [values]})"""
    flags, args, values = set(), [], {}
    it = iter(argv)
    for a in it:
        name, eq, val = a.partition("=")
        if name in _VALUE_OPTIONS:
            if not eq:
                val = next(it, None)
                if val is None:
                    raise SystemExit(f"{name} needs a value\n\n{__doc__}")
            values.setdefault(name, []).append(val)
        elif a.startswith("--"):
            flags.add(a)
        else:
            args.append(a)
    return flags, args, values


def main(argv):
    flags, args, values = _split(argv)
    model_type = "indel" if "--indel" in flags else "snv"
    poisson = "--poisson" in flags or model_type == "indel"
    if "--regions" in values:
        if len(args) != 3 or len(values.get("--focal", [])) > 1 or len(values.get("--context", [])) > 1:
            raise SystemExit(__doc__)
        return _main_regions(args, values, flags, model_type, poisson)
    if len(args) != 4 or values:
        raise SystemExit(__doc__)
    model_path, fasta, bed, out = args
    model, cfg = load_model(model_path, model_type=model_type)
    res = predict_bed(model, fasta, bed, cfg["local_radius"], cfg.get("local_order", 3), distal_radius=cfg["distal_radius"],
                      segment_center=cfg.get("segment_center", 300000), model_type=model_type)
    cal = model_path + ".fdiri_cal.pkl"
    weights = load_dirichlet_weights(cal) if os.path.exists(cal) and "--no-calibration" not in flags else None
    write_predictions(res, out, poisson=poisson, dirichlet_weights=weights)
    print(f"{len(res['start'])} sites -> {out}")


def _main_regions(args, values, flags, model_type, poisson):
    from mural_amd.predict import HipShardForward, TsvSink, predict_regions_sharded, read_regions_arg
    model_path, fasta, out = args
    if model_type == "indel":
        if "--focal" in values or "--context" in values:
            raise SystemExit("--focal / --context select SNV sites; an INDEL model takes every A/C/G/T position")
        focal, context = "ANY", "all"
    else:
        focal, context = values.get("--focal", ["A"])[0], values.get("--context", ["all"])[0]
    regions = read_regions_arg(values["--regions"])
    model, cfg = load_model(model_path, model_type=model_type)
    cal = model_path + ".fdiri_cal.pkl"
    weights = load_dirichlet_weights(cal) if os.path.exists(cal) and "--no-calibration" not in flags else None
    # the calibration chain runs in the sink, as write_predictions applies it in the BED form
    forward = HipShardForward(model, fasta, cfg["local_radius"], cfg.get("local_order", 3), distal_radius=cfg["distal_radius"],
                              model_type=model_type, poisson=False)
    sink = TsvSink(out, poisson=poisson, dirichlet_weights=weights)
    n = predict_regions_sharded(forward, regions, focal, context, model_type=model_type, sink=sink, collect=False)
    print(f"{n} sites -> {out}")


if __name__ == "__main__":
    main(sys.argv[1:])
