"""Footprints of the insertions, deletions and multi-base alleles of a variant list (mural_amd.mutagenesis.allele_footprint; DESIGN.md
section 3.29):

  python tools/allele_files.py --ref_genome FASTA --variants VCF_BODY --model_path MODEL [--model_config_path CONFIG] --out PREFIX
                               [--model_type snv|indel] [--strand pos|neg|both]

--variants holds VCF body lines (CHROM POS ID REF ALT ..., tab-separated; lines that start with '#' are skipped); a comma-separated ALT
gives one allele each.  REF / ALT are trimmed to the bases that differ (the anchor base of an insertion or deletion, then a shared
suffix).  Skipped, and counted in the closing line: symbolic alleles and '*'; alleles with bases other than A/C/G/T; alleles whose
trimmed ALT is longer than 32 bases; records whose REF is not what the FASTA holds there.

Writes PREFIX.allele_footprint.tsv, one row per (allele, strand, reachable site inside the chromosome):
  chrom  variant_pos  ref  alt  site_pos  strand  focal  delta_logp1 .. delta_logp{n_class}
variant_pos / ref / alt are the record's own (POS is 1-based), site_pos the 0-based reference position of the site, focal the reference
base there on `strand`, delta_logp the change of the site's log-probabilities on the alternate haplotype (%.4g).  Sites inside the
replaced span and on inserted bases are not part of a footprint.  --model_path / --model_config_path / --ref_genome are the reference's
flag names (MuRaL/commands/predict.py); the config defaults to MODEL.config.pkl."""
import argparse
import gzip
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from mural_amd.data.ingest import read_fasta  # noqa: E402
from mural_amd.model.nn_utils import load_model  # noqa: E402
from mural_amd.mutagenesis import MAX_ALT, Alleles, allele_footprint  # noqa: E402

SYMBOLS = "ACGTNRYMSWKBDHV"          # MURAL_SYM_* codes as letters
SKIPS = ("symbolic", "non_acgt", "too_long", "ref_mismatch")
BATCH = 256                          # alleles per footprint call


def output_name(prefix):
    return prefix + ".allele_footprint.tsv"


def fasta_text(path, names):
    """{name: upper-case sequence} of the records `names`: the host copy the REF column is checked against"""
    out, name = {}, None
    with (gzip.open(path, "rt") if path.endswith(".gz") else open(path)) as fh:
        for line in fh:
            if line.startswith(">"):
                name = line[1:].split()[0] if line[1:].split() else ""
                name = name if name in names else None
                if name is not None:
                    out[name] = []
            elif name is not None:
                out[name].append(line.strip().upper())
    return {k: "".join(v) for k, v in out.items()}


def read_variants(path):
    """[(chrom, pos1, ref, alt)] with one entry per ALT, in file order"""
    records = []
    with open(path) as fh:
        for line in fh:
            if line.startswith("#") or not line.strip():
                continue
            f = line.rstrip("\n").split("\t")
            if len(f) < 5:
                raise SystemExit(f"{path}: a variant line needs CHROM POS ID REF ALT, got {line!r}")
            records += [(f[0], int(f[1]), f[3], alt) for alt in f[4].split(",")]
    return records


def classify(record, text):
    """(skip reason or None, (p, d, alt)) of one (chrom, pos1, ref, alt) against its chromosome's text"""
    _, pos1, ref, alt = record
    if alt == "*" or alt == "." or any(ch in alt for ch in "<>[]"):
        return "symbolic", None
    if set(ref.upper()) - set("ACGT") or set(alt.upper()) - set("ACGT"):
        return "non_acgt", None
    if pos1 < 1 or text[pos1 - 1:pos1 - 1 + len(ref)] != ref.upper():
        return "ref_mismatch", None
    p, d, trimmed = Alleles.from_vcf_fields(pos1, ref, alt)
    if len(trimmed) > MAX_ALT:
        return "too_long", None
    return None, (p, d, trimmed)


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--ref_genome", required=True)
    ap.add_argument("--variants", required=True, help="VCF body lines: CHROM POS ID REF ALT ...")
    ap.add_argument("--model_path", required=True)
    ap.add_argument("--model_config_path", default=None)
    ap.add_argument("--out", required=True, help="prefix of PREFIX.allele_footprint.tsv")
    ap.add_argument("--model_type", default="snv", choices=["snv", "indel"])
    ap.add_argument("--strand", default="both", choices=["pos", "neg", "both"])
    args = ap.parse_args(argv)
    model, cfg = load_model(args.model_path, args.model_config_path, model_type=args.model_type)
    records = read_variants(args.variants)
    chroms = list(dict.fromkeys(r[0] for r in records))
    texts = fasta_text(args.ref_genome, set(chroms))
    strands = {"pos": [0], "neg": [1], "both": [0, 1]}[args.strand]
    skipped = dict.fromkeys(SKIPS, 0)
    out, rows, kept = output_name(args.out), 0, 0
    with open(out, "w") as fh:
        header = ["chrom", "variant_pos", "ref", "alt", "site_pos", "strand", "focal"]
        fh.write("\t".join(header + [f"delta_logp{c + 1}" for c in range(cfg["n_class"])]) + "\n")
        for chrom in chroms:
            if chrom not in texts:
                raise SystemExit(f"{args.variants}: chromosome {chrom} is not in {args.ref_genome}")
            live = []
            for rec in (r for r in records if r[0] == chrom):
                why, allele = classify(rec, texts[chrom])
                if why:
                    skipped[why] += 1
                else:
                    live += [(rec, allele, s) for s in strands]
            kept += len(live) // len(strands)
            genome = read_fasta(args.ref_genome, "cuda", names=[chrom])[chrom]
            for b0 in range(0, len(live), BATCH):
                part = live[b0:b0 + BATCH]
                table = Alleles.from_host([a[0] for _, a, _ in part], [a[1] for _, a, _ in part], [a[2] for _, a, _ in part], "cuda")
                strand = torch.tensor([s for _, _, s in part], dtype=torch.uint8, device="cuda")
                if args.model_type == "indel":
                    delta, focal = allele_footprint(model, genome, table, strand, distal_radius=cfg["distal_radius"])
                    R, slots = cfg["distal_radius"], 2 * cfg["distal_radius"] - 1
                else:
                    delta, focal = allele_footprint(model, genome, table, strand, cfg["local_radius"], cfg.get("local_order", 3))
                    R, slots = cfg["distal_radius"], 2 * cfg["distal_radius"]
                delta, focal = delta.cpu().numpy(), focal.cpu().numpy()
                e = np.arange(slots) - R
                for i, ((_, pos1, ref, alt), (p, d, _), s) in enumerate(part):
                    site = np.where(e < 0, p + e, p + d + e)
                    for c in np.nonzero(~np.isnan(delta[i]).any(axis=1))[0].tolist():
                        vals = "\t".join("%.4g" % v for v in delta[i, c])
                        fh.write(f"{chrom}\t{pos1}\t{ref}\t{alt}\t{site[c]}\t{'-' if s else '+'}\t{SYMBOLS[focal[i, c]]}\t{vals}\n")
                        rows += 1
    print(f"{kept} alleles, {rows} rows -> {out}; skipped: " + ", ".join(f"{k} {skipped[k]}" for k in SKIPS))
    return dict(alleles=kept, rows=rows, skipped=skipped)


if __name__ == "__main__":
    main()
