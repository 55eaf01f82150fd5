"""Saturation-mutagenesis table of BED sites (mural_amd.mutagenesis.saturation_mutagenesis; DESIGN.md sections 3.27, 3.28):

  python tools/mutagenesis_files.py --ref_genome FASTA --sites BED --model_path MODEL [--model_config_path CONFIG] --out PREFIX
                                    [--model_type snv|indel] [--top K] [--batch_sites N] [--profile [--per_site]]
                                    [--group_by none|name|strand]

Writes PREFIX.mutagenesis.tsv, one row per (site, window column, alternative base):
  chrom  site_start  strand  offset  genomic_pos  ref  alt  delta_logp1 .. delta_logp{n_class}
offset is the column's distance from the site in window orientation (negative = 5' of the site on the site's strand), genomic_pos the
0-based '+'-strand position of that column, ref / alt the base there and its replacement ON THE GENOMIC '+' STRAND, delta_logp the change
of the model's log-probabilities (%.4g).  Columns that are not A/C/G/T in the genome (N, IUPAC codes, beyond the chromosome ends) have no
rows.  --top K keeps, per site, the K columns of largest importance (max |delta| over alternatives and classes).  --model_path /
--model_config_path / --ref_genome are the reference's flag names (MuRaL/commands/predict.py); the config defaults to MODEL.config.pkl.
--model_type indel: a UNet_Small checkpoint; the window is [site - R + 1, site + R] (R = the config's distal_radius), so on '+' the
offsets run from -(R - 1) to R and on '-' from -R to R - 1; the same table otherwise.

--profile writes PREFIX.mutagenesis.profile.tsv INSTEAD: the maps of all sites reduced on the device
(mural_amd.mutagenesis.mutagenesis_profile), one row per populated cell:
  group  offset  ref  alt  class  n  mean  mean_abs  rms
ref / alt are bases IN WINDOW ORIENTATION (the site's strand), offset the column's distance from the site (for --model_type indel the
distance on '+'; a '-' site's is one less), class 1-based, n the number of (site, substitution) terms, the statistics those of
delta_logp (%.6g).  No map is held: the sites stream through in batches of --batch_sites, which then bounds the site arrays only
(default 65536 with --profile alone).  --group_by name groups by column 4 of the BED, labels numbered in order of first appearance;
--group_by strand by the site's strand; the labels are the first column.  --per_site writes the per-site table as well."""
import argparse
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from mural_amd.data.ingest import read_bed, read_fasta  # noqa: E402
from mural_amd.model.nn_utils import load_model  # noqa: E402
from mural_amd.mutagenesis import mutagenesis_profile, saturation_mutagenesis  # noqa: E402


def output_name(prefix):
    return prefix + ".mutagenesis.tsv"


def profile_name(prefix):
    return prefix + ".mutagenesis.profile.tsv"


def bed_names(path, rows):
    """Column 4 of the BED's data rows, in file order (the device reader keeps no text)."""
    names = []
    with open(path) as fh:
        for line in fh:
            if not line.strip() or line.startswith(("#", "track", "browser")):
                continue
            cols = line.rstrip("\n").split("\t")
            if len(cols) < 4:
                raise SystemExit(f"{path}: --group_by name needs the name column (column 4) in every row")
            names.append(cols[3])
    if len(names) != rows:
        raise SystemExit(f"{path}: {len(names)} rows with a name, {rows} sites read")
    return names


def site_groups(bed, group_by, path=None):
    """(labels, int32 group id per BED row): ids in order of first appearance."""
    if group_by == "none":
        return ["all"], np.zeros(len(bed.start), np.int32)
    if group_by == "strand":
        return ["+", "-"], (np.asarray(bed.strand) != 0).astype(np.int32)
    labels, ids = {}, np.empty(len(bed.start), np.int32)
    for i, name in enumerate(bed_names(path, len(bed.start))):
        ids[i] = labels.setdefault(name, len(labels))
    return list(labels), ids


def write_profile(path, prof, labels):
    """One row per populated cell of a ``MutagenesisProfile``; returns the number of rows."""
    n, mean, mean_abs, rms, off = prof.counts(), prof.mean(), prof.mean_abs(), prof.rms(), prof.offsets()
    rows = 0
    with open(path, "w") as fh:
        fh.write("group\toffset\tref\talt\tclass\tn\tmean\tmean_abs\trms\n")
        for g, j, ref, alt, c in np.argwhere(~np.isnan(n)).tolist():
            at = (g, j, ref, alt, c)
            fh.write(f"{labels[g]}\t{off[j]}\t{'ACGT'[ref]}\t{'ACGT'[alt]}\t{c + 1}\t{int(n[at])}\t{mean[at]:.6g}\t{mean_abs[at]:.6g}\t{rms[at]:.6g}\n")
            rows += 1
    return rows


def write_rows(fh, chrom, res, top=None):
    """The rows of one ``MutagenesisMap`` (host side: a few thousand short lines per site)."""
    delta = res.delta.cpu().numpy()
    sym = res.ref_symbols.cpu().numpy()
    gpos = res.genomic_positions().cpu().numpy()
    imp = res.importance().cpu().numpy()
    pos, strand = res.pos.cpu().numpy(), res.strand.cpu().numpy()
    R = res.radius
    rows = 0
    for s in range(len(pos)):
        neg = bool(strand[s])
        site_col = R if res.model_type == "snv" or neg else R - 1      # the window column that holds the site itself
        cols = np.nonzero(sym[s] < 4)[0]
        if top is not None:
            keep = cols[np.argsort(-imp[s, cols], kind="stable")[:top]]
            cols = np.sort(keep)
        for j in cols.tolist():
            ref_w = int(sym[s, j])
            ref = "ACGT"[3 - ref_w if neg else ref_w]
            for b in range(4):
                if b == ref_w:
                    continue
                alt = "ACGT"[3 - b if neg else b]
                vals = "\t".join("%.4g" % v for v in delta[s, j, b])
                fh.write(f"{chrom}\t{pos[s]}\t{'-' if neg else '+'}\t{j - site_col}\t{gpos[s, j]}\t{ref}\t{alt}\t{vals}\n")
                rows += 1
    return rows


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--ref_genome", required=True)
    ap.add_argument("--sites", required=True, help="six-column BED (chrom start end name score strand)")
    ap.add_argument("--model_path", required=True)
    ap.add_argument("--model_config_path", default=None)
    ap.add_argument("--out", required=True, help="prefix of PREFIX.mutagenesis.tsv")
    ap.add_argument("--model_type", default="snv", choices=["snv", "indel"])
    ap.add_argument("--top", type=int, default=None)
    ap.add_argument("--batch_sites", type=int, default=None,
                    help="sites per call: per map held on the device (default 64), or, with --profile alone, per batch of site arrays (default 65536)")
    ap.add_argument("--profile", action="store_true", help="write PREFIX.mutagenesis.profile.tsv instead of the per-site table")
    ap.add_argument("--per_site", action="store_true", help="with --profile: write the per-site table as well")
    ap.add_argument("--group_by", default="none", choices=["none", "name", "strand"])
    args = ap.parse_args(argv)
    if args.top is not None and args.top < 1:
        raise SystemExit("--top must be positive")
    if not args.profile and (args.per_site or args.group_by != "none"):
        raise SystemExit("--per_site and --group_by go with --profile")
    maps = not args.profile or args.per_site
    batch = args.batch_sites if args.batch_sites is not None else (64 if maps else 65536)
    if batch < 1:
        raise SystemExit("--batch_sites must be positive")
    model, cfg = load_model(args.model_path, args.model_config_path, model_type=args.model_type)
    bed = read_bed(args.sites)
    labels, group_ids = site_groups(bed, args.group_by, args.sites) if args.profile else (None, None)
    if args.model_type == "indel":
        model_kw = dict(distal_radius=cfg["distal_radius"])
    else:
        model_kw = dict(local_radius=cfg["local_radius"], local_order=cfg.get("local_order", 3))
    out, rows, prof = output_name(args.out), 0, None
    with open(out if maps else os.devnull, "w") as fh:
        header = ["chrom", "site_start", "strand", "offset", "genomic_pos", "ref", "alt"]
        fh.write("\t".join(header + [f"delta_logp{c + 1}" for c in range(cfg["n_class"])]) + "\n")
        for cid, chrom in enumerate(bed.chrom_names):
            sel = np.nonzero(bed.chrom_id == cid)[0]
            genome = read_fasta(args.ref_genome, "cuda", names=[chrom]).get(chrom)
            if genome is None:
                raise SystemExit(f"{args.sites}: chromosome {chrom} is not in {args.ref_genome}")
            for b0 in range(0, len(sel), batch):
                part = sel[b0:b0 + batch]
                pos = torch.from_numpy(bed.start[part]).cuda()
                strand = torch.from_numpy(bed.strand[part]).cuda()
                if args.profile:
                    prof = mutagenesis_profile(model, genome, pos, strand, groups=torch.from_numpy(group_ids[part]).cuda(),
                                               n_groups=len(labels), into=prof, **model_kw)
                if maps:
                    rows += write_rows(fh, chrom, saturation_mutagenesis(model, genome, pos, strand, **model_kw), args.top)
    if maps:
        print(f"{len(bed.start)} sites, {rows} rows -> {out}")
    if args.profile:
        if prof is None:
            raise SystemExit(f"{args.sites}: no sites")
        cells = write_profile(profile_name(args.out), prof, labels)
        bits, nonfinite, out_of_range = prof.status_host()
        if bits:
            print(f"left out of the profile: {nonfinite} non-finite terms, {out_of_range} terms of |delta_logp| >= 256")
        print(f"{len(bed.start)} sites, {cells} cells -> {profile_name(args.out)}")


if __name__ == "__main__":
    main()
