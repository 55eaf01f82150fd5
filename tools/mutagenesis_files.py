"""Saturation-mutagenesis table of BED sites (mural_amd.mutagenesis.saturation_mutagenesis; DESIGN.md sections 3.27, 3.28):

  python tools/mutagenesis_files.py --ref_genome FASTA --sites BED --model_path MODEL [--model_config_path CONFIG] --out PREFIX
                                    [--model_type snv|indel] [--top K] [--batch_sites N]

Writes PREFIX.mutagenesis.tsv, one row per (site, window column, alternative base):
  chrom  site_start  strand  offset  genomic_pos  ref  alt  delta_logp1 .. delta_logp{n_class}
offset is the column's distance from the site in window orientation (negative = 5' of the site on the site's strand), genomic_pos the
0-based '+'-strand position of that column, ref / alt the base there and its replacement ON THE GENOMIC '+' STRAND, delta_logp the change
of the model's log-probabilities (%.4g).  Columns that are not A/C/G/T in the genome (N, IUPAC codes, beyond the chromosome ends) have no
rows.  --top K keeps, per site, the K columns of largest importance (max |delta| over alternatives and classes).  --model_path /
--model_config_path / --ref_genome are the reference's flag names (MuRaL/commands/predict.py); the config defaults to MODEL.config.pkl.
--model_type indel: a UNet_Small checkpoint; the window is [site - R + 1, site + R] (R = the config's distal_radius), so on '+' the
offsets run from -(R - 1) to R and on '-' from -R to R - 1; the same table otherwise."""
import argparse
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from mural_amd.data.ingest import read_bed, read_fasta  # noqa: E402
from mural_amd.model.nn_utils import load_model  # noqa: E402
from mural_amd.mutagenesis import saturation_mutagenesis  # noqa: E402


def output_name(prefix):
    return prefix + ".mutagenesis.tsv"


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
    ap.add_argument("--batch_sites", type=int, default=64, help="sites per map held on the device")
    args = ap.parse_args(argv)
    if args.top is not None and args.top < 1:
        raise SystemExit("--top must be positive")
    model, cfg = load_model(args.model_path, args.model_config_path, model_type=args.model_type)
    bed = read_bed(args.sites)
    out, rows = output_name(args.out), 0
    with open(out, "w") as fh:
        header = ["chrom", "site_start", "strand", "offset", "genomic_pos", "ref", "alt"]
        fh.write("\t".join(header + [f"delta_logp{c + 1}" for c in range(cfg["n_class"])]) + "\n")
        for cid, chrom in enumerate(bed.chrom_names):
            sel = np.nonzero(bed.chrom_id == cid)[0]
            genome = read_fasta(args.ref_genome, "cuda", names=[chrom]).get(chrom)
            if genome is None:
                raise SystemExit(f"{args.sites}: chromosome {chrom} is not in {args.ref_genome}")
            for b0 in range(0, len(sel), args.batch_sites):
                part = sel[b0:b0 + args.batch_sites]
                pos = torch.from_numpy(bed.start[part]).cuda()
                strand = torch.from_numpy(bed.strand[part]).cuda()
                if args.model_type == "indel":
                    res = saturation_mutagenesis(model, genome, pos, strand, distal_radius=cfg["distal_radius"])
                else:
                    res = saturation_mutagenesis(model, genome, pos, strand, cfg["local_radius"], cfg.get("local_order", 3))
                rows += write_rows(fh, chrom, res, args.top)
    print(f"{len(bed.start)} sites, {rows} rows -> {out}")


if __name__ == "__main__":
    main()
