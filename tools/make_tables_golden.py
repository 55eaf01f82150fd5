"""Record the reference's outputs for the prediction-table tools into tests/golden/tables.npz.

Runs only where the reference tree is present (oracle/ref_import.py: MURAL_REFERENCE_ROOT); never on a GPU machine.  It imports the
reference's own MuRaL/scripts/scaling.py, calc_kmer_corr.py and calc_regional_corr.py and feeds them the seeded cases of
tests/_tables_data.py.  Three libraries those scripts import are absent here and are replaced by small functional stand-ins:

  Bio.SeqIO.parse            FASTA records with .id (text after '>' up to white space) and .seq
  Bio.Seq.reverse_complement A<->T, C<->G, reversed
  pybedtools.BedTool         from a path (chrom start end ...) or from_dataframe; to_dataframe; intersect(b): every row of
                             self once per region of b on its chromosome with b.start < row.end and row.start < b.end, in
                             self's order -- bedtools intersect without -u.

The benchmark-region parity of calc_scaling_factor therefore rests on this restatement of bedtools' counting rule, not on bedtools.

    python tools/make_tables_golden.py
"""
import contextlib
import io
import os
import sys
import tempfile
import types

import numpy as np
import pandas as pd

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from tests import _tables_data as D  # noqa: E402


# ---------------------------------------------------------------------------------------------------------------------------------
# stand-ins
# ---------------------------------------------------------------------------------------------------------------------------------
class _Record:
    def __init__(self, rid, seq):
        self.id, self.seq = rid, seq


def _parse(path, fmt):
    assert fmt == "fasta"
    rid, parts = None, []
    with open(path) as fh:
        for line in fh:
            if line.startswith(">"):
                if rid is not None:
                    yield _Record(rid, "".join(parts))
                rid, parts = line[1:].split()[0], []
            else:
                parts.append(line.strip())
    if rid is not None:
        yield _Record(rid, "".join(parts))


_COMP = str.maketrans("ACGTacgtN", "TGCAtgcaN")


def _reverse_complement(s):
    return str(s).translate(_COMP)[::-1]


class BedTool:
    def __init__(self, src=None):
        if isinstance(src, pd.DataFrame):
            self.df = src.reset_index(drop=True)
        else:
            rows = [ln.split("\t")[:3] for ln in open(os.fspath(src)).read().splitlines() if ln.strip()]
            self.df = pd.DataFrame({"chrom": [r[0] for r in rows], "start": [int(r[1]) for r in rows], "end": [int(r[2]) for r in rows]})

    @classmethod
    def from_dataframe(cls, df):
        out = df.copy()
        out.columns = ["chrom", "start", "end", "name", "score", "strand"][:out.shape[1]]
        out["chrom"] = out["chrom"].astype(str)
        return cls(out)

    def intersect(self, other):
        reg = {}
        for c, a, b in zip(other.df["chrom"], other.df["start"], other.df["end"]):
            reg.setdefault(str(c), []).append((int(a), int(b)))
        keep = []
        for i, (c, s, e) in enumerate(zip(self.df["chrom"], self.df["start"], self.df["end"])):
            keep.extend(i for a, b in reg.get(str(c), ()) if a < int(e) and int(s) < b)
        return BedTool(self.df.iloc[keep])

    def to_dataframe(self):
        return self.df.copy()


def _install_standins():
    bio, seqio, seqm, pbt = (types.ModuleType(n) for n in ("Bio", "Bio.SeqIO", "Bio.Seq", "pybedtools"))
    bio.__path__ = []
    seqio.parse = _parse
    seqm.reverse_complement = _reverse_complement
    bio.SeqIO, bio.Seq = seqio, seqm
    pbt.BedTool = BedTool
    sys.modules.update({"Bio": bio, "Bio.SeqIO": seqio, "Bio.Seq": seqm, "pybedtools": pbt})


def _load_reference():
    _install_standins()
    from oracle import ref_import
    ref_import.load()
    import importlib
    return (importlib.import_module("MuRaL.scripts.scaling"), importlib.import_module("MuRaL.scripts.calc_kmer_corr"),
            importlib.import_module("MuRaL.scripts.calc_regional_corr"))


def _read(path):
    with open(path) as fh:
        return fh.read()


def record():
    scaling, kmer, regional = _load_reference()
    out = {}
    with tempfile.TemporaryDirectory() as d:
        for name in D.CASES:
            c = D.case(name)
            table, fasta, bed = D.write_case(d, name)
            nc, mt = c["n_class"], c["model_type"]
            scaled = os.path.join(d, f"{name}.scaled.tsv")
            scaling.apply_scaling(table, D.SCALE_FACTOR, nc, scaled)
            out[f"{name}/scale"] = _read(scaled)
            for tag, regions in (("all", ""), ("bench", bed)):
                args = types.SimpleNamespace(benchmark_regions=regions, genomewide_mu=D.GENOMEWIDE_MU, g_proportions=[D.G_PROP],
                                             m_proportions=[D.M_PROP], pred_files=[table], do_scaling=False, n_class=nc)
                buf = io.StringIO()
                with contextlib.redirect_stdout(buf):
                    factor = scaling.calc_mu_scaling_factor(args, mt)
                n_sites = [int(ln.split()[1]) for ln in buf.getvalue().splitlines() if ln.startswith("n_sites:")][0]
                out[f"{name}/factor_{tag}"] = np.float64(factor)
                out[f"{name}/n_sites_{tag}"] = np.int64(n_sites)
                out[f"{name}/stdout_{tag}"] = buf.getvalue().replace(table, "<pred>")
            for k in c["kmers"]:
                for strand in c["strands"]:
                    prefix = os.path.join(d, "kmer")
                    args = types.SimpleNamespace(pred_file=table, ref_genome=fasta, out_prefix=prefix, kmer_length=k, n_class=nc,
                                                 strand=strand)
                    kmer.run_kmer_corr_calc(args, mt)
                    key = f"{name}/kmer{k}_{D.strand_tag(strand)}"
                    out[key + "/rates"] = _read(f"{prefix}.{k}-mer.mut_rates.tsv")
                    out[key + "/corr"] = _read(f"{prefix}.{k}-mer.corr.txt")
            for w in c["windows"]:
                prefix = os.path.join(d, "region")
                args = types.SimpleNamespace(pred_file=table, window_size=w, ratio_cutoff=0.2, n_class=nc, out_prefix=prefix)
                regional.run_regional_corr_calc(args)
                window = f"{int(int(w) / 1000)}Kb"
                out[f"{name}/win{w}/rates"] = _read(f"{prefix}.{window}.mut_rates.tsv")
                out[f"{name}/win{w}/corr"] = _read(f"{prefix}.{window}.corr.txt")
    np.savez_compressed(D.GOLDEN, **{k: (np.str_(v) if isinstance(v, str) else v) for k, v in out.items()})
    print(f"wrote {D.GOLDEN}: {len(out)} entries, {os.path.getsize(D.GOLDEN)} bytes")


if __name__ == "__main__":
    record()
