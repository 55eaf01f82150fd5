"""Record the reference's motif correlation outputs into tests/golden/motif.npz.

Runs only where the reference tree is present (oracle/ref_import.py: MURAL_REFERENCE_ROOT); never on a GPU machine.  It imports the
reference's own MuRaL/scripts/calc_motif_corr.py with the functional stand-ins of tools/make_tables_golden.py for Bio.SeqIO.parse and
Bio.Seq.reverse_complement, and runs its run_motif_corr_calc on the seeded cases of tests/_motif_data.py.  Two more things the script
needs as it stands: the name `data` it calls extend_interval through is bound to the reference's MuRaL.data package (the script imports
only MuRaL.data.preprocessing), and an INDEL run is given a `strand` (assigned per row and never read).

Per case and motif length the fixture holds the text of the two files the reference wrote -- the entry names in order, the rates and
the counts, and the correlation lines; tests/_motif_data.golden parses them.

    python tools/make_motif_golden.py
"""
import importlib
import os
import sys
import tempfile
import types

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from tests import _motif_data as D  # noqa: E402
from tools import make_tables_golden as G  # noqa: E402


def _load_reference():
    G._install_standins()
    from oracle import ref_import
    ref_import.load()
    motif = importlib.import_module("MuRaL.scripts.calc_motif_corr")
    motif.data = importlib.import_module("MuRaL.data")
    importlib.import_module("MuRaL.data.preprocessing")
    return motif


def record():
    motif = _load_reference()
    out = {}
    with tempfile.TemporaryDirectory() as d:
        for name in D.CASES:
            c = D.case(name)
            table, fasta = D.write_case(d, name)
            nc = c["n_class"]
            for m in D.MOTIFS:
                prefix = os.path.join(d, "motif")
                args = types.SimpleNamespace(pred_file=table, ref_genome=fasta, out_prefix=prefix, motif_length=m, n_class=nc, strand="+")
                motif.run_motif_corr_calc(args, c["model_type"])
                rates, corr = G._read(f"{prefix}.{m}-motif.mut_rates.tsv"), G._read(f"{prefix}.{m}-motif.corr.txt")
                key = f"{name}/motif{m}"
                out[key + "/rates"], out[key + "/corr"] = rates, corr
    np.savez_compressed(D.GOLDEN, **{k: (np.str_(v) if isinstance(v, str) else v) for k, v in out.items()})
    print(f"wrote {D.GOLDEN}: {len(out)} entries, {os.path.getsize(D.GOLDEN)} bytes")


if __name__ == "__main__":
    record()
