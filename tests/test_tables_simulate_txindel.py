"""The INDEL structure simulation from a written table (mural_amd.tables.simulate_indel_structure_table, run_simulate_indel_structure_calc),
its writer (write_indel_structure_simulation_outputs: the observed / expected columns are those of the INDEL structure file, 'NA' without
labels) and the command line's refusals, one line each."""
import os
import subprocess
import sys

import numpy as np
import pytest

from tests import _conseq_data as D
from tests import _txindel_sim_data as X

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
R, SEED = 33, 12345


def _rows():
    prob, start, strand, label = X.rows(400, 8, seed=7, extra=40)
    prob = np.array([[float("%.4g" % v) for v in row] for row in prob])      # what the table's text holds; class 0 is never read
    return prob, start, strand, label


def _write_table(path, prob, start, strand, label):
    head = "chrom\tstart\tend\tstrand\tmut_type\t" + "\t".join(f"prob{c}" for c in range(8))
    lines = [head] + ["\t".join(["chr1", str(s), str(s + 1), "+-"[int(m)], str(int(lab))] + ["%.4g" % v for v in p])
                      for p, s, m, lab in zip(prob, start, strand, label)]
    path.write_text("\n".join(lines) + "\n")


@pytest.mark.gpu
@pytest.mark.parametrize("kind", ["insertion", "deletion_end"])
def test_table_route_and_writer_on_a_written_table(tmp_path, kind):
    from mural_amd import tables
    from mural_amd.summaries import simulate_chrom_key, simulate_indel_lof_counts, simulate_txindel_host, summary_txindel_host
    text = X.toy_text() + X.random_text(seed=4, n_tx=8, span=(40, 700))
    bed = tmp_path / "tx.bed"
    bed.write_text(text)
    names, segments, features = X.read(text)
    prob, start, strand, label = _rows()
    out = tmp_path / "t.tsv"
    _write_table(out, prob, start, strand, label)
    got = tables.simulate_indel_structure_table(str(out), str(bed), 8, kind, R, SEED, chrom_lengths={"chr1": 640}, chunk_bytes=16 << 10)
    k = tables.check_indel_kind(kind)
    want, status = simulate_txindel_host(prob, start, strand, 8, segments, features, len(names), k, simulate_chrom_key("chr1"), SEED, R,
                                         chrom_length=640)
    lof, upper = simulate_indel_lof_counts(want)
    assert status == 0 and got[0] == names and got[1].tobytes() == want.tobytes() and want.any()
    assert np.array_equal(got[2], lof) and np.array_equal(got[3], upper)
    table, rows, _ = summary_txindel_host(prob, start, label, 8, segments, features, len(names), k, chrom_length=640)
    expected, observed = tables.indel_structure_cells_from_sums(table)
    assert got[4] == observed and got[5] == expected

    class Args:
        pred_file, indel_transcripts, n_class, indel_kind, out_prefix, chrom_lengths, simulate, seed = str(out), str(bed), 8, kind, str(tmp_path / "calc"), {"chr1": 640}, R, SEED
    sim = [ln.split("\t") for ln in open(tables.run_simulate_indel_structure_calc(Args)).read().splitlines()]
    plain = [ln.split("\t") for ln in open(tables.run_indel_structure_calc(Args)).read().splitlines()]
    assert sim[0] == ["name", "bin", "observed", "expected", "sim_mean", "sim_min", "sim_max", "n_ge", "n_le", "p_upper", "p_lower"]
    assert len(sim) == 1 + 12 * len(names)
    what_all = tables.INDEL_STRUCTURE_BINS + ("lof", "lof_upper")
    for t, line in enumerate(plain[1:]):      # the observed / expected columns are the INDEL structure file's
        for b, what in enumerate(what_all):
            row = sim[1 + 12 * t + b]
            assert row[:2] == [line[0], what]
            assert row[3] == line[plain[0].index(f"expected_{what}")] and row[2] == line[plain[0].index(f"observed_{what}")]
            column = want[t, b] if b < 10 else (lof, upper)[b - 10][t]
            n_ge = int((column >= int(row[2])).sum())
            assert int(row[5]) == column.min() and int(row[6]) == column.max() and int(row[7]) == n_ge
            assert row[9] == tables._float_text((n_ge + 1) / (R + 1))


def test_writer_without_labels_and_the_existing_file_is_unchanged(tmp_path):
    from mural_amd import tables
    from mural_amd.summaries import simulate_indel_lof_counts, simulate_txindel_host, summary_txindel_host
    text = X.toy_text()
    names, segments, features = X.read(text)
    prob, start, strand, label = _rows()
    counts, _ = simulate_txindel_host(prob, start, strand, 8, segments, features, 2, 1, X.KEY, SEED, R)
    table, rows, _ = summary_txindel_host(prob, start, label, 8, segments, features, 2, 1)
    expected, observed = tables.indel_structure_cells_from_sums(table)
    lof, upper = simulate_indel_lof_counts(counts)
    path = tables.write_indel_structure_simulation_outputs(names, counts, lof, upper, None, expected, str(tmp_path / "na"))
    assert path.endswith("na.indel_structure.sim.tsv")
    lines = [ln.split("\t") for ln in open(path).read().splitlines()[1:]]
    assert len(lines) == 24 and all(f[2] == "NA" and f[7:] == ["NA"] * 4 and f[3] != "NA" and f[4] != "NA" for f in lines)
    # the INDEL structure file through the shared helper: the numbers of the formula it documents, formed here on their own
    meta = dict(chrom=["chr1", "chr1"], strand=[0, 1])
    got = [ln.split("\t") for ln in open(tables.write_indel_structure_outputs(names, meta, table, rows, 1, str(tmp_path / "s"))).read().splitlines()]
    cells = table.tolist()
    for t in range(2):
        twelve = cells[t] + [[sum(cells[t][b][w] for b in (3, 6, 7)) for w in range(3)]]
        twelve.append([twelve[10][w] + cells[t][9][w] for w in range(3)])
        flat = []
        for count, hi, lo in twelve:
            flat += [tables._float_text(((hi << 40) + lo) / (1 << 71)), str(count)]
        assert got[1 + t][6:] == flat


_ALL = ["--indel", "--summary", "P", "--indel_transcripts", "T", "--indel_kind", "insertion", "--simulate", "5", "--seed", "3",
        "--simulate_indel_structure"]


def _drop(*names):
    out, skip = [], 0
    for a in _ALL:
        if skip:
            skip -= 1
        elif a in names:
            skip = 0 if a in ("--indel", "--simulate_indel_structure") else 1
        else:
            out.append(a)
    return out


@pytest.mark.parametrize("argv,what", [
    (_drop("--indel_transcripts", "--indel_kind"), "--simulate_indel_structure needs --indel_transcripts"),
    (_drop("--simulate", "--seed"), "--simulate_indel_structure needs --simulate R --seed S"),
    (_drop("--seed"), "--simulate_indel_structure needs --simulate R --seed S"),
    (_drop("--indel"), "--indel"),
])
def test_command_line_refusals_are_one_line(argv, what, tmp_path):
    (tmp_path / "tx.bed").write_text(D.bed12("chr1", "t", "+", [(0, 30)]) + "\n")
    argv = [str(tmp_path / "tx.bed") if a == "T" else a for a in argv]
    done = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "predict_files.py"), "m", "f", "b", "o"] + argv, capture_output=True,
                          text=True, cwd=ROOT)
    assert done.returncode != 0
    message = done.stderr.strip().splitlines()
    assert len(message) == 1 and what in message[0], done.stderr


def test_the_sink_names_what_is_missing():
    import io
    from mural_amd.predict import SummarySink
    text = X.toy_text()
    with pytest.raises(ValueError, match="simulate_indel_structure needs simulate=R with simulate_seed"):
        SummarySink(None, indel_transcripts=io.StringIO(text), indel_kind="insertion", simulate_indel_structure=True)
    with pytest.raises(ValueError, match="simulate_indel_structure needs indel_transcripts="):
        SummarySink(None, simulate=4, simulate_seed=1, simulate_indel_structure=True)
    with pytest.raises(ValueError, match="simulate_table_bytes_max"):
        SummarySink(None, indel_transcripts=io.StringIO(text), indel_kind="insertion", simulate=1000, simulate_seed=1,
                    simulate_indel_structure=True, simulate_table_bytes_max=1000)
    SummarySink(None, indel_transcripts=io.StringIO(text), indel_kind="insertion", simulate=4, simulate_seed=1, simulate_indel_structure=True)
