"""CPU tests of the prediction-table tools' host logic (mural_amd.tables): header validation, output file names, argument errors,
and the fixture of tests/golden/tables.npz checked against a numpy restatement of the reference scripts on the seeded inputs."""
import gzip

import numpy as np
import pytest

from tests import _tables_data as D


def test_header_validation_messages():
    from mural_amd import tables
    head = "chrom\tstart\tend\tstrand\tmut_type\tprob0\tprob1\tprob2\tprob3"
    assert tables.check_header(head, 4)[-1] == "prob3"
    with pytest.raises(ValueError, match=r"Invalid file header: start\tend, header should be continue with 'chrom'"):
        tables.check_header("start\tend", 4)
    with pytest.raises(ValueError, match="Column count mismatch. Expected 13 columns, got 9 in line"):
        tables.check_header(head, 8)


def test_read_header_plain_and_gzip(tmp_path):
    from mural_amd import tables
    text = "chrom\tstart\r\nx\t1\n"
    (tmp_path / "a.tsv").write_text(text)
    (tmp_path / "b.bin").write_bytes(gzip.compress(text.encode()))      # gzip is recognised by its magic bytes, not the name
    assert tables.read_header(str(tmp_path / "a.tsv")) == "chrom\tstart"
    assert tables.read_header(str(tmp_path / "b.bin")) == "chrom\tstart"


def test_output_names():
    from mural_amd import tables
    assert tables.kmer_output_names("out/p", 5) == ("out/p.5-mer.mut_rates.tsv", "out/p.5-mer.corr.txt")
    assert tables.regional_output_names("p", 100000) == ("p.100Kb.mut_rates.tsv", "p.100Kb.corr.txt", "100Kb")
    assert tables.regional_output_names("p", 2500)[2] == "2Kb"
    assert tables.scaled_output_name("x.tsv.gz") == "x.tsv.gz.scaled.tsv.gz"


def test_argument_errors():
    from mural_amd import tables
    assert tables.check_kmer_length(10) == 10
    with pytest.raises(ValueError, match="larger than 10"):
        tables.check_kmer_length(11)
    with pytest.raises(ValueError):
        tables.check_kmer_length(0)
    assert tables.strand_mode("snv") == 0
    assert [tables.strand_mode("indel", s) for s in ("pos", "+", "neg", "-", "both")] == [1, 1, 2, 2, 3]
    with pytest.raises(ValueError, match="Invalid strand"):
        tables.strand_mode("indel", "up")
    with pytest.raises(ValueError, match="not supported"):
        tables.strand_mode("cnv")
    assert tables.kmer_name(0b000110_11, 4) == "ACGT"


def test_the_legacy_name_is_not_the_in_memory_rule():
    from mural_amd import calibration, tables
    assert tables.apply_scaling is tables.apply_scaling_file
    assert calibration.apply_scaling is not tables.apply_scaling


def _rows(text):
    lines = text.rstrip("\n").split("\n")
    return lines[0].split("\t"), [ln.split("\t") for ln in lines[1:]]


@pytest.mark.parametrize("name", D.CASES)
def test_fixture_against_numpy_restatement(name):
    """scale, calc_scaling_factor and the regional counts of the fixture, restated in numpy on the seeded inputs."""
    g = np.load(D.GOLDEN)
    c = D.case(name)
    nc = c["n_class"]
    head, rows = _rows(c["table"])
    prob = np.array([[float(v) for v in r[5:]] for r in rows])
    start = np.array([int(r[1]) for r in rows])
    end = np.array([int(r[2]) for r in rows])
    chrom = [r[0] for r in rows]
    # scale: prob1.. *= f, prob0 = 1 - their sum, '%.4g'
    sc = prob[:, 1:] * D.SCALE_FACTOR
    p0 = np.zeros(len(rows))
    for j in range(nc - 1):
        p0 = p0 + sc[:, j]
    want = "\t".join(head) + "\n" + "".join(
        "\t".join(r[:5] + ["%.4g" % (1 - s)] + ["%.4g" % v for v in q]) + "\n" for r, s, q in zip(rows, p0, sc))
    assert str(g[f"{name}/scale"]) == want
    # factor: mu * n_sites * m / g / prob_sum, with regions a row counting once per overlapping region
    gp = D.G_PROP if c["model_type"] == "snv" else 1
    rs = prob[:, 1:].sum(axis=1)
    assert int(g[f"{name}/n_sites_all"]) == len(rows)
    f = D.GENOMEWIDE_MU * len(rows) * D.M_PROP / gp / rs.sum()
    assert abs(float(g[f"{name}/factor_all"]) - f) <= 1e-12 * f
    regs = [ln.split("\t") for ln in c["bed"].splitlines()]
    w = np.array([sum(1 for rc, a, b in regs if rc == ch and int(a) < e and s < int(b)) for ch, s, e in zip(chrom, start, end)])
    assert int(g[f"{name}/n_sites_bench"]) == w.sum()
    f = D.GENOMEWIDE_MU * w.sum() * D.M_PROP / gp / (w * rs).sum()
    assert abs(float(g[f"{name}/factor_bench"]) - f) <= 1e-12 * f
    # regional: rows per (chrom, window_end) in first-appearance order
    W = c["windows"][-1]
    keys = {}
    for ch, s in zip(chrom, start):
        k = (ch, s // W * W + W)
        keys[k] = keys.get(k, 0) + 1
    _, reg = _rows(str(g[f"{name}/win{W}/rates"]))
    assert [(r[0], int(r[1])) for r in reg] == list(keys)
    assert [int(r[-2]) for r in reg] == list(keys.values())
