"""The prediction-table tools on the device (mural_amd.tables) against the reference scripts' own outputs (tests/golden/tables.npz,
recorded by tools/make_tables_golden.py on the seeded cases of tests/_tables_data.py): scale, calc_scaling_factor, k-mer and
regional evaluation, chunk boundaries and the errors."""
import contextlib
import gzip
import io
import types

import numpy as np
import pytest

from tests import _tables_data as D

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def golden():
    return np.load(D.GOLDEN)


@pytest.fixture(scope="module")
def files(tmp_path_factory):
    d = tmp_path_factory.mktemp("tables")
    out = {}
    for name in D.CASES:
        out[name] = D.write_case(str(d), name)
        out[name + ".gz"] = D.write_case(str(d), name, gz=True)
    return out


def _text(path):
    with open(path, "rb") as fh:
        raw = fh.read()
    return (gzip.decompress(raw) if raw[:2] == b"\x1f\x8b" else raw).decode()


def _cmp_rates(got, want, f32=False):
    g = [ln.split("\t") for ln in got.splitlines()]
    w = [ln.split("\t") for ln in want.splitlines()]
    assert g[0] == w[0]
    assert len(g) == len(w)
    for gr, wr in zip(g[1:], w[1:]):
        assert len(gr) == len(wr)
        for h, a, b in zip(w[0], gr, wr):
            if not h.startswith("avg_"):
                assert a == b, (h, gr, wr)      # group names, row order, counts, used_or_deprecated
            elif f32:
                ua, ub = np.float32(a).view(np.int32), np.float32(b).view(np.int32)
                assert abs(int(ua) - int(ub)) <= 1, (h, a, b)
            else:
                fa, fb = float(a), float(b)
                assert fa == fb or abs(fa - fb) <= 1e-12 * abs(fb), (h, a, b)


def _cmp_corr(got, want):
    g = [ln.split("\t") for ln in got.splitlines()]
    w = [ln.split("\t") for ln in want.splitlines()]
    assert len(g) == len(w)
    for gr, wr in zip(g, w):
        assert gr[:3] == wr[:3], (gr, wr)        # label, class, r to 5 decimals
        pa, pb = float(gr[3]), float(wr[3])
        assert pa == pb or abs(pa - pb) <= 1e-9 * abs(pb), (gr, wr)


@pytest.mark.parametrize("name", D.CASES)
@pytest.mark.parametrize("gz_in,gz_out", [(False, False), (True, True), (False, True)])
def test_scale_matches_reference(files, golden, tmp_path, name, gz_in, gz_out):
    from mural_amd import tables
    table = files[name + (".gz" if gz_in else "")][0]
    out = str(tmp_path / ("scaled.tsv" + (".gz" if gz_out else "")))
    tables.scaling_files([table], [D.SCALE_FACTOR], D.case(name)["n_class"], [out])
    if gz_out:
        assert open(out, "rb").read(2) == b"\x1f\x8b"
    # byte-identical: the seeded SNV table's digit-only chromosome '01' shares its column with other names, so pandas keeps it a
    # string there too (pandas re-types it only in a table whose every chromosome name is a number -- the documented deviation)
    assert _text(out) == str(golden[f"{name}/scale"])


@pytest.mark.parametrize("name", D.CASES)
@pytest.mark.parametrize("tag", ["all", "bench"])
def test_scaling_factor_matches_reference(files, golden, tmp_path, name, tag):
    from mural_amd import tables
    c = D.case(name)
    table, _, bed = files[name + ".gz"]
    args = types.SimpleNamespace(benchmark_regions=bed if tag == "bench" else "", genomewide_mu=D.GENOMEWIDE_MU,
                                 g_proportions=[D.G_PROP], m_proportions=[D.M_PROP], pred_files=[table], do_scaling=True,
                                 n_class=c["n_class"])
    buf = io.StringIO()
    with contextlib.redirect_stdout(buf):
        (factor,) = tables.calc_mu_scaling_factor(args, c["model_type"])
    want = float(golden[f"{name}/factor_{tag}"])
    assert abs(factor - want) <= 1e-12 * abs(want)
    _, n_sites = tables.prob_sum_file(table, c["n_class"], bed if tag == "bench" else None)
    assert n_sites == int(golden[f"{name}/n_sites_{tag}"])
    got_lines = buf.getvalue().replace(table, "<pred>").splitlines()
    want_lines = str(golden[f"{name}/stdout_{tag}"]).splitlines()
    assert [ln for ln in got_lines if not ln.startswith(("prob_sum", "scaling factor"))] == \
        [ln for ln in want_lines if not ln.startswith(("prob_sum", "scaling factor"))]
    # --do_scaling: <pred>.scaled.tsv.gz through the scaling path
    scaled = _text(tables.scaled_output_name(table))
    assert scaled.split("\n", 1)[0] == str(golden[f"{name}/scale"]).split("\n", 1)[0]
    assert scaled.count("\n") == str(golden[f"{name}/scale"]).count("\n")


def _kmer_params():
    out = []
    for name in D.CASES:
        c = D.case(name)
        out += [(name, k, s) for k in c["kmers"] for s in c["strands"]]
    return out


@pytest.mark.parametrize("name,k,strand", _kmer_params())
def test_kmer_corr_matches_reference(files, golden, tmp_path, name, k, strand):
    from mural_amd import tables
    c = D.case(name)
    table, fasta, _ = files[name]
    prefix = str(tmp_path / "kmer")
    args = types.SimpleNamespace(pred_file=table, ref_genome=fasta, out_prefix=prefix, kmer_length=k, n_class=c["n_class"], strand=strand)
    tables.run_kmer_corr_calc(args, c["model_type"])
    rates, corr = tables.kmer_output_names(prefix, k)
    key = f"{name}/kmer{k}_{D.strand_tag(strand)}"
    _cmp_rates(open(rates).read(), str(golden[key + "/rates"]))
    _cmp_corr(open(corr).read(), str(golden[key + "/corr"]))


@pytest.mark.parametrize("name,w", [(n, w) for n in D.CASES for w in D.case(n)["windows"]])
def test_regional_corr_matches_reference(files, golden, tmp_path, name, w):
    from mural_amd import tables
    c = D.case(name)
    table = files[name + ".gz"][0]
    prefix = str(tmp_path / "region")
    args = types.SimpleNamespace(pred_file=table, window_size=w, ratio_cutoff=0.2, n_class=c["n_class"], out_prefix=prefix)
    tables.run_regional_corr_calc(args)
    rates, corr, _ = tables.regional_output_names(prefix, w)
    _cmp_rates(open(rates).read(), str(golden[f"{name}/win{w}/rates"]), f32=True)
    _cmp_corr(open(corr).read(), str(golden[f"{name}/win{w}/corr"]))


@pytest.mark.parametrize("chunk_bytes", [1, 97, 1000, 4096])
def test_chunk_boundaries(files, golden, tmp_path, chunk_bytes):
    """Rows and chromosome runs straddle chunks (chunk_bytes = 1: one row per chunk); every output stays the same."""
    from mural_amd import tables
    name = "snv"
    table, fasta, bed = files[name + (".gz" if chunk_bytes % 2 else "")]
    out = str(tmp_path / "scaled.tsv")
    tables.scaling_files([table], [D.SCALE_FACTOR], 4, [out], chunk_bytes=chunk_bytes)
    assert _text(out) == str(golden[f"{name}/scale"])
    _, n_sites = tables.prob_sum_file(table, 4, bed, chunk_bytes=chunk_bytes)
    assert n_sites == int(golden[f"{name}/n_sites_bench"])
    prefix = str(tmp_path / "r")
    args = types.SimpleNamespace(pred_file=table, ref_genome=fasta, out_prefix=prefix, kmer_length=5, n_class=4, strand=None)
    tables.run_kmer_corr_calc(args, "snv", chunk_bytes=chunk_bytes)
    _cmp_rates(open(tables.kmer_output_names(prefix, 5)[0]).read(), str(golden[f"{name}/kmer5_row/rates"]))
    args = types.SimpleNamespace(pred_file=table, window_size=1000, ratio_cutoff=0.2, n_class=4, out_prefix=prefix)
    tables.run_regional_corr_calc(args, chunk_bytes=chunk_bytes)
    _cmp_rates(open(tables.regional_output_names(prefix, 1000)[0]).read(), str(golden[f"{name}/win1000/rates"]), f32=True)


def test_one_chunk_of_more_tiles_than_scan_threads(tmp_path):
    """A chunk's newline counts per tile of 4096 bytes are scanned by ONE workgroup of 256 threads (nl_scan_kernel): a table of a
    little over 1 MiB read as one chunk has more tiles than that, so a thread owns a run of two tiles and the last threads none.
    Row for row -- every column goes through the scaled table's text -- it equals the same file read in chunks of 4096 bytes (one
    tile each), the route that test_chunk_boundaries ties to the reference."""
    from mural_amd import tables
    rng = np.random.default_rng(11)
    n = 26_000
    start = np.cumsum(rng.integers(1, 2000, size=n))
    prob = rng.dirichlet([40, 1, 1, 1], size=n)
    lines = [_HEAD]
    for i in range(n):
        lines.append("chr%d\t%d\t%d\t%s\t%d\t%s" % (1 + i * 3 // n, start[i], start[i] + 1, "+-"[i % 7 == 0], i % 4,
                                                   "\t".join("%.4g" % p for p in prob[i])))
    table = _bad_table(tmp_path, lines)
    size = len(open(table, "rb").read())
    assert 257 * 4096 < size < (1 << 21)
    texts = []
    for chunk_bytes in (1 << 21, 4096):
        out = str(tmp_path / f"scaled{chunk_bytes}.tsv")
        tables.apply_scaling_file(table, 0.5, 4, out, chunk_bytes=chunk_bytes)
        texts.append(_text(out).splitlines())
    assert len(texts[0]) == n + 1 and texts[0] == texts[1]


def _bad_table(tmp_path, lines, gz=False):
    text = "".join(ln + "\n" for ln in lines)
    p = tmp_path / ("bad.tsv" + (".gz" if gz else ""))
    p.write_bytes(gzip.compress(text.encode()) if gz else text.encode())
    return str(p)


_HEAD = "chrom\tstart\tend\tstrand\tmut_type\tprob0\tprob1\tprob2\tprob3"
_ROW = "chrA\t10\t11\t+\t0\t0.9\t0.05\t0.03\t0.02"


@pytest.mark.parametrize("row,what", [("chrA\t10\t11\t+\t0\t0.9\t0.05\t0.03", "wrong number of columns"),
                                      ("chrA\t10\t11\t+\t0\t0.9\t0.05\t0.03\t0.02\t0.1", "wrong number of columns"),
                                      ("chrA\t10\t11\t+\t0\t0.9\t0.0x5\t0.03\t0.02", "malformed number"),
                                      ("chrA\t10\t11\t+\t0\tnan\t0.05\t0.03\t0.02", "malformed number"),
                                      ("chrA\t1x0\t11\t+\t0\t0.9\t0.05\t0.03\t0.02", "malformed number"),
                                      ("chrA\t10\t11\t.\t0\t0.9\t0.05\t0.03\t0.02", "strand")])
@pytest.mark.parametrize("gz", [False, True])
def test_malformed_rows_raise_with_the_row(tmp_path, row, what, gz):
    from mural_amd import tables
    path = _bad_table(tmp_path, [_HEAD] + [_ROW] * 40 + [row] + [_ROW] * 5, gz)
    for chunk in (tables.DEFAULT_CHUNK_BYTES, 64):
        with pytest.raises(ValueError, match=f"line 42\\b.*{what}"):
            tables.prob_sum_file(path, 4, chunk_bytes=chunk)


def test_header_errors(tmp_path):
    from mural_amd import tables
    with pytest.raises(ValueError, match="header should be continue with 'chrom'"):
        tables.prob_sum_file(_bad_table(tmp_path, ["position\tstart", _ROW]), 4)
    with pytest.raises(ValueError, match="Column count mismatch. Expected 9 columns, got 8"):
        tables.prob_sum_file(_bad_table(tmp_path, [_HEAD.rsplit("\t", 1)[0], _ROW]), 4)


def test_missing_chromosome_and_large_k(files, tmp_path):
    from mural_amd import tables
    _, fasta, _ = files["snv"]
    path = _bad_table(tmp_path, [_HEAD, _ROW.replace("chrA", "chrZ")])
    args = types.SimpleNamespace(pred_file=path, ref_genome=fasta, out_prefix=str(tmp_path / "x"), kmer_length=3, n_class=4, strand=None)
    with pytest.raises(ValueError, match="Chromosome chrZ not found .*line 2"):
        tables.run_kmer_corr_calc(args, "snv")
    args.kmer_length = 11
    with pytest.raises(ValueError, match="larger than 10"):
        tables.run_kmer_corr_calc(args, "snv")


def test_empty_table_and_no_final_newline(tmp_path):
    from mural_amd import tables
    assert tables.prob_sum_file(_bad_table(tmp_path, [_HEAD]), 4) == (0.0, 0)
    p = tmp_path / "nonl.tsv"
    p.write_text(_HEAD + "\n" + _ROW + "\n" + _ROW)
    s, n = tables.prob_sum_file(str(p), 4)
    assert n == 2 and abs(s - 2 * (0.05 + 0.03 + 0.02)) < 1e-15
