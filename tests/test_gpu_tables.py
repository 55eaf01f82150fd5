"""The prediction-table tools on the device (mural_amd.tables) against the reference scripts' own outputs (tests/golden/tables.npz,
recorded by tools/make_tables_golden.py on the seeded cases of tests/_tables_data.py): scale, calc_scaling_factor, k-mer and
regional evaluation, chunk boundaries and the errors."""
import contextlib
import ctypes as C
import gzip
import io
import types

import numpy as np
import pytest

from mural_amd import _lib
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


# fields outside the grammar of csrc/tables.hip (number = [+-] digits [. digits] [(e|E) [+-] digits] with a digit in the mantissa;
# integer = [+-] 1 .. 18 digits), in the prob1 column: Python's float() takes several of them
_NOT_NUMBERS = [".", "e5", "1e", "1e+", "1.2.3", "0x10", "1_0", " 1", "1 ", "inf", "nan", "--1", ""]


@pytest.mark.parametrize("row,what", [("chrA\t10\t11\t+\t0\t0.9\t0.05\t0.03", "wrong number of columns"),
                                      ("chrA\t10\t11\t+\t0\t0.9\t0.05\t0.03\t0.02\t0.1", "wrong number of columns"),
                                      ("chrA\t10\t11\t+\t0\t0.9\t0.0x5\t0.03\t0.02", "malformed number"),
                                      ("chrA\t10\t11\t+\t0\tnan\t0.05\t0.03\t0.02", "malformed number"),
                                      ("chrA\t1x0\t11\t+\t0\t0.9\t0.05\t0.03\t0.02", "malformed number"),
                                      ("chrA\t10\t11\t.\t0\t0.9\t0.05\t0.03\t0.02", "strand")]
                         + [(f"chrA\t10\t11\t+\t0\t0.9\t{bad}\t0.03\t0.02", r"malformed number \(prob1\)") for bad in _NOT_NUMBERS]
                         + [("chrA\t10\t1234567890123456789\t+\t0\t0.9\t0.05\t0.03\t0.02", r"malformed number \(end\)"),
                            ("chrA\t10\t11\t+\t-1234567890123456789\t0.9\t0.05\t0.03\t0.02", r"malformed number \(mut_type\)")])
@pytest.mark.parametrize("gz", [False, True])
def test_malformed_rows_raise_with_the_row(tmp_path, row, what, gz):
    """A field outside the reader's grammar is refused with its line and column, whatever float() would make of it.  The EMPTY
    probability field among them is what the writer emits for NaN (pandas' na_rep): a table with a NaN row is refused when it is read
    back.  That is today's contract and is pinned here as it stands."""
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


# ------------------------------------------------------------------------------------------------------------------
# the reader's numbers, bit for bit (parse_f64 / parse_int of csrc/tables.hip and the host patch of the slow fields)
# ------------------------------------------------------------------------------------------------------------------
def _takes_fast_path(text):
    """The rule of parse_f64: the digits of the mantissa without leading zeros are at most 19 and their integer is <= 2^53, and the
    power of ten that is left is within +-22 (a zero mantissa is always fast)."""
    mant, _, exp = text.lower().lstrip("+-").partition("e")
    whole, _, frac = mant.partition(".")
    digits = (whole + frac).lstrip("0")
    if not digits:
        return True
    exp10 = int(exp or 0) - len(frac)
    return len(digits) <= 19 and int(digits) <= 2 ** 53 and -22 <= exp10 <= 22


def _to_host(ptr, count, dtype):
    """`count` items of `dtype` at the device address `ptr` (a column of a chunk; the reader has synchronised its stream)."""
    out = np.empty(count, dtype)
    if count:
        copy = _lib.lib().hipMemcpy          # resolved through the library's own dependency on the HIP runtime
        copy.restype, copy.argtypes = C.c_int, [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int]
        assert copy(out.ctypes.data, ptr, out.nbytes, 2) == 0      # hipMemcpyDeviceToHost
    return out


def _read_columns(path, n_class, chunk_bytes=None):
    """Every column of the table as host arrays, chunk after chunk, and the number of chunks."""
    from mural_amd import tables
    cols = {"start": [], "end": [], "mut_type": [], "label": [], "strand": [], "prob": []}
    kinds = {"start": np.int64, "end": np.int64, "mut_type": np.int32, "label": np.float32, "strand": np.uint8, "prob": np.float64}
    chunks = 0
    with tables.TableReader(path, n_class, chunk_bytes or tables.DEFAULT_CHUNK_BYTES) as rd:
        for c in rd:
            chunks += 1
            n = int(c.n_rows)
            for key, dt in kinds.items():
                cols[key].append(_to_host(getattr(c, key), n * (n_class if key == "prob" else 1), dt))
    out = {key: np.concatenate(v) if v else np.zeros(0, kinds[key]) for key, v in cols.items()}
    out["prob"] = out["prob"].reshape(-1, n_class)
    return out, chunks


def _cells_table(tmp_path, cells, n_class=4, ints=None, name="cells.tsv"):
    """A table whose probability cells are `cells` row after row (the last row filled up with '0.25'); ints: per row (start, end,
    mut_type) texts, default the row number, the next one and 0."""
    cells = list(cells) + ["0.25"] * (-len(cells) % n_class)
    lines = ["\t".join(["chrom", "start", "end", "strand", "mut_type"] + ["prob%d" % c for c in range(n_class)])]
    for r in range(len(cells) // n_class):
        s, e, m = ints[r] if ints else (str(r), str(r + 1), "0")
        lines.append("\t".join(["chr%d" % (1 + r // 50 % 4), s, e, "+-"[r % 2], m] + cells[r * n_class:(r + 1) * n_class]))
    p = tmp_path / name
    p.write_text("".join(ln + "\n" for ln in lines))
    return str(p), cells


def _bits(a):
    return np.ascontiguousarray(a, np.float64).view(np.uint64)


def _assert_cells(got, cells, what):
    want = _bits([float(t) for t in cells])
    bad = np.nonzero(_bits(got).ravel() != want)[0]
    assert bad.size == 0, (what, [(int(i), cells[i], float(got.ravel()[i]).hex(), float(cells[i]).hex()) for i in bad[:5]])


_M53 = ["9007199254740992", "9007199254740993"]
_GRAMMAR_FAST = _M53[:1] + [_M53[0] + e for e in ("e22", "e-22")] + [
    "1e22", "1e-22", "1000e20", "12345678e-22", "0e999999999", "-0e5", "5.", ".5", "+.5e+1", "1E-5", "1e+05", "-0", "-0.0", "00012.50",
    "0." + "0" * 21 + "1", "0.5"]
_GRAMMAR_SLOW = _M53[1:] + [_M53[0] + e for e in ("e23", "e-23")] + [_M53[1] + e for e in ("e22", "e23", "e-22", "e-23")] + [
    "1234567890123456789", "9999999999999999999", "1.234567890123456789", "12345678901234567890", "99999999999999999999",
    "0.12345678901234567890", "123456789012345678e5",
    "0." + "0" * 25 + "12345", "0." + "0" * 25 + "9007199254740993", "-0." + "0" * 25 + "5",
    "0.5" + "0" * 20, "1e23", "1.5e-22", "1234.5678e-19", "0." + "0" * 22 + "1",
    "%.17g" % 1.7976931348623157e308, "%.17g" % 2.2250738585072014e-308, "%.17g" % 2.2250738585072009e-308, "%.17g" % 5e-324,
    "-%.17g" % 5e-324, "1e400", "-1e400", "1e-400", "-1e-400", "2.4703282292062327e-324", "2.4703282292062328e-324"]


@pytest.mark.parametrize("chunk_bytes", [None, 97, 4096], ids=["default", "97", "4096"])
def test_number_grammar_bit_for_bit(tmp_path, chunk_bytes):
    """Every cell's float64 bit pattern equals float(text)'s (-0 keeps its sign, 1e400 is inf, 1e-400 is 0): the borders of the exact
    fast path (mantissa 2^53 / 2^53 + 1, power of ten +-22 / +-23, 19 / 20 digits), zeros before the digits, the largest and smallest
    normal and subnormal and the half-way point below the smallest, and the forms of the grammar.  Slow and fast cells are mixed in a
    row; at 97 and 4096 bytes a chunk the slow fields lie in many chunks and in both text buffers.  Integers: 18 digits, signs, -0."""
    for t in _GRAMMAR_FAST:
        assert _takes_fast_path(t), t
    for t in _GRAMMAR_SLOW:
        assert not _takes_fast_path(t), t
    cells = [t for pair in zip(_GRAMMAR_SLOW, (_GRAMMAR_FAST * 3)[:len(_GRAMMAR_SLOW)]) for t in pair] * 6
    ints = [("123456789012345678", "-123456789012345678", "+7"), ("+7", "-7", "-0"), ("-0", "+0", "-7"), ("007", "999999999999999999", "12")]
    n_rows = -(-len(cells) // 4)
    ints = (ints * n_rows)[:n_rows]
    path, cells = _cells_table(tmp_path, cells, ints=ints)
    got, chunks = _read_columns(path, 4, chunk_bytes)
    assert chunks > (10 if chunk_bytes == 97 else 1 if chunk_bytes else 0)
    assert got["prob"].shape == (n_rows, 4)
    _assert_cells(got["prob"], cells, chunk_bytes)
    assert got["start"].tolist() == [int(s) for s, _, _ in ints]
    assert got["end"].tolist() == [int(e) for _, e, _ in ints]
    assert got["mut_type"].tolist() == [int(m) for _, _, m in ints]
    assert got["label"].tolist() == [float(int(m)) for _, _, m in ints]
    assert got["strand"].tolist() == [r % 2 for r in range(n_rows)]


def _format_chunks(path, n_class):
    """The rows of the table parsed and written again by the device formatter, chunk after chunk (tables._scale_file without the
    scaling)."""
    import torch
    from mural_amd import tables
    lib = _lib.lib()
    text = b""
    with tables.TableReader(path, n_class) as rd:
        count = torch.zeros(1, dtype=torch.int64, device=rd.device)
        for c in rd:
            n = int(c.n_rows)
            names = tables._name_table(rd.chrom_names(c.n_chroms))
            t = _lib.MuralTsvRows()
            t.chrom_names, t.n_chroms, t.name_stride = C.cast(names, C.c_char_p), max(c.n_chroms, 1), tables._NAME_STRIDE
            t.chrom_id, t.start, t.end, t.strand, t.label, t.prob = c.chrom_id, c.start, c.end, c.strand, c.label, c.prob
            t.prob_f64, t.n_class, t.prob_stride, t.perm, t.n, t.layout = 1, n_class, n_class, None, n, 0
            out = torch.empty(n * int(lib.mural_tsv_row_bound(C.byref(t))), dtype=torch.uint8, device=rd.device)
            ws = torch.empty(int(lib.mural_tsv_format_workspace_bytes(n)) + max(c.n_chroms, 1) * tables._NAME_STRIDE + 16,
                             dtype=torch.uint8, device=rd.device)
            _lib.check(lib.mural_tsv_format_device(C.byref(t), out.data_ptr(), out.numel(), count.data_ptr(), ws.data_ptr(), ws.numel(),
                                                  _lib.current_stream_ptr(rd.device)))
            text += out[:int(count.item())].cpu().numpy().tobytes()
    return text


def test_four_digit_text_round_trips_through_reader_and_formatter(tmp_path):
    """'%.4g' text of N x 10^(e10 - 3) -- all N = 1000 .. 9999 for e10 = -30 .. 4, every 37th N from a seeded offset in every other
    decade of the double range, signs alternating -- parses to float(text) bit for bit, and the device formatter writes the parsed
    column back as the same text.  The fast / slow border runs through the four digits: '1e-22' is fast and '1.5e-22' is slow."""
    rng = np.random.default_rng(37)
    cells = []
    for e10 in range(-323, 309):
        ns = range(1000, 10000) if -30 <= e10 <= 4 else range(1000 + int(rng.integers(0, 37)), 10000, 37)
        cells += ["%.4g" % v for v in (float("%s%de%d" % ("-" if n % 2 else "", n, e10 - 3)) for n in ns) if abs(v) < np.inf]
    fast = sum(map(_takes_fast_path, cells))
    assert len(cells) > 450_000 and 100_000 < fast < len(cells) - 100_000
    assert _takes_fast_path("1e-22") and not _takes_fast_path("1.5e-22") and "1e-22" in cells and "1.5e-22" in cells
    path, cells = _cells_table(tmp_path, cells)
    got, _ = _read_columns(path, 4)
    _assert_cells(got["prob"], cells, "parse")
    with open(path, "rb") as fh:
        body = fh.read().split(b"\n", 1)[1]
    again = _format_chunks(path, 4)
    if again != body:
        a, b = again.split(b"\n"), body.split(b"\n")
        assert len(a) == len(b)
        assert not [(x, y) for x, y in zip(a, b) if x != y][:5]


@pytest.mark.parametrize("chunk_bytes", [None, 97, 4096], ids=["default", "97", "4096"])
@pytest.mark.parametrize("every", [1, 2], ids=["all_slow", "alternating"])
def test_slow_fields_are_patched_into_their_own_cells(tmp_path, every, chunk_bytes):
    """The host patch of the fields outside the fast path: 1500 x 4 cells of which every one (or every second one) is a distinct
    '%.17g' value -- consecutive doubles, so a value patched into a neighbour's cell shows -- come back cell for cell.  With every cell
    slow the kernel lists rows x classes fields per chunk; alternating, fast '%.4g' cells sit between them."""
    n_rows, nc = 1500, 4
    base = np.float64(0.3).view(np.uint64)
    slow = ["%.17g" % v for v in (base + np.arange(2 * n_rows * nc, dtype=np.uint64)).view(np.float64)]
    slow = [t for t in slow if not _takes_fast_path(t)][:n_rows * nc]      # (a text that ends in zeros has 16 digits or fewer: fast)
    assert len(slow) == n_rows * nc == len(set(slow))
    fast = ["%.4g" % (0.001 + 0.0001 * (i % 9000)) for i in range(n_rows * nc)]
    assert all(map(_takes_fast_path, fast))
    cells = [s if i % every == 0 else f for i, (s, f) in enumerate(zip(slow, fast))]
    path, cells = _cells_table(tmp_path, cells, nc)
    got, chunks = _read_columns(path, nc, chunk_bytes)
    assert got["prob"].shape == (n_rows, nc) and (chunks > 1 or chunk_bytes is None)
    _assert_cells(got["prob"], cells, (every, chunk_bytes))
    assert got["start"].tolist() == list(range(n_rows))
