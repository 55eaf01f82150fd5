"""Prediction over genomic regions: the sites are enumerated on the device from the resident genome (csrc/sites.hip,
PackedGenome.enumerate_sites, predict_regions_sharded) instead of being read from a BED file with one row per site.  The
enumeration is checked against a plain-Python loop over the sequence, the prediction table byte for byte against the table the BED
path writes for a BED file of the same sites."""
import importlib.util
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

SELECTIONS = [("A", "all"), ("C", "all"), ("C", "CpG"), ("C", "nonCpG"), ("ANY", "all")]
TILE = 256 * 32                # bases per block of the enumeration kernels


def _plant(seq, at, text):
    seq[at:at + len(text)] = list(text)


def _record_main():
    """5003 bases (no multiple of 32) with the places where the enumeration can go wrong."""
    rng = np.random.default_rng(11)
    s = list(rng.choice(list("ACGT"), size=5003))
    _plant(s, 0, "GC")                       # a G first: a '-' site without a previous base (nonCpG)
    _plant(s, 31, "CG")                      # CpG pairs over the borders of a 32-base and a 64-base word
    _plant(s, 63, "CG")
    _plant(s, 95, "CGCG")
    _plant(s, 100, "N" * 40)                 # runs of N, one of them over a word border
    _plant(s, 158, "NNNN")
    _plant(s, 200, "ACNGT")                  # N as the neighbour of a C and of a G
    _plant(s, 300, "CRG")                    # IUPAC codes as neighbours ...
    _plant(s, 310, "CYG")
    _plant(s, 320, "ARTYA")                  # ... and where a site could be
    _plant(s, 350, "CGRCGYCG")
    s[1000:1100] = [c.lower() for c in s[1000:1100]]      # lower case
    _plant(s, 1040, "acgcgt")
    _plant(s, 2000, "N" * 200)               # no site of any kind
    _plant(s, 2300, "CG" * 100)              # no A/T site, CpG only
    _plant(s, 3000, "A" * 300)               # all A
    _plant(s, 3400, "T" * 70)
    _plant(s, 4990, "ACGTACGTACCGC")         # a C last: a '+' site without a next base (nonCpG)
    return "".join(s)


def _record_long():
    """70 001 bases: CpG pairs over the borders of the 8192-base tiles, a tile without any site, sites around every tile border."""
    rng = np.random.default_rng(12)
    s = list(rng.choice(list("ACGTN"), size=70_001, p=[.245, .245, .245, .245, .02]))
    for t in range(1, 8):
        _plant(s, t * TILE - 1, "CG")
    _plant(s, 3 * TILE - 3, "ATCGAT")
    _plant(s, 4 * TILE, "N" * TILE)          # tile 4: nothing
    _plant(s, 5 * TILE - 1, "NG")            # a G first in its tile behind an N
    _plant(s, 70_000, "T")
    return "".join(s)


def py_sites(seq, lo, hi, focal, context="all"):
    """The specification, base by base: [(position, strand)] of the window [lo, hi) clamped to the record."""
    s = seq.upper()
    n = len(s)
    out = []
    for p in range(max(lo, 0), min(hi, n)):
        b = s[p]
        if focal == "ANY":
            if b in "ACGT":
                out.append((p, 0))
        elif focal == "A":
            if b in "AT":
                out.append((p, 0 if b == "A" else 1))
        elif b in "CG":
            cpg = (p + 1 < n and s[p + 1] == "G") if b == "C" else (p > 0 and s[p - 1] == "C")
            if context == "all" or (context == "CpG") == cpg:
                out.append((p, 0 if b == "C" else 1))
    return out


MAIN, LONG = _record_main(), _record_long()
SECOND = "".join(np.random.default_rng(13).choice(list("ACGT"), size=1203))
RECORDS = {"chrA": MAIN, "chr10": SECOND, "chrFew": "CCGCCACCGGTCCCGG", "chrNone": "NNNNCCGGNN" * 3}      # (file order; chr10 < chrA by name)


def _windows(n):
    return [(0, n), (0, 1), (n - 1, n), (700, 700), (45, 1999), (33, 63), (n - 600, n + 500), (-7, 40), (n + 10, n + 20)]


@pytest.fixture(scope="module")
def genomes():
    from mural_amd.data import PackedGenome
    return {"main": (MAIN, PackedGenome.from_sequence(MAIN, "cuda")), "long": (LONG, PackedGenome.from_sequence(LONG, "cuda"))}


def _got(g, lo, hi, focal, context, **kw):
    pos, strand = g.enumerate_sites(lo, hi, focal, context, **kw)
    assert pos.dtype == torch.int64 and strand.dtype == torch.uint8 and pos.is_cuda and strand.is_cuda
    return list(zip(pos.cpu().tolist(), strand.cpu().tolist()))


# ---- 1. enumeration against plain Python -----------------------------------------------------------------------------------------
@pytest.mark.parametrize("focal,context", SELECTIONS)
def test_enumeration_equals_a_python_loop(genomes, focal, context):
    seq, g = genomes["main"]
    assert MAIN[0] == "G" and MAIN[-1] == "C" and len(MAIN) % 32 and MAIN[31:33] == "CG" and MAIN[63:65] == "CG"
    for lo, hi in _windows(len(seq)):
        want = py_sites(seq, lo, hi, focal, context)
        assert _got(g, lo, hi, focal, context) == want, (lo, hi)
        assert g.count_sites(lo, hi, focal, context) == len(want)
        assert _got(g, lo, hi, focal, context) == want               # a second run: the same, bit for bit
    whole = py_sites(seq, 0, len(seq), focal, context)
    if focal == "ANY" or context == "nonCpG":              # sites at the first and at the last position: a G, a C, no CpG
        assert whole[0] == (0, int(focal == "C")) and whole[-1] == (len(seq) - 1, 0)
    n = len(whole)
    for first, m in [(0, 10), (5, 1), (100, 777), (n - 3, None), (n - 3, 50), (n, None), (n + 5, 4), (17, 0)]:
        assert _got(g, 0, len(seq), focal, context, first=first, n=m) == whole[first:][:m], (first, m)


@pytest.mark.parametrize("focal,context", SELECTIONS)
def test_enumeration_over_tile_borders(genomes, focal, context):
    seq, g = genomes["long"]
    whole = py_sites(seq, 0, len(seq), focal, context)
    assert _got(g, 0, len(seq), focal, context) == whole
    for lo, hi in [(TILE - 1, TILE + 1), (TILE, 2 * TILE), (3 * TILE - 5, 3 * TILE + 5), (4 * TILE - 2, 5 * TILE + 2), (12_345, 54_321)]:
        assert _got(g, lo, hi, focal, context) == py_sites(seq, lo, hi, focal, context), (lo, hi)
    # slices that start and end in the middle of a tile, and one inside the window of a mid-tile start
    n = len(whole)
    for first, m in [(1, 5), (n // 3, n // 3), (n // 2 + 11, 4000), (n - 1, None)]:
        assert _got(g, 0, len(seq), focal, context, first=first, n=m) == whole[first:][:m], (first, m)
    sub = py_sites(seq, 9000, 60_000, focal, context)
    assert _got(g, 9000, 60_000, focal, context, first=len(sub) // 2, n=3000) == sub[len(sub) // 2:][:3000]
    a, b = g.enumerate_sites(0, len(seq), focal, context), g.enumerate_sites(0, len(seq), focal, context)
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])


# ---- 2. CpG partition --------------------------------------------------------------------------------------------------------------
def test_cpg_and_noncpg_partition_the_c_sites(genomes):
    for key in ("main", "long"):
        seq, g = genomes[key]
        for lo, hi in _windows(len(seq)) + [(31, 32), (32, 33), (TILE - 1, TILE), (TILE, TILE + 1)]:
            every, cpg, non = (_got(g, lo, hi, "C", c) for c in ("all", "CpG", "nonCpG"))
            assert not set(cpg) & set(non) and sorted(cpg + non) == every, (key, lo, hi)
    seq, g = genomes["main"]
    assert _got(g, 0, 1, "C", "nonCpG") == [(0, 1)] and _got(g, len(seq) - 1, len(seq), "C", "nonCpG") == [(len(seq) - 1, 0)]


def test_selection_errors(genomes):
    _, g = genomes["main"]
    for focal, context in [("A", "CpG"), ("ANY", "nonCpG"), ("G", "all"), ("C", "islands")]:
        with pytest.raises(ValueError):
            g.enumerate_sites(0, 10, focal, context)


# ---- files and models of the table tests -----------------------------------------------------------------------------------------
R_LOCAL, R_DISTAL = 5, 250


@pytest.fixture(scope="module")
def files(tmp_path_factory):
    d = tmp_path_factory.mktemp("regions")
    fa = d / "g.fa"
    fa.write_text("".join(f">{k}\n" + "\n".join(s[i:i + 60] for i in range(0, len(s), 60)) + "\n" for k, s in RECORDS.items()))
    return d, str(fa)


@pytest.fixture(scope="module")
def snv_model():
    from mural_amd.model import model_choice, weights_init
    ncol = 2 * R_LOCAL + 1 - 2
    config = dict(local_radius=R_LOCAL, local_order=3, local_hidden1_size=150, local_hidden2_size=75, distal_radius=R_DISTAL,
                  emb_dropout=0.1, local_dropout=0.1, CNN_kernel_size=3, CNN_out_channels=32, distal_fc_dropout=0.25, n_class=4,
                  model_no=2, seq_only=True, emb_dims=[(65, 2)] * ncol, segment_center=300000)
    common = dict(emb_dims=config["emb_dims"], n_cont=0, n_class=4, distal_order=1, in_channels=4)
    torch.manual_seed(5)
    model = model_choice(2, config, common, "snv")
    model.apply(weights_init)
    return model.cuda().eval(), config


def _write_bed(path, rows):
    with open(path, "w") as fh:
        fh.write("".join(f"{c}\t{p}\t{p + 1}\t.\t0\t{'-' if st else '+'}\n" for c, p, st in rows))
    return str(path)


def _bed_rows(regions, focal, context):
    """[(chrom, pos, strand)] of {chrom: [(lo, hi)]} by the Python enumeration, in the FASTA's record order."""
    return [(c, p, st) for c in RECORDS for lo, hi in regions.get(c, []) for p, st in py_sites(RECORDS[c], lo, hi, focal, context)]


def _forward(snv_model, fa, **kw):
    from mural_amd.predict import HipShardForward
    return HipShardForward(snv_model[0], fa, local_radius=R_LOCAL, local_order=3, **kw)


def _region_table(snv_model, fa, out, regions, focal, context="all", fwd_kw=None, **kw):
    from mural_amd.predict import TsvSink, predict_regions_sharded
    fwd = _forward(snv_model, fa, **(fwd_kw or {}))
    n = predict_regions_sharded(fwd, regions, focal, context, sink=TsvSink(out), collect=False, **kw)
    return n, fwd, open(out, "rb").read()


WHOLE = {c: [(0, len(s))] for c, s in RECORDS.items()}


# ---- 3. table parity against the BED path -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("focal,context,fwd_kw", [
    ("A", "all", dict(reuse=True)), ("A", "all", dict(reuse=False)), ("C", "CpG", dict(reuse=True)), ("C", "CpG", dict(reuse=False)),
    ("A", "all", dict(reuse=True, poisson=True)), ("C", "nonCpG", dict(reuse=False, poisson=True))])
def test_region_table_is_the_bed_path_s_table(files, snv_model, focal, context, fwd_kw):
    from mural_amd.predict import TsvSink, predict_bed_sharded
    d, fa = files
    rows = _bed_rows(WHOLE, focal, context)
    n, fwd, got = _region_table(snv_model, fa, d / "r.tsv", list(RECORDS), focal, context, fwd_kw)
    assert n == len(rows)
    if fwd_kw["reuse"] and focal == "A":
        assert fwd.reuse_sites > 0                         # the dense path really is taken
    bed = _write_bed(d / "s.bed", rows)
    m = predict_bed_sharded(_forward(snv_model, fa, **fwd_kw), bed, sink=TsvSink(d / "b.tsv"), collect=False)
    want = open(d / "b.tsv", "rb").read()
    assert m == len(rows) and want.count(b"\n") == len(rows) + 1
    assert got == want
    chroms = [ln.split(b"\t")[0] for ln in got.split(b"\n")[1:-1]]
    assert chroms == sorted(chroms) and chroms[0] == b"chr10"      # ascending names, not the FASTA's order


def test_aligned_region_route_fills_its_timings_keys(files, snv_model):
    """The `timings` keys of the aligned route (tools/bench_regions.py reads them), as recorded by running the commit BEFORE the drivers
    shared one loop on this input."""
    d, fa = files
    T = {}
    n, _, _ = _region_table(snv_model, fa, d / "t.tsv", {"chrA": [(40, 90), (3290, 3410)], "chr10": [(0, 100)]}, "A", timings=T)
    print(sorted(T))
    assert n > 0 and set(T) == {"emulation", "enumerate", "compute_enqueue", "gather", "sink", "focal_wait", "aligned_shards", "sink_close"}
    assert T["aligned_shards"] == 2


def test_collected_rows_are_the_table_s_rows(files, snv_model):
    """collect=True (and a sink that gets the gathered shard): the same table, and the rows back in its order."""
    from mural_amd.predict import TsvSink, predict_regions_sharded, write_predictions
    d, fa = files
    regions = {"chrA": [(40, 90), (3290, 3410)], "chr10": [(0, 100)]}
    rows = sorted(_bed_rows(regions, "A", "all"))
    res = predict_regions_sharded(_forward(snv_model, fa), regions, "A", sink=TsvSink(d / "c.tsv"))
    assert [(c, int(p), int(s == "-")) for c, p, s in zip(res["chrom"], res["start"], res["strand"])] == rows
    assert np.array_equal(res["end"], res["start"] + 1) and not res["label"].any() and np.array_equal(res["order"], np.arange(len(rows)))
    assert np.allclose(res["prob"].sum(axis=1), 1.0, atol=1e-5)
    write_predictions(res, d / "w.tsv")
    assert open(d / "c.tsv", "rb").read() == open(d / "w.tsv", "rb").read()
    assert _region_table(snv_model, fa, d / "a.tsv", regions, "A")[2] == open(d / "c.tsv", "rb").read()


# ---- 4. INDEL ------------------------------------------------------------------------------------------------------------------------
def test_indel_region_table_is_the_bed_path_s_table(files):
    from mural_amd.predict import HipShardForward, TsvSink, predict_bed_sharded, predict_regions_sharded
    from tests import _util as U
    from tests.test_gpu_indel import product_from
    d, fa = files
    fx = U.load("indel_synth_small.npz")
    model = product_from(fx)
    model.load_state_dict(U.indel_state_for(fx, U.indel_oracle_from_hp(fx["hp"], fx["down"])))
    model = model.cuda().eval()
    R = int(fx["hp"][0])
    regions = {"chrA": [(60, 420)]}                       # N runs and IUPAC codes inside
    rows = _bed_rows(regions, "ANY", "all")
    assert 200 < len(rows) < 360
    make = lambda: HipShardForward(model, fa, local_radius=R_LOCAL, local_order=3, distal_radius=R, model_type="indel")      # noqa: E731
    n = predict_regions_sharded(make(), "chrA:61-420", "ANY", model_type="indel", sink=TsvSink(d / "ir.tsv"), collect=False)
    bed = _write_bed(d / "i.bed", rows)
    predict_bed_sharded(make(), bed, model_type="indel", sink=TsvSink(d / "ib.tsv"), collect=False)
    got = open(d / "ir.tsv", "rb").read()
    assert n == len(rows) and got.count(b"\n") == len(rows) + 1 and got == open(d / "ib.tsv", "rb").read()


# ---- 5. regions ----------------------------------------------------------------------------------------------------------------------
def _starts(table):
    return [(f[0].decode(), int(f[1]), f[3].decode()) for f in (ln.split(b"\t") for ln in table.split(b"\n")[1:-1])]


def test_regions_are_merged_parsed_and_honoured(files, snv_model):
    d, fa = files
    union = _region_table(snv_model, fa, d / "u.tsv", "chrA:1-2500", "A")[2]
    assert _region_table(snv_model, fa, d / "m.tsv", ["chrA:1-1000", "chrA:500-2000", "chrA:2001-2500"], "A")[2] == union
    assert _starts(union) == [("chrA", p, "-" if st else "+") for p, st in py_sites(MAIN, 0, 2500, "A")]
    # chr:start-end (1-based, inclusive), a BED-style interval in a file, and the interval itself select the same sites
    reg = d / "regions.bed"
    reg.write_text("chrA\t3050\t3100\tstretch\nchr10\t7\t300\n")
    by_file = _region_table(snv_model, fa, d / "f.tsv", str(reg), "A")[2]
    assert _region_table(snv_model, fa, d / "s.tsv", ["chr10:8-300", "chrA:3051-3100"], "A")[2] == by_file
    assert _region_table(snv_model, fa, d / "i.tsv", {"chrA": [(3050, 3100)], "chr10": [(7, 300)]}, "A")[2] == by_file
    # inside the all-A stretch: the A just before and the A just behind the region are sites of the record, not of the region
    assert MAIN[3049] == "A" and MAIN[3100] == "A"
    got = _starts(by_file)
    assert [r for r in got if r[0] == "chrA"] == [("chrA", p, "+") for p in range(3050, 3100)]
    assert [r for r in got if r[0] == "chr10"] == [("chr10", p, "-" if st else "+") for p, st in py_sites(SECOND, 7, 300, "A")]
    # a site at the region's edge is CpG by the base OUTSIDE the region: the C of the CG at 31/32 alone, and its G alone
    assert _starts(_region_table(snv_model, fa, d / "e1.tsv", "chrA:32-32", "C", "CpG")[2]) == [("chrA", 31, "+")]
    assert _starts(_region_table(snv_model, fa, d / "e2.tsv", "chrA:33-33", "C", "CpG")[2]) == [("chrA", 32, "-")]
    assert _starts(_region_table(snv_model, fa, d / "e3.tsv", ["chrA:32-32", "chrA:33-33"], "C", "nonCpG")[2]) == []


# ---- 6. ranks --------------------------------------------------------------------------------------------------------------------------
def test_emulated_ranks_write_the_slices_of_the_table(files, snv_model):
    """Rank i of 3 takes shard_bounds(sites of the chromosome, i, 3) of every chromosome's enumeration; chrFew has two A/T sites (one
    rank without a row), chrNone none."""
    from mural_amd.predict import TsvSink, predict_regions_sharded, shard_bounds
    d, fa = files
    regions = ["chrA:1-700", "chrA:2950-3500", "chr10", "chrFew", "chrNone"]
    assert len(py_sites(RECORDS["chrFew"], 0, 99, "A")) == 2 and not py_sites(RECORDS["chrNone"], 0, 99, "A")
    n, _, table = _region_table(snv_model, fa, d / "w1.tsv", regions, "A")
    body = table.split(b"\n")[1:-1]
    assert n == len(body) > 0
    by_chrom = {}
    for ln in body:
        by_chrom.setdefault(ln.split(b"\t")[0], []).append(ln)
    assert sorted(by_chrom) == [b"chr10", b"chrA", b"chrFew"]
    parts = []
    for i in range(3):
        out = d / "w3.tsv"
        predict_regions_sharded(_forward(snv_model, fa), regions, "A", sink=TsvSink(out, parts=(i, 3)), collect=False, emulate=(i, 3))
        parts.append(open(str(out) + ".part%04d" % i, "rb").read().split(b"\n")[:-1])
        want = []
        for c in sorted(by_chrom):
            lo, hi = shard_bounds(len(by_chrom[c]), i, 3)
            want += by_chrom[c][lo:hi]
        assert parts[i] == want, i
    # the parts' rows in rank order, strung together chromosome by chromosome as the part-file sink does it: the world-1 body
    assert sorted((ln for p in parts for ln in p), key=lambda ln: ln.split(b"\t")[0]) == body
    with pytest.raises(ValueError, match="emulate"):
        predict_regions_sharded(_forward(snv_model, fa), regions, "A", emulate=(1, 3))


# ---- 7. command line -------------------------------------------------------------------------------------------------------------------
def test_command_line_writes_the_api_s_table(files, snv_model):
    from mural_amd.model import nn_utils
    d, fa = files
    ckpt = str(d / "model")
    nn_utils.save_model(snv_model[0], None, snv_model[1], ckpt)
    spec = importlib.util.spec_from_file_location("predict_files", os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))),
                                                                                  "tools", "predict_files.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    mod.main([ckpt, fa, str(d / "cli.tsv"), "--regions", "chrA:1-3000", "--focal", "A"])
    n, _, want = _region_table(snv_model, fa, d / "api.tsv", "chrA:1-3000", "A")
    assert n == len(py_sites(MAIN, 0, 3000, "A")) and open(d / "cli.tsv", "rb").read() == want
    mod.main([ckpt, fa, "--regions=chrA:1-3000", "--regions", "chr10", str(d / "cli2.tsv"), "--focal", "C", "--context", "nonCpG"])
    assert open(d / "cli2.tsv", "rb").read() == _region_table(snv_model, fa, d / "api2.tsv", ["chr10", "chrA:1-3000"], "C", "nonCpG")[2]


# ---- 8. errors ---------------------------------------------------------------------------------------------------------------------------
def test_region_driver_errors(files, snv_model):
    from mural_amd.predict import TsvSink, predict_bed_sharded, predict_regions_sharded
    d, fa = files
    with pytest.raises(KeyError) as by_region:
        predict_regions_sharded(_forward(snv_model, fa), ["chr10", "chrZ:1-50"], "A", sink=TsvSink(d / "k.tsv"), collect=False)
    assert not (d / "k.tsv").exists()
    bed = _write_bed(d / "z.bed", [("chrZ", 5, 0)])
    with pytest.raises(KeyError) as by_bed:
        predict_bed_sharded(_forward(snv_model, fa), bed, collect=False)
    assert by_region.value.args == by_bed.value.args == ("chrZ",)
    for focal, context, model_type in [("A", "CpG", "snv"), ("ANY", "nonCpG", "indel"), ("ANY", "all", "snv"), ("A", "all", "indel"),
                                       ("C", "all", "indel")]:
        with pytest.raises(ValueError):
            predict_regions_sharded(_forward(snv_model, fa), "chr10", focal, context, model_type=model_type)
