"""One regions run with one model per site class (mural_amd.predict.ModelSetForward, focal "SET"): the device kernels that classify,
split and re-interleave the rows (csrc/sites.hip: mural_sites_classify, mural_rows_split, mural_rows_scatter, the union enumeration)
against plain Python / numpy, and the table byte for byte against the three single-model tables' rows interleaved by start.  The
records and the tiny Network2 are those of tests/test_gpu_regions.py; the three members are built under three seeds, so a row that
went to the wrong model shows."""
import importlib.util
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

TILE = 256 * 32                # bases per block of the enumeration kernels
CLASSES = ("A", "nonCpG", "CpG")
SINGLE = {"A": ("A", "all"), "nonCpG": ("C", "nonCpG"), "CpG": ("C", "CpG")}
BIT = {"A": 1, "nonCpG": 2, "CpG": 4}


def _plant(seq, at, text):
    seq[at:at + len(text)] = list(text)


def _record_main():
    """5003 bases (no multiple of 32) with the places where the enumeration can go wrong."""
    rng = np.random.default_rng(11)
    s = list(rng.choice(list("ACGT"), size=5003))
    _plant(s, 0, "GC")
    _plant(s, 31, "CG")
    _plant(s, 63, "CG")
    _plant(s, 95, "CGCG")
    _plant(s, 100, "N" * 40)
    _plant(s, 158, "NNNN")
    _plant(s, 200, "ACNGT")
    _plant(s, 300, "CRG")
    _plant(s, 310, "CYG")
    _plant(s, 320, "ARTYA")
    _plant(s, 350, "CGRCGYCG")
    s[1000:1100] = [c.lower() for c in s[1000:1100]]
    _plant(s, 1040, "acgcgt")
    _plant(s, 2000, "N" * 200)
    _plant(s, 2300, "CG" * 100)
    _plant(s, 3000, "A" * 300)
    _plant(s, 3400, "T" * 70)
    _plant(s, 4990, "ACGTACGTACCGC")
    return "".join(s)


def _record_long():
    """70 001 bases: CpG pairs over the borders of the 8192-base tiles, a tile without any site, sites around every tile border."""
    rng = np.random.default_rng(12)
    s = list(rng.choice(list("ACGTN"), size=70_001, p=[.245, .245, .245, .245, .02]))
    for t in range(1, 8):
        _plant(s, t * TILE - 1, "CG")
    _plant(s, 3 * TILE - 3, "ATCGAT")
    _plant(s, 4 * TILE, "N" * TILE)
    _plant(s, 5 * TILE - 1, "NG")
    _plant(s, 70_000, "T")
    return "".join(s)


def _record_crafted():
    """8192 + 45 bases for the classifier: CG over the packed2 word border (15/16), the nmask word border (31/32) and the tile border
    (8191/8192), masked and ambiguous neighbours, a G first and a C last, lower case."""
    rng = np.random.default_rng(14)
    s = list(rng.choice(list("ACGT"), size=TILE + 45))
    _plant(s, 0, "GCA")
    _plant(s, 15, "CG")
    _plant(s, 31, "CG")
    _plant(s, 46, "AGCA")                    # the same borders the other way round: no CpG
    _plant(s, 62, "AGCA")
    _plant(s, 70, "ACNAT")                   # CN
    _plant(s, 80, "ANGAT")                   # NG
    _plant(s, 90, "ACRGA")                   # CR, RG
    _plant(s, 127, "CN")                     # a masked neighbour across a word border
    _plant(s, 159, "NG")
    _plant(s, 200, "acgcgtcatg")             # lower case
    _plant(s, TILE - 1, "CG")
    _plant(s, TILE + 30, "TTCGACCGTAACGGC")  # .. and a C last
    return "".join(s)


def py_sites(seq, lo, hi, focal, context="all"):
    """The specification, base by base: [(position, strand)] of the window [lo, hi) clamped to the record."""
    s = seq.upper()
    n = len(s)
    out = []
    for p in range(max(lo, 0), min(hi, n)):
        b = s[p]
        if focal == "A":
            if b in "AT":
                out.append((p, 0 if b == "A" else 1))
        elif b in "CG":
            cpg = (p + 1 < n and s[p + 1] == "G") if b == "C" else (p > 0 and s[p - 1] == "C")
            if context == "all" or (context == "CpG") == cpg:
                out.append((p, 0 if b == "C" else 1))
    return out


def py_class(s, p, st):
    """The specification of classify_sites for one row of the upper-case record `s`."""
    n = len(s)
    if p < 0 or p >= n:
        return 255
    b = s[p]
    if st == 0 and b == "A" or st == 1 and b == "T":
        return 0
    if st == 0 and b == "C":
        return 2 if p + 1 < n and s[p + 1] == "G" else 1
    if st == 1 and b == "G":
        return 2 if p > 0 and s[p - 1] == "C" else 1
    return 255


MAIN, LONG, CRAFTED = _record_main(), _record_long(), _record_crafted()
SECOND = "".join(np.random.default_rng(13).choice(list("ACGT"), size=1203))
RECORDS = {"chrA": MAIN, "chr10": SECOND, "chrFew": "CCGCCACCGGTCCCGG", "chrNone": "NNNNCCGGNN" * 3}      # (file order; chr10 < chrA by name)


def _windows(n):
    return [(0, n), (0, 1), (n - 1, n), (700, 700), (45, 1999), (33, 63), (n - 600, n + 500), (-7, 40), (n + 10, n + 20)]


@pytest.fixture(scope="module")
def genomes():
    from mural_amd.data import PackedGenome
    return {"main": (MAIN, PackedGenome.from_sequence(MAIN, "cuda")), "long": (LONG, PackedGenome.from_sequence(LONG, "cuda")),
            "crafted": (CRAFTED, PackedGenome.from_sequence(CRAFTED, "cuda"))}


def _pairs(ps):
    return list(zip(ps[0].cpu().tolist(), ps[1].cpu().tolist()))


# ---- 1. classify ---------------------------------------------------------------------------------------------------------------------
def test_classify_equals_a_python_loop(genomes):
    seq, g = genomes["crafted"]
    s, n = seq.upper(), len(seq)
    assert s[0] == "G" and s[-1] == "C" and s[15:17] == s[31:33] == s[TILE - 1:TILE + 1] == "CG" and s[71:73] == "CN" and s[81:83] == "NG"
    assert s[91:93] == "CR" and seq[200:210].islower()
    pos = np.r_[np.repeat(np.arange(-1, n + 1), 2), [5, 5, n // 2]].astype(np.int64)
    strand = np.r_[np.tile([0, 1], n + 2), [2, 255, 7]].astype(np.uint8)
    want = np.array([py_class(s, int(p), int(st)) for p, st in zip(pos, strand)], np.uint8)
    assert (want[:2] == 255).all() and (want[-5:] == 255).all() and set(want.tolist()) == {0, 1, 2, 255}
    got = g.classify_sites(torch.from_numpy(pos).cuda(), torch.from_numpy(strand).cuda())
    assert got.dtype == torch.uint8 and got.is_cuda
    bad = np.nonzero(got.cpu().numpy() != want)[0]
    assert not len(bad), (pos[bad[:5]], strand[bad[:5]], got.cpu().numpy()[bad[:5]], want[bad[:5]])
    # the CpG pairs over the three borders, and their reverse
    by = {(int(p), int(st)): int(c) for p, st, c in zip(pos, strand, got.cpu().numpy())}
    for at in (15, 31, TILE - 1):
        assert by[(at, 0)] == 2 and by[(at + 1, 1)] == 2 and by[(at, 1)] == 255
    assert by[(47, 1)] == 1 and by[(48, 0)] == 1 and by[(63, 1)] == 1 and by[(64, 0)] == 1 and by[(0, 1)] == 1 and by[(n - 1, 0)] == 1 and by[(71, 0)] == 1 and by[(82, 1)] == 1
    assert g.classify_sites(np.zeros(0, np.int64), np.zeros(0, np.uint8)).shape == (0,)
    # every other record of this file as well
    for key in ("main", "long"):
        seq, g = genomes[key]
        s = seq.upper()
        pos = np.repeat(np.arange(len(s)), 2).astype(np.int64)
        strand = np.tile([0, 1], len(s)).astype(np.uint8)
        want = np.array([py_class(s, int(p), int(st)) for p, st in zip(pos, strand)], np.uint8)
        assert np.array_equal(g.classify_sites(pos, strand).cpu().numpy(), want), key


# ---- 2. union enumeration --------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def single_sites(genomes):
    """{(record, lo, hi): {class: [(pos, strand)]}} by the single-class enumerations, once for all masks."""
    out = {}
    for key, extra in (("main", []), ("long", [(TILE - 1, TILE + 1), (TILE, 2 * TILE), (3 * TILE - 5, 3 * TILE + 5), (4 * TILE - 2, 5 * TILE + 2),
                                               (12_345, 54_321), (9000, 60_000)])):
        seq, g = genomes[key]
        for lo, hi in _windows(len(seq)) + extra:
            out[(key, lo, hi)] = {c: _pairs(g.enumerate_sites(lo, hi, *SINGLE[c])) for c in CLASSES}
    return out


@pytest.mark.parametrize("mask", range(1, 8))
def test_union_enumeration_is_the_merge_of_the_classes(genomes, single_sites, mask):
    names = tuple(c for c in CLASSES if BIT[c] & mask)
    allowed = {CLASSES.index(c) for c in names}
    for (key, lo, hi), per_class in single_sites.items():
        seq, g = genomes[key]
        want = sorted(ps for c in names for ps in per_class[c])
        pos, strand = g.enumerate_sites(lo, hi, "SET", classes=mask)
        assert pos.dtype == torch.int64 and strand.dtype == torch.uint8
        assert _pairs((pos, strand)) == want, (key, lo, hi)
        assert g.count_sites(lo, hi, "SET", classes=names) == len(want)
        assert set(g.classify_sites(pos, strand).cpu().tolist()) <= allowed
        if mask == 7:
            assert pos.cpu().tolist() == g.enumerate_sites(lo, hi, "ANY")[0].cpu().tolist()
        if (lo, hi) in ((0, len(seq)), (9000, 60_000)):      # slices that start and end in the middle of a tile
            n = len(want)
            for first, m in [(0, 10), (5, 1), (1, 5), (n // 3, n // 3), (n // 2 + 11, 4000), (n - 3, None), (n - 3, 50), (n, None), (n + 5, 4), (17, 0)]:
                assert _pairs(g.enumerate_sites(lo, hi, "SET", first=first, n=m, classes=mask)) == want[first:][:m], (key, first, m)
    seq, g = genomes["long"]
    a, b = g.enumerate_sites(0, len(seq), "SET", classes=mask), g.enumerate_sites(0, len(seq), "SET", classes=mask)
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])
    if mask == 6:
        assert _pairs(a) == _pairs(g.enumerate_sites(0, len(seq), "C")) == _pairs(g.enumerate_sites(0, len(seq), "SET", classes="C"))


# ---- 3. split --------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [0, 1, 255, 256, 257, 70_001])
def test_split_is_the_stable_argsort(n):
    from mural_amd.data import split_rows
    rng = np.random.default_rng(n)
    columns = {"mixed": rng.choice(np.array([0, 1, 2, 255], np.uint8), size=n, p=[.4, .3, .2, .1]),
               "no class 1": rng.choice(np.array([0, 2, 255, 9], np.uint8), size=n),
               "all class 2": np.full(n, 2, np.uint8), "all 255": np.full(n, 255, np.uint8),
               "runs": np.repeat(np.array([2, 0, 1, 0], np.uint8), (n + 3) // 4)[:n]}
    for name, cls in columns.items():
        key = np.where(cls < 3, cls, 3)
        order = np.argsort(key, kind="stable")
        want_counts = np.bincount(key, minlength=4)
        kept = n - int(want_counts[3])
        dev = torch.from_numpy(cls).cuda()
        perm, counts = split_rows(dev, 3)
        assert perm.dtype == torch.int64 and perm.shape == (n,) and counts.shape == (4,)
        assert counts.cpu().tolist() == want_counts.tolist(), name
        assert np.array_equal(perm[:kept].cpu().numpy(), order[:kept]), name
        again = split_rows(dev, 3)
        assert torch.equal(again[0][:kept], perm[:kept]) and torch.equal(again[1], counts)
    # another number of classes: 2 (class 2 is left out with the 255s) and 1
    cls = columns["mixed"]
    for k in (1, 2):
        key = np.where(cls < k, cls, k)
        perm, counts = split_rows(torch.from_numpy(cls).cuda(), k)
        kept = int((key < k).sum())
        assert counts.cpu().tolist() == np.bincount(key, minlength=k + 1).tolist()
        assert np.array_equal(perm[:kept].cpu().numpy(), np.argsort(key, kind="stable")[:kept])
    with pytest.raises(ValueError):
        split_rows(torch.zeros(4, dtype=torch.uint8, device="cuda"), 9)


# ---- 4. scatter ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", [torch.float32, torch.float64])
def test_scatter_puts_rows_where_perm_says(dtype):
    from mural_amd.data import scatter_rows
    rng = np.random.default_rng(3)
    for m, rows in [(0, 7), (1, 1), (257, 257), (1000, 1500), (70_001, 70_001)]:
        perm = torch.from_numpy(rng.permutation(rows)[:m].astype(np.int64)).cuda()
        src = torch.from_numpy(rng.standard_normal((m, 5))).to(dtype).cuda()
        dst = torch.full((rows, 5), -1.0, dtype=dtype, device="cuda")
        want = dst.clone()
        want[perm] = src
        assert scatter_rows(src, perm, dst) is dst and torch.equal(dst, want), (m, rows)
    with pytest.raises(ValueError):
        scatter_rows(torch.zeros(3, 5, device="cuda"), torch.zeros(3, dtype=torch.int64, device="cuda"), torch.zeros(3, 5, dtype=torch.float64, device="cuda"))


# ---- files and models of the table tests -------------------------------------------------------------------------------------------------
R_LOCAL, R_DISTAL = 5, 250


@pytest.fixture(scope="module")
def files(tmp_path_factory):
    d = tmp_path_factory.mktemp("model_set")
    fa = d / "g.fa"
    fa.write_text("".join(f">{k}\n" + "\n".join(s[i:i + 60] for i in range(0, len(s), 60)) + "\n" for k, s in RECORDS.items()))
    return d, str(fa)


@pytest.fixture(scope="module")
def models():
    """{class: (tiny Network2, config)}: one architecture under three seeds."""
    from mural_amd.model import model_choice, weights_init
    ncol = 2 * R_LOCAL + 1 - 2
    out = {}
    for seed, name in zip((5, 6, 7), CLASSES):
        config = dict(local_radius=R_LOCAL, local_order=3, local_hidden1_size=150, local_hidden2_size=75, distal_radius=R_DISTAL,
                      emb_dropout=0.1, local_dropout=0.1, CNN_kernel_size=3, CNN_out_channels=32, distal_fc_dropout=0.25, n_class=4,
                      model_no=2, seq_only=True, emb_dims=[(65, 2)] * ncol, segment_center=300000)
        common = dict(emb_dims=config["emb_dims"], n_cont=0, n_class=4, distal_order=1, in_channels=4)
        torch.manual_seed(seed)
        model = model_choice(2, config, common, "snv")
        model.apply(weights_init)
        out[name] = (model.cuda().eval(), config)
    return out


# regions over the records: all three classes, chrFew with two sites (an A and a non-CpG C), chrNone with none; chrA's A/T and non-CpG
# sites are enough (1024 and 0.1 per base) for the members' cross-position reuse path
REGIONS = {"chrA": [(0, 2400), (2950, 5003)], "chr10": [(0, 1203)], "chrFew": [(5, 7)], "chrNone": [(0, 4)]}
_SINGLE_TABLES = {}


def _member(models, name, fa=None, **kw):
    from mural_amd.predict import HipShardForward
    return HipShardForward(models[name][0], fa, local_radius=R_LOCAL, local_order=3, **kw)


def _single_table(models, files, name, tag, fwd_kw, **run_kw):
    """The single-model table of class `name` over REGIONS (computed once per `tag`), and the run's timings."""
    from mural_amd.predict import TsvSink, predict_regions_sharded
    if (name, tag) not in _SINGLE_TABLES:
        d, fa = files
        out, T = d / f"single_{name}_{tag}.tsv", {}
        predict_regions_sharded(_member(models, name, fa, **fwd_kw), REGIONS, *SINGLE[name], sink=TsvSink(out), collect=False, timings=T, **run_kw)
        _SINGLE_TABLES[(name, tag)] = (open(out, "rb").read(), T)
    return _SINGLE_TABLES[(name, tag)]


def _interleave(tables):
    """Header + the tables' rows sorted by (chromosome, start)."""
    lines = [t.split(b"\n") for t in tables]
    assert all(ln[0] == lines[0][0] and ln[-1] == b"" for ln in lines)
    rows = sorted((r for ln in lines for r in ln[1:-1]), key=lambda r: (r.split(b"\t")[0].decode(), int(r.split(b"\t")[1])))
    return b"\n".join([lines[0][0]] + rows + [b""])


def _set(models, fa, names=CLASSES, kw=None):
    from mural_amd.predict import ModelSetForward
    members = {k: _member(models, k, None, **(kw or {}).get(k, {})) for k in names}
    return ModelSetForward(members, fasta_path=fa), members


def _set_table(models, files, out, names=CLASSES, kw=None, **run_kw):
    from mural_amd.predict import TsvSink, predict_regions_sharded
    d, fa = files
    fwd, members = _set(models, fa, names, kw)
    T = {}
    n = predict_regions_sharded(fwd, REGIONS, "SET", sink=TsvSink(d / out), collect=False, timings=T, **run_kw)
    return n, fwd, members, T, open(d / out, "rb").read()


def _site_count(names):
    return sum(len(py_sites(RECORDS[c], lo, hi, *SINGLE[k])) for c, iv in REGIONS.items() for lo, hi in iv for k in names)


# ---- 5. the table is the interleave ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("reuse", [False, True])
def test_set_table_is_the_interleave_of_the_single_tables(files, models, reuse):
    kw = dict(reuse=reuse)
    singles = [_single_table(models, files, k, f"reuse{reuse}", kw)[0] for k in CLASSES]
    assert len({t for t in singles}) == 3 and all(t.count(b"\n") > 50 for t in singles)
    n, fwd, members, _, got = _set_table(models, files, f"set_{reuse}.tsv", kw={k: kw for k in CLASSES})
    assert n == _site_count(CLASSES) == got.count(b"\n") - 1
    assert got == _interleave(singles)
    assert fwd.classes == 7 and fwd.model is members["A"].model and not fwd.calibrated
    if reuse:
        assert fwd.reuse_sites > 0
    rows = [r.split(b"\t") for r in got.split(b"\n")[1:-1]]
    assert [r[0] for r in rows if r[0] == b"chrFew"] == [b"chrFew"] * 2 and not any(r[0] == b"chrNone" for r in rows)


def test_a_row_through_another_member_is_another_row(files, models):
    """The three seeds give three functions: the A rows computed by the CpG member's model differ from the A member's."""
    from mural_amd.predict import HipShardForward, TsvSink, predict_regions_sharded
    d, fa = files
    want = _single_table(models, files, "A", "reuseFalse", dict(reuse=False))[0]
    other = HipShardForward(models["CpG"][0], fa, local_radius=R_LOCAL, local_order=3, reuse=False)
    predict_regions_sharded(other, REGIONS, "A", sink=TsvSink(d / "other.tsv"), collect=False)
    assert open(d / "other.tsv", "rb").read() != want


# ---- 6. ranks ----------------------------------------------------------------------------------------------------------------------------
def test_emulated_ranks_write_the_slices_of_the_interleave(files, models):
    from mural_amd.predict import TsvSink, predict_regions_sharded, shard_bounds
    d, fa = files
    kw = dict(reuse=False)
    body = _interleave([_single_table(models, files, k, "reuseFalse", kw)[0] for k in CLASSES]).split(b"\n")[1:-1]
    by_chrom = {}
    for ln in body:
        by_chrom.setdefault(ln.split(b"\t")[0], []).append(ln)
    assert sorted(by_chrom) == [b"chr10", b"chrA", b"chrFew"]
    for i in range(3):
        fwd, _ = _set(models, fa, kw={k: kw for k in CLASSES})
        out = d / "ranks.tsv"
        predict_regions_sharded(fwd, REGIONS, "SET", sink=TsvSink(out, parts=(i, 3)), collect=False, emulate=(i, 3))
        got = open(str(out) + ".part%04d" % i, "rb").read().split(b"\n")[:-1]
        want = []
        for c in sorted(by_chrom):
            lo, hi = shard_bounds(len(by_chrom[c]), i, 3)
            want += by_chrom[c][lo:hi]
        assert got == want, i


# ---- 7. per-member calibration ---------------------------------------------------------------------------------------------------------
def test_members_keep_their_own_calibration(files, models):
    from mural_amd.predict import ModelSetForward
    d, fa = files
    rng = np.random.default_rng(21)
    eye = np.hstack([np.eye(4), np.zeros((4, 1))])
    kw = {"A": dict(scale_factor=2.0, dirichlet_weights=eye + 0.2 * rng.standard_normal((4, 5))),
          "nonCpG": dict(scale_factor=3.0, dirichlet_weights=eye), "CpG": dict(scale_factor=0.5, dirichlet_weights=eye)}
    singles = [_single_table(models, files, k, "calibrated", kw[k])[0] for k in CLASSES]
    n, fwd, _, _, got = _set_table(models, files, "set_cal.tsv", kw=kw)
    assert fwd.calibrated and n == _site_count(CLASSES)
    assert got == _interleave(singles)
    assert got != _interleave([_single_table(models, files, k, "reuseTrue", dict(reuse=True))[0] for k in CLASSES])
    with pytest.raises(ValueError, match="calibrated"):
        ModelSetForward({"A": _member(models, "A", None, scale_factor=2.0), "CpG": _member(models, "CpG", None)}, fasta_path=fa)


# ---- 8. mutations ------------------------------------------------------------------------------------------------------------------------
def test_one_mutation_list_serves_every_member(files, models):
    d, fa = files
    picks = []
    for k in CLASSES:                        # a site of every class inside chrA's first region, behind the N run
        p, st = [ps for ps in py_sites(MAIN, 400, 700, *SINGLE[k])][3]
        picks.append((p, st, 1 + CLASSES.index(k)))
    assert MAIN[120] == "N"
    lines = sorted(picks + [(120, 0, 2)])
    muts = d / "muts.bed"
    muts.write_text("".join(f"chrA\t{p}\t{p + 1}\t.\t{lab}\t{'-' if st else '+'}\n" for p, st, lab in lines))
    singles = [_single_table(models, files, k, "muts", dict(reuse=False), mutations=str(muts)) for k in CLASSES]
    assert [T["mutations"]["matched"] for _, T in singles] == [1, 1, 1]
    n, _, _, T, got = _set_table(models, files, "set_muts.tsv", kw={k: dict(reuse=False) for k in CLASSES}, mutations=str(muts))
    assert got == _interleave([t for t, _ in singles])
    assert T["mutations"] == {"in_regions": 4, "matched": 3, "unmatched": 1}
    labels = {int(r.split(b"\t")[1]): r.split(b"\t")[4] for r in got.split(b"\n")[1:-1] if r.startswith(b"chrA\t")}
    assert all(float(labels[p]) == lab for p, _, lab in picks) and sum(float(v) != 0 for v in labels.values()) == 3
    with pytest.raises(ValueError, match="mutations"):
        _set_table(models, files, "set_strict.tsv", kw={k: dict(reuse=False) for k in CLASSES}, mutations=str(muts), strict_mutations=True)
    assert not (d / "set_strict.tsv").exists()


# ---- 9. two members ----------------------------------------------------------------------------------------------------------------------
def test_two_member_set_writes_its_classes_only(files, models):
    d, fa = files
    kw = dict(reuse=False)
    n, fwd, _, _, got = _set_table(models, files, "set_two.tsv", names=("A", "CpG"), kw={k: kw for k in ("A", "CpG")})
    assert fwd.classes == 5 and n == _site_count(("A", "CpG"))
    assert got == _interleave([_single_table(models, files, k, "reuseFalse", kw)[0] for k in ("A", "CpG")])
    # a row of the class the set lacks, handed to the forward directly: refused with its place
    p, st = py_sites(MAIN, 400, 700, "C", "nonCpG")[0]
    q, q_st = py_sites(MAIN, 400, 700, "A")[0]
    with pytest.raises(ValueError, match=f"chrA:{p} on strand '[{'+-'[st]}]'"):
        fwd("chrA", np.array([q, p], np.int64), np.array([q_st, st], np.uint8))
    with pytest.raises(ValueError, match="chrA:120 "):
        fwd("chrA", np.array([120], np.int64), np.array([0], np.uint8))
    assert fwd("chrA", np.zeros(0, np.int64), np.zeros(0, np.uint8)).shape == (0, 5)


def test_c_member_serves_both_contexts(files, models):
    """'C' = nonCpG | CpG through one model: the table of A + C is the interleave of the A table and the focal-C table."""
    from mural_amd.predict import HipShardForward, ModelSetForward, TsvSink, predict_regions_sharded
    d, fa = files
    mk = lambda name, f: HipShardForward(models[name][0], f, local_radius=R_LOCAL, local_order=3, reuse=False)      # noqa: E731
    predict_regions_sharded(mk("CpG", fa), REGIONS, "C", sink=TsvSink(d / "c_all.tsv"), collect=False)
    fwd = ModelSetForward({"A": mk("A", None), "C": mk("CpG", None)}, fasta_path=fa)
    assert fwd.classes == 7
    predict_regions_sharded(fwd, REGIONS, "SET", sink=TsvSink(d / "set_ac.tsv"), collect=False)
    want = _interleave([_single_table(models, files, "A", "reuseFalse", dict(reuse=False))[0], open(d / "c_all.tsv", "rb").read()])
    assert open(d / "set_ac.tsv", "rb").read() == want


# ---- 10. one upload ----------------------------------------------------------------------------------------------------------------------
def test_only_the_set_packs_and_uploads(files, models):
    n, fwd, members, _, _ = _set_table(models, files, "set_pack.tsv")
    assert n > 0 and fwd.seconds["pack"] > 0.0
    for m in members.values():
        assert m.seconds == {"pack_wait": 0.0, "pack": 0.0} and m._scan is None and m._resident == (None, None) and m.genome_from is fwd
    assert fwd._resident[0] == "chrNone"                  # the last chromosome by name; exactly one is resident
    # members that were built with the file are bound to the set as well
    from mural_amd.predict import ModelSetForward
    d, fa = files
    own = {k: _member(models, k, fa) for k in ("A", "CpG")}
    both = ModelSetForward(own)
    assert both.fasta_path == fa and all(m.genome_from is both for m in own.values())
    assert own["A"].genome("chrFew") is both.genome("chrFew") and own["A"].seconds["pack"] == 0.0
    with pytest.raises(RuntimeError, match="fasta_path=None"):
        _member(models, "A", None).genome("chrFew")


# ---- 11. command line --------------------------------------------------------------------------------------------------------------------
def test_command_line_writes_the_api_s_table(files, models):
    from mural_amd.model import nn_utils
    d, fa = files
    paths = {}
    for k in CLASSES:
        paths[k] = str(d / f"model_{k}")
        nn_utils.save_model(models[k][0], None, models[k][1], paths[k])
    spec = importlib.util.spec_from_file_location("predict_files", os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))),
                                                                                  "tools", "predict_files.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    spec_args = [f"{c}:{lo + 1}-{hi}" for c, iv in REGIONS.items() for lo, hi in iv]
    mod.main([fa, str(d / "cli.tsv"), "--regions", spec_args[0]] + [a for s in spec_args[1:] for a in ("--regions", s)]
             + ["--model_set"] + [f"{k}={paths[k]}" for k in CLASSES])
    assert open(d / "cli.tsv", "rb").read() == _set_table(models, files, "api.tsv")[4]
    # per-class factors: every member scaled behind its own head
    factors = {"A": 2.0, "nonCpG": 3.0, "CpG": 0.5}
    mod.main([fa, "--model_set=A=" + paths["A"], f"nonCpG={paths['nonCpG']}", f"CpG={paths['CpG']}", str(d / "cli_sf.tsv"), "--regions", "chrA:1-700",
              "--scale_factors"] + [f"{k}={v}" for k, v in factors.items()])
    from mural_amd.predict import TsvSink, predict_regions_sharded
    fwd, _ = _set(models, fa, kw={k: dict(scale_factor=v) for k, v in factors.items()})
    predict_regions_sharded(fwd, "chrA:1-700", "SET", sink=TsvSink(d / "api_sf.tsv"), collect=False)
    assert open(d / "cli_sf.tsv", "rb").read() == open(d / "api_sf.tsv", "rb").read()
    with pytest.raises(SystemExit, match="scale_factors"):
        mod.main([fa, str(d / "x.tsv"), "--regions", "chrA:1-700", "--model_set"] + [f"{k}={paths[k]}" for k in CLASSES] + ["--scale_factors", "A=2"])
