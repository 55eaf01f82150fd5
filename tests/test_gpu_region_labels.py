"""Observed mutations joined to the enumerated sites of a regions run (csrc/sites.hip: mural_sites_label,
data.genome.label_sites, predict_regions_sharded(mutations=)): the lookup against its numpy twin, labels and both `stats` words
exactly; the regions + mutations table byte for byte against the table the BED path writes for the dense BED (every enumerated site a
row, its score taken from the list); the in-flight summaries of the two routes; ranks, counts, refusals and the command line."""
import importlib.util
import os

import numpy as np
import pytest
import torch

from tests.test_gpu_regions import LONG, MAIN, R_DISTAL, R_LOCAL, SECOND, TILE, py_sites

pytestmark = pytest.mark.gpu

NEVER = np.iinfo(np.int64).max
LABEL_MAX_BLOCKS = 1 << 12      # csrc/sites.hip: SL_MAX_BLOCKS blocks of 256 lanes; a longer call strides


# ---- 1. the lookup against its numpy twin ------------------------------------------------------------------------------------------------
def _lookup_case(n, m, variant, rng):
    """(pos, strand, (list start, strand, label)): `ends` keeps the list inside [pos[0], pos[-1]] with entries ON both (a match at the
    first and the last site = the first and the last list entry), `outside` adds entries below pos[0] and above pos[-1]."""
    span = 16 * max(n, m) + 64
    pos = np.sort(rng.choice(span, size=n, replace=False)).astype(np.int64) + 5000
    strand = rng.integers(0, 2, n).astype(np.uint8)
    if variant == "ends":
        must = [int(pos[0]), int(pos[-1])]
        pool = np.arange(pos[0], pos[-1] + 1) if pos[-1] - pos[0] + 1 >= m else np.arange(pos[0], pos[0] + 4 * m)
    else:
        must = [int(pos[0]) - 7, int(pos[-1]) + 9, int(pos[0]), int(pos[-1])]
        pool = np.arange(pos[0] - 3000, pos[-1] + 3000)
    must = list(dict.fromkeys(must))[:m]
    pool = np.setdiff1d(pool, must)
    on_site = np.intersect1d(pool, pos)
    take_sites = on_site[rng.permutation(len(on_site))[:(m - len(must)) // 2]]
    rest = np.setdiff1d(pool, take_sites)
    fill = rest[rng.permutation(len(rest))[:m - len(must) - len(take_sites)]]
    m_start = np.sort(np.r_[must, take_sites, fill]).astype(np.int64)
    assert len(m_start) == m and (np.diff(m_start) > 0).all()
    # the site's own strand on a matched entry (no mismatch yet), any strand elsewhere
    m_strand = rng.integers(0, 2, m).astype(np.uint8)
    at = np.searchsorted(pos, m_start).clip(max=n - 1)
    hit = pos[at] == m_start
    m_strand[hit] = strand[at[hit]]
    m_label = rng.integers(0, 4, m).astype(np.float32)
    return pos, strand, (m_start, m_strand, m_label)


def _device_labels(pos, strand, muts, check, cuts=None):
    """label_sites on device copies, in the calls `cuts` names (one by default): (labels, stats) back on the host."""
    from mural_amd.data.genome import label_sites, new_label_stats
    up = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()      # noqa: E731
    stats = new_label_stats(torch.device("cuda", torch.cuda.current_device()))
    dm = None if muts is None else tuple(up(a) for a in muts)
    cuts = [0, len(pos)] if cuts is None else cuts
    out = [label_sites(up(pos[a:b]), up(strand[a:b]), dm, check, stats) for a, b in zip(cuts[:-1], cuts[1:])]
    assert all(o.dtype == torch.float32 and o.is_cuda for o in out)
    return torch.cat(out).cpu().numpy(), stats.cpu().tolist()


def _host_labels(pos, strand, muts, check):
    from mural_amd.data.genome import label_sites_host, new_label_stats
    stats = new_label_stats()
    return label_sites_host(pos, strand, muts, check, stats), stats.tolist()


@pytest.mark.parametrize("n", [1, 63, 64, 65, 4097])
def test_lookup_equals_the_numpy_twin(n):
    rng = np.random.default_rng(n)
    for m in (0, 1, 2, 3, 1025):
        for variant in ("ends", "outside"):
            pos, strand, muts = _lookup_case(n, m, variant, rng)
            if m >= 2 and variant == "outside":
                assert muts[0][0] < pos[0] and muts[0][-1] > pos[-1]
            if variant == "ends" and m >= 1:
                assert muts[0][0] == pos[0] and (muts[0][-1] == pos[-1] or n == 1 or m == 1)
            want, want_stats = _host_labels(pos, strand, muts, True)
            got, stats = _device_labels(pos, strand, muts if m else None, True)
            assert np.array_equal(got, want) and stats == want_stats, (m, variant)
            assert want_stats[1] == NEVER and (want_stats[0] >= min(m, 1) or variant == "outside")
            if m == 1025 and n > 1:
                assert 0 < want_stats[0] and (want != 0).any()
            if n > 1:                                      # two calls accumulate to the one-call result
                got2, stats2 = _device_labels(pos, strand, muts if m else None, True, [0, n // 2, n])
                assert np.array_equal(got2, want) and stats2 == want_stats
            # planted strand mismatches: stats[1] is the SMALLEST list index among them; check_strand = 0 leaves the word alone
            on = np.nonzero(np.isin(muts[0], pos))[0]
            if len(on):
                flip = on[[len(on) // 2, -1]]
                bad = (muts[0], muts[1].copy(), muts[2])
                bad[1][flip] ^= 1
                want_bad, host_bad = _host_labels(pos, strand, bad, True)
                assert host_bad == [want_stats[0], int(flip.min())] and np.array_equal(want_bad, want)
                assert _device_labels(pos, strand, bad, True)[1] == host_bad
                if n > 1:
                    assert _device_labels(pos, strand, bad, True, [0, n // 2, n])[1] == host_bad
                got0, stats0 = _device_labels(pos, strand, bad, False)
                assert np.array_equal(got0, want) and stats0 == [want_stats[0], NEVER]


def test_lookup_strides_over_a_call_longer_than_its_grid():
    """More sites than the capped grid has lanes: every lane takes a second site, the last ones a third."""
    n, m = LABEL_MAX_BLOCKS * 256 * 2 + 300, 20_001
    rng = np.random.default_rng(8)
    pos = np.cumsum(rng.integers(1, 4, n)).astype(np.int64)
    strand = (pos & 1).astype(np.uint8)
    m_start = np.unique(np.r_[pos[0], pos[-1], pos[-300:][::7], rng.integers(0, pos[-1] + 50, m)])
    muts = (m_start, (m_start & 1).astype(np.uint8), rng.integers(1, 4, len(m_start)).astype(np.float32))
    last = int(np.searchsorted(m_start, pos[-1]))
    muts[1][last] ^= 1                                     # the one mismatch sits on pos[-1]: a site only the stride reaches
    want, want_stats = _host_labels(pos, strand, muts, True)
    got, stats = _device_labels(pos, strand, muts, True)
    assert want[0] != 0 and want[-1] != 0 and want_stats[1] == last and want_stats[0] > m // 4
    assert np.array_equal(got, want) and stats == want_stats


def test_lookup_argument_errors_and_empty_calls():
    from mural_amd import _lib
    from mural_amd.data.genome import label_sites, new_label_stats
    dev = torch.device("cuda", torch.cuda.current_device())
    lib, stream = _lib.lib(), _lib.current_stream_ptr(dev)
    stats = new_label_stats(dev)
    pos, strand = torch.tensor([4, 9], device=dev), torch.tensor([0, 1], dtype=torch.uint8, device=dev)
    out = torch.full((2,), 7.0, device=dev)
    # n == 0 launches nothing, whatever the pointers; m == 0 writes zeros and reads no list pointer
    assert lib.mural_sites_label(None, None, 0, None, None, None, 5, 1, None, None, stream) == 0
    assert label_sites(pos, strand, None, True, stats, out=out) is out and out.tolist() == [0.0, 0.0] and stats.tolist() == [0, NEVER]
    for bad in ((pos.data_ptr(), strand.data_ptr(), -1, None, None, None, 0, 1, out.data_ptr(), stats.data_ptr()),
                (pos.data_ptr(), strand.data_ptr(), 2, None, None, None, -1, 1, out.data_ptr(), stats.data_ptr()),
                (pos.data_ptr(), strand.data_ptr(), 2, None, None, None, 3, 1, out.data_ptr(), stats.data_ptr()),
                (None, strand.data_ptr(), 2, None, None, None, 0, 1, out.data_ptr(), stats.data_ptr()),
                (pos.data_ptr(), strand.data_ptr(), 2, None, None, None, 0, 1, out.data_ptr(), None)):
        with pytest.raises(ValueError, match="sites_label"):
            _lib.check(lib.mural_sites_label(*bad, stream))
    with pytest.raises(ValueError, match="label_sites"):
        label_sites(pos.cpu(), strand, None, True, stats)
    with pytest.raises(ValueError, match="label_sites"):
        label_sites(pos, strand.to(torch.int64), None, True, stats)


# ---- files, models and mutation lists of the table tests ------------------------------------------------------------------------------
RECORDS = {"chrA": MAIN, "chr10": SECOND, "chrL": LONG[:9800], "chrFew": "CCGCCACCGGTCCCGG"}      # (file order; chr10 < chrA by name)
# chrA: two regions with a run of N inside; chr10: in the regions, not in any list; chrL: one region longer than a tile of the enumeration
# (the tiles count from the region's first word); chrFew: in the lists, in no region
REGIONS = {"chrA": [(40, 2500), (2950, 4990)], "chr10": [(0, len(SECOND))], "chrL": [(100, 9500)]}
assert REGIONS["chrL"][0][1] - REGIONS["chrL"][0][0] > TILE and "N" in MAIN[40:2500]


@pytest.fixture(scope="module")
def files(tmp_path_factory):
    d = tmp_path_factory.mktemp("region_labels")
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


class Listed:
    """A mutation list for a selection over `regions`: about a fifth of the enumerated sites (labels 0 .. n_class - 1, a 0 counts as
    matched), the first and the last site of every region, the bases just outside every region, an N and a base of the other kind
    inside one, and a chromosome no region names.  `rows`: [(chrom, start, label, strand)] in a shuffled order."""

    def __init__(self, regions, focal, context="all", n_class=4, skip=("chr10",), seed=3):
        rng = np.random.default_rng(seed)
        self.regions, self.focal, self.context = regions, focal, context
        self.sites = {c: [s for lo, hi in iv for s in py_sites(RECORDS[c], lo, hi, focal, context)] for c, iv in regions.items()}
        rows, self.in_regions, self.wrong_base, self.on_n = {}, 0, None, None
        for c, iv in regions.items():
            if c in skip:
                continue
            seq = RECORDS[c].upper()
            for lo, hi in iv:
                s = py_sites(RECORDS[c], lo, hi, focal, context)
                for p, st in s:
                    if rng.random() < 0.2:
                        rows[(c, p)] = (int(rng.integers(0, n_class)), st)
                rows[(c, s[0][0])], rows[(c, s[-1][0])] = (1, s[0][1]), (n_class - 1, s[-1][1])      # both ends of the region
                for p in (lo - 1, hi):                     # just outside it: whatever lies there, it labels no row
                    if 0 <= p < len(seq):
                        rows[(c, p)] = (2, int(seq[p] in "TG"))
            lo, hi = iv[0]
            if "N" in seq[lo:hi]:
                self.on_n = (c, lo + seq[lo:hi].index("N"))
                rows[self.on_n] = (1, 0)
            other = "CG" if focal == "A" else "AT" if focal == "C" else ""
            p = next((p for p in range(lo + 5, hi) if seq[p] in other), None)
            if p is not None and self.wrong_base is None:
                self.wrong_base = (c, p)
                rows[self.wrong_base] = (3, 0)
        rows[("chrFew", 5)] = (1, 0)
        self.by_site = rows
        keys = list(rows)
        self.rows = [(c, p, *rows[(c, p)]) for c, p in (keys[i] for i in rng.permutation(len(keys)))]

    def counts(self):
        """timings['mutations'] from the sequence and the list: plain loops."""
        inside = [(c, p) for c, p in self.by_site if any(lo <= p < hi for lo, hi in self.regions.get(c, []))]
        matched = sum((c, p) in {(c, q) for q, _ in self.sites[c]} for c, p in inside)
        return {"in_regions": len(inside), "matched": matched, "unmatched": len(inside) - matched}

    def write(self, path, drop=(), flip=None):
        with open(path, "w") as fh:
            fh.write("".join(f"{c}\t{p}\t{p + 1}\t.\t{lab}\t{'+-'[st ^ int((c, p) == flip)]}\n" for c, p, lab, st in self.rows if (c, p) not in drop))
        return str(path)

    def dense_bed(self, path):
        """Every enumerated site a row, its score taken from the list: the BED a user had to write before."""
        with open(path, "w") as fh:
            for c in RECORDS:
                for p, st in self.sites.get(c, []):
                    fh.write(f"{c}\t{p}\t{p + 1}\t.\t{self.by_site.get((c, p), (0,))[0]}\t{'+-'[st]}\n")
        return str(path), sum(len(s) for s in self.sites.values())


def _forward(snv_model, fa, **kw):
    from mural_amd.predict import HipShardForward
    return HipShardForward(snv_model[0], fa, local_radius=R_LOCAL, local_order=3, **kw)


def _labelled_table(snv_model, fa, out, listed, mutations, fwd_kw=None, sink=None, **kw):
    from mural_amd.predict import TsvSink, predict_regions_sharded
    fwd = _forward(snv_model, fa, **(fwd_kw or {}))
    n = predict_regions_sharded(fwd, listed.regions, listed.focal, listed.context, sink=sink or TsvSink(out), collect=False,
                                mutations=mutations, **kw)
    return n, open(out, "rb").read() if os.path.exists(out) else None


def _labels_of(table):
    return [ln.split(b"\t")[4] for ln in table.split(b"\n")[1:-1]]


# ---- 2. table parity against the BED path's table for the dense BED -------------------------------------------------------------------
@pytest.mark.parametrize("focal,context,fwd_kw", [
    ("A", "all", dict(reuse=True)), ("A", "all", dict(reuse=False)), ("C", "CpG", dict(reuse=True)), ("C", "CpG", dict(reuse=False)),
    ("A", "all", dict(reuse=True, poisson=True)), ("C", "nonCpG", dict(reuse=False, poisson=True))])
def test_labelled_region_table_is_the_bed_path_s_table(files, snv_model, focal, context, fwd_kw):
    from mural_amd.predict import TsvSink, predict_bed_sharded
    d, fa = files
    listed = Listed(REGIONS, focal, context)
    assert listed.wrong_base is not None and listed.on_n is not None and listed.counts()["unmatched"] >= 2
    T = {}
    n, got = _labelled_table(snv_model, fa, d / "r.tsv", listed, listed.write(d / "m.bed"), fwd_kw, timings=T)
    bed, rows = listed.dense_bed(d / "dense.bed")
    m = predict_bed_sharded(_forward(snv_model, fa, **fwd_kw), bed, sink=TsvSink(d / "b.tsv"), collect=False)
    want = open(d / "b.tsv", "rb").read()
    assert n == m == rows and want.count(b"\n") == rows + 1
    assert got == want
    assert len(set(_labels_of(got))) == 4                          # mut_type 0 .. 3 all occur
    assert T["mutations"] == listed.counts() and T["label"] > 0.0
    # what read_mutations returns is taken as well as the path
    from mural_amd.data.ingest import read_mutations
    assert _labelled_table(snv_model, fa, d / "r2.tsv", listed, read_mutations(d / "m.bed", 4), fwd_kw)[1] == want


def test_labelled_indel_region_table_is_the_bed_path_s_table(files):
    from mural_amd.predict import HipShardForward, TsvSink, predict_bed_sharded, predict_regions_sharded
    from tests import _util as U
    from tests.test_gpu_indel import product_from
    d, fa = files
    fx = U.load("indel_synth_small.npz")
    model = product_from(fx)
    model.load_state_dict(U.indel_state_for(fx, U.indel_oracle_from_hp(fx["hp"], fx["down"])))
    model = model.cuda().eval()
    R, k = int(fx["hp"][0]), int(model.n_class)
    listed = Listed({"chrA": [(60, 420)]}, "ANY", n_class=k)        # N runs and IUPAC codes inside
    assert listed.on_n is not None and listed.wrong_base is None and 200 < len(listed.sites["chrA"]) < 360
    # every strand in the list is taken as it is: every position is a '+' site and no strand is compared
    rows = [(c, p, lab, int(i % 2)) for i, (c, p, lab, _) in enumerate(listed.rows)]
    listed.rows = rows
    make = lambda: HipShardForward(model, fa, local_radius=R_LOCAL, local_order=3, distal_radius=R, model_type="indel")      # noqa: E731
    T = {}
    n = predict_regions_sharded(make(), "chrA:61-420", "ANY", model_type="indel", sink=TsvSink(d / "ir.tsv"), collect=False,
                                mutations=listed.write(d / "im.bed"), timings=T)
    bed, n_rows = listed.dense_bed(d / "i.bed")
    predict_bed_sharded(make(), bed, model_type="indel", sink=TsvSink(d / "ib.tsv"), collect=False)
    got = open(d / "ir.tsv", "rb").read()
    assert n == n_rows and got.count(b"\n") == n_rows + 1 and got == open(d / "ib.tsv", "rb").read()
    assert len(set(_labels_of(got))) == k and T["mutations"] == listed.counts()
    (d / "big.bed").write_text(f"chrA\t70\t71\t.\t{k}\t+\n")
    with pytest.raises(ValueError, match="chrA:70"):                # a label the model has no class for
        predict_regions_sharded(make(), "chrA:61-420", "ANY", model_type="indel", collect=False, mutations=str(d / "big.bed"))


# ---- 3. the in-flight summaries of the two routes ---------------------------------------------------------------------------------------
RTOL = 1e-12                   # tests/test_gpu_summary.py: the float64 bound of a window's sum in any order


def test_summaries_of_the_two_routes_agree(files, snv_model, monkeypatch):
    from mural_amd import predict as P
    from mural_amd import tables
    d, fa = files
    monkeypatch.setattr(P, "_ALIGNED_PART_ROWS", 700)      # several parts per chromosome: the stats words accumulate over them
    listed = Listed(REGIONS, "A")
    kw = dict(windows=(1000, 64), kmers=(3, 5), motifs=(3, 5))
    fwd = _forward(snv_model, fa)
    by_regions = P.SummarySink(d / "sr", genome=fwd.genome, **kw)
    T = {}
    n = P.predict_regions_sharded(fwd, REGIONS, "A", sink=by_regions, collect=False, mutations=listed.write(d / "sm.bed"), timings=T)
    fwd = _forward(snv_model, fa)
    by_bed = P.SummarySink(d / "sb", genome=fwd.genome, **kw)
    bed, rows = listed.dense_bed(d / "sdense.bed")
    assert P.predict_bed_sharded(fwd, bed, sink=by_bed, collect=False) == rows == n
    assert T["aligned_shards"] == 3 and T["mutations"] == listed.counts()
    a, b = by_regions.result(), by_bed.result()
    on_site = {(c, q) for c, s in listed.sites.items() for q, _ in s}
    mutated = sum(1 for key, (lab, _) in listed.by_site.items() if lab and key in on_site)
    assert mutated > 100
    # the integer k-mer and motif tables bit for bit, the order of first appearance with them
    for k in kw["kmers"]:
        assert a["kmers"][k][0] == b["kmers"][k][0]
        assert all(np.array_equal(x, y) for x, y in zip(by_regions.kmer_sums()[k], by_bed.kmer_sums()[k]))
    for m in kw["motifs"]:
        assert a["motifs"][m][0] == b["motifs"][m][0]
        assert all(np.array_equal(x, y) for x, y in zip(by_regions.motif_sums()[m], by_bed.motif_sums()[m]))
    # the window tables and the scaling totals as tests/test_gpu_summary.py compares two reductions of the same rows
    for W in kw["windows"]:
        (ka, ta), (kb, tb) = a["windows"][W], b["windows"][W]
        assert ka == kb and np.array_equal(ta[:, :5], tb[:, :5])
        err = np.abs(ta[:, 5:] - tb[:, 5:])
        print("W", W, "largest relative difference of a probability sum", float((err / np.maximum(tb[:, 5:], 1e-300)).max()))
        assert (err <= RTOL * tb[:, 5:]).all()
        assert ta[:, 2:5].sum() == mutated
    assert a["n_sites"] == b["n_sites"] == n and abs(a["prob_sum"] - b["prob_sum"]) <= RTOL * b["prob_sum"]
    # the correlations carry signal now: without labels every observed rate is 0 and no r is a finite non-zero number
    names = [tables.regional_output_names(str(d / "sr"), 1000)[1]] + [tables.kmer_output_names(str(d / "sr"), k)[1] for k in kw["kmers"]] \
        + [tables.motif_output_names(str(d / "sr"), m)[1] for m in kw["motifs"]]
    r = [float(ln.split("\t")[2]) for p in names for ln in open(p)]
    print("r", r)
    assert len(r) == 3 * len(names) and any(np.isfinite(v) and v != 0.0 for v in r)
    r_bed = [float(ln.split("\t")[2]) for p in names for ln in open(p.replace(str(d / "sr"), str(d / "sb")))]
    assert np.allclose(r, r_bed, rtol=0, atol=1e-5, equal_nan=True)      # (the files print r with five decimals)


# ---- 4. ranks ---------------------------------------------------------------------------------------------------------------------------
def test_emulated_ranks_label_their_slices(files, snv_model):
    from mural_amd.predict import TsvSink, shard_bounds
    d, fa = files
    listed = Listed(REGIONS, "A")
    mut = listed.write(d / "em.bed")
    T1 = {}
    n, table = _labelled_table(snv_model, fa, d / "w1.tsv", listed, mut, timings=T1)
    body = table.split(b"\n")[1:-1]
    by_chrom = {}
    for ln in body:
        by_chrom.setdefault(ln.split(b"\t")[0], []).append(ln)
    parts, matched = [], []
    for i in range(3):
        out, T = d / "w3.tsv", {}
        _labelled_table(snv_model, fa, out, listed, mut, sink=TsvSink(out, parts=(i, 3)), emulate=(i, 3), timings=T)
        parts.append(open(str(out) + ".part%04d" % i, "rb").read().split(b"\n")[:-1])
        want = []
        for c in sorted(by_chrom):
            lo, hi = shard_bounds(len(by_chrom[c]), i, 3)
            want += by_chrom[c][lo:hi]
        assert parts[i] == want, i
        assert T["mutations"]["in_regions"] == T1["mutations"]["in_regions"]
        matched.append(T["mutations"]["matched"])
    assert sorted((ln for p in parts for ln in p), key=lambda ln: ln.split(b"\t")[0]) == body
    print("matched per rank", matched)
    assert sum(matched) == T1["mutations"]["matched"] == listed.counts()["matched"] and min(matched) > 0
    from mural_amd.predict import predict_regions_sharded
    with pytest.raises(ValueError, match="strict_mutations"):      # one rank's matches say nothing about the list
        predict_regions_sharded(_forward(snv_model, fa), REGIONS, "A", collect=False, emulate=(1, 3), mutations=mut, strict_mutations=True)


# ---- 5. refusals ------------------------------------------------------------------------------------------------------------------------
def test_strict_mutations_raises_on_the_wrong_base_entry(files, snv_model):
    d, fa = files
    listed = Listed({"chrA": [(3000, 3400)]}, "A")              # the all-A stretch and what follows: no N inside
    assert listed.on_n is None and listed.wrong_base is not None and listed.counts()["unmatched"] == 1
    n, plain = _labelled_table(snv_model, fa, d / "s0.tsv", listed, listed.write(d / "s.bed"))      # counted, not refused
    assert n == len(listed.sites["chrA"])
    with pytest.raises(ValueError, match=r"1 of the \d+ listed mutations"):
        _labelled_table(snv_model, fa, d / "s1.tsv", listed, listed.write(d / "s.bed"), strict_mutations=True)
    assert not (d / "s1.tsv").exists()
    T = {}
    n, got = _labelled_table(snv_model, fa, d / "s2.tsv", listed, listed.write(d / "s.bed", drop={listed.wrong_base}), strict_mutations=True,
                             timings=T)
    assert got == plain and T["mutations"]["unmatched"] == 0 and T["mutations"]["matched"] == listed.counts()["matched"]


def test_a_strand_mismatch_raises_and_leaves_no_table(files, snv_model):
    d, fa = files
    listed = Listed(REGIONS, "C", "CpG")
    c, p = "chrL", listed.sites["chrL"][len(listed.sites["chrL"]) // 2][0]
    listed.by_site[(c, p)] = (2, listed.sites["chrL"][len(listed.sites["chrL"]) // 2][1])
    listed.rows = [r for r in listed.rows if (r[0], r[1]) != (c, p)] + [(c, p, *listed.by_site[(c, p)])]
    st = listed.by_site[(c, p)][1]
    with pytest.raises(ValueError) as err:
        _labelled_table(snv_model, fa, d / "x.tsv", listed, listed.write(d / "x.bed", flip=(c, p)))
    msg = str(err.value)
    assert f"{c}:{p}" in msg and f"strand '{'+-'[st ^ 1]}'" in msg and f"strand '{'+-'[st]}'" in msg
    assert not (d / "x.tsv").exists() and not [f for f in os.listdir(d) if f.startswith("x.tsv")]
    # the same list with the entry as it should be goes through
    assert _labelled_table(snv_model, fa, d / "x.tsv", listed, listed.write(d / "x.bed"))[1] is not None


# ---- 6. command line ----------------------------------------------------------------------------------------------------------------------
def test_command_line_writes_the_api_s_table(files, snv_model, capsys):
    from mural_amd.model import nn_utils
    d, fa = files
    ckpt = str(d / "model")
    nn_utils.save_model(snv_model[0], None, snv_model[1], ckpt)
    spec = importlib.util.spec_from_file_location("predict_files", os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))),
                                                                                  "tools", "predict_files.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    listed = Listed({"chrA": [(0, 3000)]}, "A")
    mut = listed.write(d / "cli.bed")
    mod.main([ckpt, fa, str(d / "cli.tsv"), "--regions", "chrA:1-3000", "--focal", "A", "--mutations", mut])
    n, want = _labelled_table(snv_model, fa, d / "api.tsv", listed, mut)
    assert open(d / "cli.tsv", "rb").read() == want and len(set(_labels_of(want))) == 4
    c = listed.counts()
    assert f"mutations inside the regions: {c['in_regions']}, on an enumerated site: {c['matched']}, on none: {c['unmatched']}" in capsys.readouterr().out
    with pytest.raises(ValueError, match="listed mutations"):
        mod.main([ckpt, fa, str(d / "cli2.tsv"), "--regions", "chrA:1-3000", "--mutations", mut, "--strict_mutations"])
    assert not (d / "cli2.tsv").exists()
    bed, _ = listed.dense_bed(d / "cli_dense.bed")
    for argv in ([ckpt, fa, bed, str(d / "cli3.tsv"), "--mutations", mut], [ckpt, fa, bed, str(d / "cli3.tsv"), "--strict_mutations"]):
        with pytest.raises(SystemExit, match="--regions"):
            mod.main(argv)
    assert not (d / "cli3.tsv").exists()
