"""CPU tests of the mutagenesis profile's specification (mural_amd.mutagenesis.mutagenesis_profile_host, MutagenesisProfile): the numpy
twin against a brute force in Python ints, the float64 statistics against numpy over the valid terms, and the ways tables add (merge,
save / load, all_reduce_ over gloo)."""
import os

import numpy as np
import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

from tests import _mutagenesis_profile_data as P
from tests.test_dist_gloo import _free_port


def _twin_profile(first=0, count=None, sites=None, chunk=None):
    """A host MutagenesisProfile of the synthetic rows (optionally of some sites only: the others are sent to a group outside the
    table), the twin adding in place into the profile's own memory."""
    from mural_amd.mutagenesis import MutagenesisProfile, mutagenesis_profile_host
    ref_logp, var_logp, ref_symbols, group = P.synthetic()
    if sites is not None:
        keep = np.zeros(len(group), bool)
        keep[sites] = True
        group = np.where(keep, group, -1).astype(np.int32)
    prof = MutagenesisProfile.zeros(P.RADIUS, "snv", P.N_CLASS, P.N_GROUPS)
    table, status = prof.table_host(), prof.status.numpy().view(np.uint64)
    assert np.shares_memory(table, prof.words.numpy())
    count = len(var_logp) - first if count is None else count
    step = count if chunk is None else chunk
    for f in range(first, first + count, max(step, 1)):
        m = min(step, first + count - f)
        mutagenesis_profile_host(ref_logp, var_logp[f:f + m], ref_symbols, group, f, table, status)
    return prof


@pytest.fixture(scope="module")
def want():
    ref_logp, var_logp, ref_symbols, group = P.synthetic()
    delta = P.delta_map(ref_logp, var_logp, ref_symbols)
    return delta, ref_symbols, group, P.brute_force(delta, ref_symbols, group, P.N_GROUPS)


def test_the_edge_values_quantise_as_pinned():
    for value, q in P.EDGE:
        assert P.quantise(value) == q, value
    assert sum(q is None for _, q in P.EDGE) == P.EDGE_NONFINITE + P.EDGE_RANGE


@pytest.mark.parametrize("chunk", [None, 1, 97])
def test_twin_equals_the_brute_force_in_python_ints(want, chunk):
    _, _, _, (table, status) = want
    prof = _twin_profile(chunk=chunk)
    assert np.array_equal(prof.table_host(), table)
    assert prof.status_host() == status == (3, P.EDGE_NONFINITE, P.EDGE_RANGE)
    assert int(table[..., 0].sum()) > 2000 and (table[..., 1].view(np.int64) < 0).any() and (table[..., 4] > 0).any()
    # dead columns, and the groups outside [0, 3), added nothing: per group the terms are those of its own sites' plain columns
    for g in range(P.N_GROUPS):
        own = (want[2] == g)
        assert int(table[g, ..., 0].sum()) == int((want[1][own] < 4).sum()) * 3 * P.N_CLASS - (6 if g == want[2][P.EDGE_SITE] else 0)


def test_twin_of_a_mid_column_range_and_no_group_array(want):
    from mural_amd.mutagenesis import mutagenesis_profile_host
    ref_logp, var_logp, ref_symbols, _ = P.synthetic()
    delta, _, _, _ = want
    table, status = np.zeros((1, 13, 4, 3, 4, 5), np.uint64), np.zeros(3, np.uint64)
    for first, count in ((0, 40), (40, 1), (41, 500), (541, len(var_logp) - 541)):        # cuts mid-column and mid-site
        mutagenesis_profile_host(ref_logp, var_logp[first:first + count], ref_symbols, None, first, table, status)
    bt, bs = P.brute_force(delta, ref_symbols, None, 1)
    assert np.array_equal(table, bt) and tuple(int(x) for x in status) == bs
    with pytest.raises(ValueError):
        mutagenesis_profile_host(ref_logp, var_logp[:5], ref_symbols, None, len(var_logp) - 4, table)
    with pytest.raises(ValueError):
        mutagenesis_profile_host(ref_logp, var_logp, ref_symbols, None, 0, table.astype(np.int64))


def test_statistics_against_float64_numpy_over_the_valid_terms(want):
    delta, ref_symbols, group, _ = want
    prof = _twin_profile()
    n, W, _, C = delta.shape
    terms = {}
    for s in range(n):
        if not 0 <= group[s] < P.N_GROUPS:
            continue
        for j in range(W):
            ref = int(ref_symbols[s, j])
            for alt in range(4):
                for c in range(C):
                    d = np.float64(delta[s, j, alt, c])
                    if ref < 4 and alt != ref and np.isfinite(d) and abs(d) < 256:
                        terms.setdefault((int(group[s]), j, ref, alt, c), []).append(d)
    counts, mean, mean_abs, rms = prof.counts(), prof.mean(), prof.mean_abs(), prof.rms()
    for stat in (counts, mean, mean_abs, rms):
        assert stat.dtype == np.float64 and stat.shape == (P.N_GROUPS, W, 4, 4, C)
        assert np.array_equal(np.isnan(stat), np.isnan(counts))
    filled = np.zeros(counts.shape, bool)
    # Every term's q / 2^30 differs from its delta by e, |e| <= 2^-31 (round to nearest).  mean and mean |.| move by at most mean |e|:
    # the issue's 2^-30.  rms: sqrt(mean (d + e)^2) and sqrt(mean d^2) are the L2 norms of two vectors that differ by e, so by the
    # triangle inequality they differ by at most sqrt(mean e^2) <= 2^-31; float64 rounding of values below 256 adds less than 2^-40.
    for key, ds in terms.items():
        ds = np.array(ds)
        filled[key] = True
        assert counts[key] == len(ds)
        assert abs(mean[key] - ds.mean()) <= 2.0 ** -30
        assert abs(mean_abs[key] - np.abs(ds).mean()) <= 2.0 ** -30
        assert abs(rms[key] - np.sqrt((ds * ds).mean())) <= 2.0 ** -31 + 2.0 ** -40
    assert np.array_equal(filled, ~np.isnan(counts)) and filled.sum() > 500
    assert all(np.isnan(counts[:, :, b, b]).all() for b in range(4))                      # ref == alt
    # by_distance: mean |delta| over ref and alt weighted by n, per column, with the offsets beside it
    by, off = prof.by_distance(), prof.offsets()
    assert by.shape == (P.N_GROUPS, W, C) and np.array_equal(off, np.arange(-P.RADIUS, P.RADIUS + 1))
    for g in range(P.N_GROUPS):
        for j in range(W):
            for c in range(C):
                ds = np.concatenate([np.abs(v) for k, v in terms.items() if (k[0], k[1], k[4]) == (g, j, c)] or [np.zeros(0)])
                assert (np.isnan(by[g, j, c]) and not len(ds)) or abs(by[g, j, c] - ds.mean()) <= 2.0 ** -30
    from mural_amd.mutagenesis import MutagenesisProfile
    assert np.array_equal(MutagenesisProfile.zeros(4, "indel", 8).offsets(), np.arange(-3, 5))


def test_merge_save_load_and_the_shape_refusals(tmp_path):
    from mural_amd.mutagenesis import MutagenesisProfile
    whole = _twin_profile()
    a, b = _twin_profile(sites=np.arange(0, 11)), _twin_profile(sites=np.arange(11, 24))
    assert a.status_host()[1] == P.EDGE_NONFINITE and b.status_host() == (0, 0, 0)
    before = b.words.clone()
    merged = a.merge(b)
    assert merged is a and torch.equal(a.words, whole.words) and torch.equal(b.words, before)
    c = _twin_profile(sites=np.arange(0, 11))
    c += b
    assert torch.equal(c.words, whole.words)
    path = str(tmp_path / "p.npz")
    whole.save(path)
    with np.load(path, allow_pickle=False) as z:
        assert z["table"].dtype == np.uint64 and z["status"].dtype == np.uint64 and int(z["radius"]) == P.RADIUS
    back = MutagenesisProfile.load(path)
    assert torch.equal(back.words, whole.words)
    assert (back.radius, back.model_type, back.n_class, back.n_groups) == (P.RADIUS, "snv", P.N_CLASS, P.N_GROUPS)
    assert np.array_equal(back.mean(), whole.mean(), equal_nan=True)
    # what cannot add: another radius, window kind, class count, group count
    for other in (MutagenesisProfile.zeros(P.RADIUS + 1, "snv", P.N_CLASS, P.N_GROUPS), MutagenesisProfile.zeros(P.RADIUS, "indel", P.N_CLASS, P.N_GROUPS),
                  MutagenesisProfile.zeros(P.RADIUS, "snv", P.N_CLASS + 1, P.N_GROUPS), MutagenesisProfile.zeros(P.RADIUS, "snv", P.N_CLASS, 1)):
        with pytest.raises(ValueError):
            whole.merge(other)
    # ... and what into= refuses (mutagenesis_profile asks this of the profile it is to continue)
    whole.require_continues(P.RADIUS, "snv", P.N_CLASS, 1, "cpu")
    whole.require_continues(P.RADIUS, "snv", P.N_CLASS, P.N_GROUPS, "cpu")
    for args in ((P.RADIUS + 1, "snv", P.N_CLASS, 1), (P.RADIUS, "indel", P.N_CLASS, 1), (P.RADIUS, "snv", 8, 1), (P.RADIUS, "snv", P.N_CLASS, 2)):
        with pytest.raises(ValueError, match="into"):
            whole.require_continues(*args, "cpu")
    with pytest.raises(ValueError):
        MutagenesisProfile(torch.zeros(10, dtype=torch.int64), P.RADIUS, "snv", P.N_CLASS, 1)


def _worker(rank, world, port, q):
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
    dist.init_process_group("gloo", rank=rank, world_size=world)
    try:
        prof = _twin_profile(sites=np.arange(rank, 24, world))
        prof.all_reduce_()
        q.put((rank, prof.words.numpy().tobytes()))
    finally:
        dist.destroy_process_group()


def test_all_reduce_over_gloo_gives_the_single_process_table():
    want = _twin_profile()
    assert (want.table_host()[..., 1].view(np.int64) < 0).any()                           # negative sums: the int64 view wraps as uint64
    world = 2
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    port = _free_port()
    procs = [ctx.Process(target=_worker, args=(r, world, port, q)) for r in range(world)]
    for p in procs:
        p.start()
    res = sorted(q.get(timeout=120) for _ in procs)
    for p in procs:
        p.join(timeout=60)
        assert p.exitcode == 0
    for rank, words in res:
        assert words == want.words.numpy().tobytes(), rank


def test_the_tool_groups_sites_and_writes_one_row_per_populated_cell(tmp_path):
    """tools/mutagenesis_files.py --profile: the group ids of --group_by and the rows of a profile (a twin-built one, on the host)."""
    import importlib.util
    import types
    spec = importlib.util.spec_from_file_location("mutagenesis_files", os.path.join(os.path.dirname(os.path.dirname(
        os.path.abspath(__file__))), "tools", "mutagenesis_files.py"))
    tool = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(tool)
    bed_path = tmp_path / "sites.bed"
    bed_path.write_text("# a comment\nchr1\t5\t6\tcpg\t0\t+\nchr1\t9\t10\tother\t1\t-\n\nchr2\t7\t8\tcpg\t0\t-\n")
    bed = types.SimpleNamespace(start=np.array([5, 9, 7]), strand=np.array([0, 1, 1], np.uint8))
    assert tool.site_groups(bed, "none")[0] == ["all"] and tool.site_groups(bed, "none")[1].tolist() == [0, 0, 0]
    assert tool.site_groups(bed, "strand")[0] == ["+", "-"] and tool.site_groups(bed, "strand")[1].tolist() == [0, 1, 1]
    labels, ids = tool.site_groups(bed, "name", str(bed_path))
    assert labels == ["cpg", "other"] and ids.tolist() == [0, 1, 0] and ids.dtype == np.int32
    with pytest.raises(SystemExit):
        tool.site_groups(types.SimpleNamespace(start=np.array([5]), strand=np.array([0], np.uint8)), "name", str(bed_path))
    prof = _twin_profile()
    out = tmp_path / "p.mutagenesis.profile.tsv"
    assert tool.profile_name(str(tmp_path / "p")) == str(out)
    rows = tool.write_profile(str(out), prof, ["a", "b", "c"])
    lines = out.read_text().splitlines()
    counts = prof.counts()
    assert lines[0].split("\t") == ["group", "offset", "ref", "alt", "class", "n", "mean", "mean_abs", "rms"]
    assert rows == len(lines) - 1 == int((~np.isnan(counts)).sum())
    mean = prof.mean()
    for line in lines[1:40] + lines[-40:]:
        g, off, ref, alt, c, n, m, _, _ = line.split("\t")
        at = ("abc".index(g), int(off) + P.RADIUS, "ACGT".index(ref), "ACGT".index(alt), int(c) - 1)
        assert ref != alt and int(n) == counts[at] and float(m) == float("%.6g" % mean[at])
