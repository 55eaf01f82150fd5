"""GPU tests of the mutagenesis profile (csrc/mutagenesis.hip: mural_mutagenesis_profile_window; mural_amd.mutagenesis.mutagenesis_profile;
DESIGN.md section 3.30): the device entry word for word against its numpy twin on both of its add paths, the profile against the twin
applied to the map of the same sites, and the ways the integer table must not depend on how it was reached."""
import functools

import numpy as np
import pytest
import torch

from tests import _mutagenesis_data as D
from tests import _mutagenesis_profile_data as P

pytestmark = pytest.mark.gpu


def _device_table(ref_logp, var_logp, ref_symbols, group, n_groups, chunk=None):
    """(table uint64, status ints) of the device entry over all ids in chunks of `chunk`."""
    from mural_amd.mutagenesis import MutagenesisProfile, mutagenesis_profile_window
    n, W = ref_symbols.shape
    prof = MutagenesisProfile.zeros((W - 1) // 2 if W % 2 else W // 2, "snv" if W % 2 else "indel", ref_logp.shape[1], n_groups, "cuda")
    rl, vl, rs = torch.from_numpy(ref_logp).cuda(), torch.from_numpy(var_logp).cuda(), torch.from_numpy(ref_symbols).cuda()
    gr = None if group is None else torch.from_numpy(group).cuda()
    total = len(var_logp)
    step = total if chunk is None else chunk
    for first in range(0, total, step):
        mutagenesis_profile_window(rl, vl[first:first + step].contiguous(), rs, gr, first, prof.table, prof.status)
    return prof.table_host(), prof.status_host()


def _twin_table(ref_logp, var_logp, ref_symbols, group, n_groups):
    from mural_amd.mutagenesis import mutagenesis_profile_host
    W = ref_symbols.shape[1]
    table, status = np.zeros((n_groups, W, 4, 3, ref_logp.shape[1], 5), np.uint64), np.zeros(3, np.uint64)
    mutagenesis_profile_host(ref_logp, var_logp, ref_symbols, group, 0, table, status)
    return table, tuple(int(x) for x in status)


@functools.lru_cache(maxsize=None)
def _edge_case():
    rows = P.synthetic()
    return rows, _twin_table(*rows, P.N_GROUPS), _twin_table(*rows[:3], None, 1)


@pytest.mark.parametrize("chunk", [1, 97, None])
@pytest.mark.parametrize("grouped", [True, False])
def test_device_entry_equals_the_twin_on_the_edge_rows(chunk, grouped):
    """R = 6, the synthetic rows with every edge of the quantisation (ties, the largest q, 256, infinities, NaN, dead columns, groups
    outside the table): every table word and status counter."""
    rows, with_groups, one_group = _edge_case()
    want_table, want_status = with_groups if grouped else one_group
    table, status = _device_table(*rows[:3], rows[3] if grouped else None, P.N_GROUPS if grouped else 1, chunk)
    assert status == want_status and status[1] >= P.EDGE_NONFINITE and status[2] >= P.EDGE_RANGE
    assert np.array_equal(table, want_table)
    if grouped:
        brute = P.brute_force(P.delta_map(*rows[:3]), rows[2], rows[3], P.N_GROUPS)
        assert np.array_equal(table, brute[0]) and status == brute[1]


@pytest.mark.parametrize("chunk", [1009, None])
def test_device_entry_equals_the_twin_at_radius_100(chunk):
    from mural_amd.mutagenesis import _codes, _window_symbols_host
    pos, strand = D.sites()
    ref_symbols, _ = _window_symbols_host(_codes(D.sequence()), pos, strand, 100)
    rng = np.random.default_rng(100)
    n, W, C = len(pos), 201, 3
    ref_logp = rng.normal(size=(n, C)).astype(np.float32)
    var_logp = (np.repeat(ref_logp, W * 3, axis=0) + rng.normal(0, 2.0, size=(n * W * 3, C))).astype(np.float32)
    var_logp[rng.integers(0, len(var_logp), size=50), rng.integers(0, C, size=50)] = np.float32(np.inf)
    group = rng.integers(-1, 3, size=n).astype(np.int32)
    want = _twin_table(ref_logp, var_logp, ref_symbols, group, 2)
    got = _device_table(ref_logp, var_logp, ref_symbols, group, 2, chunk)
    assert got[1] == want[1] and want[1][0] == 1 and np.array_equal(got[0], want[0])


@pytest.mark.parametrize("n_groups", [1, 3])
def test_contended_path_equals_the_twin(n_groups):
    """R = 6, 16 384 sites drawn with replacement from the fixture's 24: one chunk of 638 976 ids in which every cell receives thousands
    of terms, summed per block in LDS.  With three groups the third does not fit the block's table and is added to memory directly, and
    ids outside the table are among the sites."""
    from mural_amd.mutagenesis import _codes, _window_symbols_host
    pos, strand = D.sites()
    rng = np.random.default_rng(4096 + n_groups)
    pick = rng.integers(0, len(pos), size=16384)
    ref_symbols, _ = _window_symbols_host(_codes(D.sequence()), pos[pick], strand[pick], 6)
    n, W, C = 16384, 13, 4
    ref_logp = np.log(rng.dirichlet(np.ones(C), size=n)).astype(np.float32)
    var_logp = (np.repeat(ref_logp, W * 3, axis=0) + rng.normal(0, 3.0, size=(n * W * 3, C))).astype(np.float32)
    var_logp[rng.integers(0, len(var_logp), size=300), rng.integers(0, C, size=300)] = np.float32(300.0)
    var_logp[rng.integers(0, len(var_logp), size=300), rng.integers(0, C, size=300)] = np.float32(np.nan)
    group = None if n_groups == 1 else rng.integers(-1, n_groups + 1, size=n).astype(np.int32)
    want = _twin_table(ref_logp, var_logp, ref_symbols, group, n_groups)
    populated = want[0][..., 0][want[0][..., 0] > 0]
    assert np.median(populated) > (2000 if n_groups == 1 else 400) and int(populated.max()) > 1000
    got = _device_table(ref_logp, var_logp, ref_symbols, group, n_groups)
    assert got[1] == want[1] and want[1][0] == 3 and np.array_equal(got[0], want[0])
    # ... and through the adds to memory alone (calls too short for the LDS table): the same integers
    again = _device_table(ref_logp, var_logp, ref_symbols, group, n_groups, chunk=4099)
    assert again[1] == want[1] and np.array_equal(again[0], want[0])


def test_entry_refuses_bad_arguments():
    from mural_amd.mutagenesis import MutagenesisProfile, mutagenesis_profile_window
    rows, _, _ = _edge_case()
    rl, vl, rs = (torch.from_numpy(a).cuda() for a in rows[:3])
    prof = MutagenesisProfile.zeros(6, "snv", 4, 1, "cuda")
    with pytest.raises(ValueError, match="ids"):
        mutagenesis_profile_window(rl, vl[:5].contiguous(), rs, None, len(vl) - 4, prof.table, prof.status)
    with pytest.raises(ValueError):
        mutagenesis_profile_window(rl, vl, rs, torch.zeros(len(rl), dtype=torch.int64, device="cuda"), 0, prof.table, prof.status)
    with pytest.raises(RuntimeError, match="HIP device"):
        mutagenesis_profile_window(rl, vl, rs, None, 0, prof.table.cpu(), prof.status)
    mutagenesis_profile_window(rl, vl[:0], rs, None, 0, prof.table, prof.status)           # no ids: nothing launched
    assert not bool(prof.words.any())


# ----------------------------------------------------------------------------------------------------------------------------------
# the profile against the map
# ----------------------------------------------------------------------------------------------------------------------------------
def _sites_and_groups():
    from tests.test_gpu_mutagenesis import MAP_LENGTH, MAP_N_RUN
    pos = np.array([2, 2395, 2503, MAP_LENGTH - 2, 1000, MAP_N_RUN[0] - 3, 3000, 4100, 77], np.int64)
    strand = np.array([0, 1, 0, 1, 1, 0, 1, 0, 0], np.uint8)
    groups = np.array([0, 1, 2, 1, 0, 5, 2, -1, 1], np.int32)
    return pos, strand, groups


def _twin_of_the_map(res, groups, n_groups):
    """The twin applied to the ``delta`` of a MutagenesisMap: the alternatives' entries read back as (count, n_class) rows of differences
    from a reference of zero."""
    from mural_amd.mutagenesis import mutagenesis_profile_host
    delta, sym = res.delta.cpu().numpy(), res.ref_symbols.cpu().numpy()
    n, W, _, C = delta.shape
    ref = sym.astype(np.int64)[:, :, None]
    alt = np.arange(3)[None, None, :] + (np.arange(3)[None, None, :] >= ref)                       # (n, W, 3)
    rows = np.take_along_axis(delta, np.minimum(alt, 3)[..., None], axis=2).reshape(n * W * 3, C)   # dead columns: never read by the twin
    table, status = np.zeros((n_groups, W, 4, 3, C, 5), np.uint64), np.zeros(3, np.uint64)
    mutagenesis_profile_host(np.zeros((n, C), np.float32), rows, sym, groups, 0, table, status)
    return table, tuple(int(x) for x in status)


@pytest.mark.parametrize("model_no", [1, 2])
def test_profile_equals_the_twin_of_the_map_and_does_not_depend_on_how_it_was_reached(model_no):
    from mural_amd.data import PackedGenome
    from mural_amd.mutagenesis import MutagenesisProfile, mutagenesis_profile, saturation_mutagenesis
    from tests.test_gpu_mutagenesis import build_models, map_sequence
    r, R = 5, 100
    genome = PackedGenome.from_sequence(map_sequence(), "cuda")
    model, _ = build_models(r, R, model_no)
    pos_h, strand_h, groups_h = _sites_and_groups()
    pos, strand, groups = (torch.from_numpy(a).cuda() for a in (pos_h, strand_h, groups_h))
    res = saturation_mutagenesis(model, genome, pos, strand, local_radius=r, local_order=3)
    want_table, want_status = _twin_of_the_map(res, groups_h, 3)
    assert want_status == (0, 0, 0) and int(want_table[..., 0].sum()) > 0 and (want_table[..., 2] > 0).any()
    kw = dict(groups=groups, n_groups=3, local_radius=r, local_order=3)
    prof = mutagenesis_profile(model, genome, pos, strand, **kw)
    assert isinstance(prof, MutagenesisProfile) and prof.words.is_cuda
    assert (prof.radius, prof.model_type, prof.n_class, prof.n_groups) == (R, "snv", 4, 3)
    assert prof.status_host() == want_status and np.array_equal(prof.table_host(), want_table)
    # (a) any chunk_windows
    for chunk in (97, 4096):
        other = mutagenesis_profile(model, genome, pos, strand, chunk_windows=chunk, **kw)
        assert torch.equal(other.words, prof.words), chunk
    # (b) any order of the sites
    perm = torch.from_numpy(np.random.default_rng(5).permutation(len(pos_h))).cuda()
    other = mutagenesis_profile(model, genome, pos[perm], strand[perm], groups=groups[perm], n_groups=3, local_radius=r, local_order=3)
    assert torch.equal(other.words, prof.words)
    # (c) two calls joined by into=, and by merge
    first = mutagenesis_profile(model, genome, pos[:4], strand[:4], groups=groups[:4], n_groups=3, local_radius=r, local_order=3)
    second = mutagenesis_profile(model, genome, pos[4:], strand[4:], groups=groups[4:], n_groups=3, local_radius=r, local_order=3)
    joined = mutagenesis_profile(model, genome, pos[4:], strand[4:], groups=groups[4:], local_radius=r, local_order=3, into=first)
    assert joined is first and torch.equal(joined.words, prof.words)
    first = mutagenesis_profile(model, genome, pos[:4], strand[:4], groups=groups[:4], n_groups=3, local_radius=r, local_order=3)
    first += second
    assert torch.equal(first.words, prof.words)
    # no groups: one group of every site; timings has the three phases of the map's
    timings = {}
    plain = mutagenesis_profile(model, genome, pos, strand, local_radius=r, local_order=3, timings=timings)
    assert plain.n_groups == 1 and np.array_equal(plain.table_host(), _twin_of_the_map(res, None, 1)[0])
    assert sorted(timings) == ["forward_ms", "reduce_ms", "rows_encode_ms"]
    # the statistics come from the integers; the map is what it was
    assert np.array_equal(prof.mean(), MutagenesisProfile(prof.words.cpu(), R, "snv", 4, 3).mean(), equal_nan=True)
    again = saturation_mutagenesis(model, genome, pos, strand, local_radius=r, local_order=3)
    assert torch.equal(again.delta.view(torch.int32), res.delta.view(torch.int32))
    # into= refuses a profile of another shape
    with pytest.raises(ValueError, match="into"):
        mutagenesis_profile(model, genome, pos, strand, local_radius=r, local_order=3, into=MutagenesisProfile.zeros(R + 1, "snv", 4, 1, "cuda"))
    with pytest.raises(ValueError, match="into"):
        mutagenesis_profile(model, genome, pos, strand, local_radius=r, local_order=3, n_groups=2, into=prof)
    with pytest.raises(ValueError, match="groups"):
        mutagenesis_profile(model, genome, pos, strand, local_radius=r, local_order=3, groups=groups[:3])


def test_indel_profile_equals_the_twin_of_the_map_at_one_chunk_size():
    from mural_amd.data import PackedGenome
    from mural_amd.mutagenesis import mutagenesis_profile, saturation_mutagenesis
    from tests.test_gpu_mutagenesis_indel import MAP_SITES, map_sequence, models
    model, _, R = models("indel_synth_small.npz")
    genome = PackedGenome.from_sequence(map_sequence(), "cuda")
    pos, strand = torch.from_numpy(MAP_SITES[0]).cuda(), torch.from_numpy(MAP_SITES[1]).cuda()
    groups = (np.arange(len(MAP_SITES[0])) % 2).astype(np.int32)
    chunk = 1000
    res = saturation_mutagenesis(model, genome, pos, strand, distal_radius=R, chunk_windows=chunk)
    want_table, want_status = _twin_of_the_map(res, groups, 2)
    prof = mutagenesis_profile(model, genome, pos, strand, groups=groups, n_groups=2, distal_radius=R, chunk_windows=chunk)
    assert (prof.radius, prof.model_type, prof.n_class, prof.width) == (R, "indel", model.n_class, 2 * R)
    assert prof.status_host() == want_status and np.array_equal(prof.table_host(), want_table)
    assert int(want_table[..., 0].sum()) > 0 and np.array_equal(prof.offsets(), np.arange(-R + 1, R + 1))
    assert prof.by_distance().shape == (2, 2 * R, model.n_class)


def test_unsupported_models_and_inputs_raise_with_the_reason():
    """The refusals of tests/test_gpu_mutagenesis.py::test_unsupported_models_and_inputs_raise_with_the_reason, for the profile."""
    from mural_amd.data import PackedGenome
    from mural_amd.mutagenesis import mutagenesis_profile
    from tests.test_gpu_mutagenesis import build_models, map_sequence
    genome = PackedGenome.from_sequence(map_sequence(), "cuda")
    pos, strand = torch.tensor([1000, 2000], device="cuda"), torch.tensor([0, 1], dtype=torch.uint8, device="cuda")
    net0, _ = build_models(5, 100, 0)
    with pytest.raises(RuntimeError, match="Network0"):
        mutagenesis_profile(net0, genome, pos, strand)
    model, _ = build_models(5, 100, 2)
    model.train()
    with pytest.raises(RuntimeError, match="eval mode"):
        mutagenesis_profile(model, genome, pos, strand)
    model.eval()
    with pytest.raises(RuntimeError, match="HIP device"):
        mutagenesis_profile(model, genome, pos.cpu(), strand.cpu())
    on_cpu = build_models(5, 100, 1)[0].cpu()
    with pytest.raises(RuntimeError, match="HIP device"):
        mutagenesis_profile(on_cpu, genome, pos, strand)
    with pytest.raises(ValueError):
        mutagenesis_profile(model, genome, pos, strand, chunk_windows=0)
    empty = mutagenesis_profile(model, genome, pos[:0], strand[:0])
    assert empty.table.shape == (1, 201, 4, 3, 4, 5) and not bool(empty.words.any()) and np.isnan(empty.mean()).all()
