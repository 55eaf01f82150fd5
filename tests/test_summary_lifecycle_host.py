"""The lifecycle the table reducers of SummarySink share (``summaries._TableReducer``), on the host: ``merge`` adds the states of the
ranks table by table and folds the limb tables' carries -- ``_kmer_fold`` for the annotation table, ``_conseq_fold`` for the three
[transcripts][bins][3] tables, none for the row counters and the uint32 replicate tables --, skips ranks without a state and never
hands back one of its inputs."""
import io

import numpy as np
import pytest

from tests import _conseq_data as D

BED12 = "\n".join([D.bed12("chr1", "plus", "+", [(10, 40), (60, 90)], (20, 80)), D.bed12("chr1", "minus", "-", [(30, 70)], (35, 60))]) + "\n"
ANNOTATIONS = {"chr1": [(0, 50, "a"), (40, 120, "b")]}
SIM = dict(simulate=3, simulate_seed=1)
# reducer -> (the sink's keywords, classes, the fold of its first table by name)
CASES = {
    "annotations": (dict(annotations=ANNOTATIONS), 4, "_kmer_fold"),
    "consequences": (dict(transcripts=BED12), 4, "_conseq_fold"),
    "transcript_structure": (dict(transcripts=BED12, transcript_structure=True), 4, "_conseq_fold"),
    "indel_structure": (dict(indel_transcripts=BED12, indel_kind="insertion"), 8, "_conseq_fold"),
    "simulation": (dict(annotations=ANNOTATIONS, **SIM), 4, None),
    "consequence_simulation": (dict(transcripts=BED12, simulate_transcripts=True, **SIM), 4, None),
    "structure_simulation": (dict(transcripts=BED12, transcript_structure=True, simulate_transcripts=True, simulate_structure=True, **SIM), 4, None),
    "indel_structure_simulation": (dict(indel_transcripts=BED12, indel_kind="insertion", simulate_indel_structure=True, **SIM), 8, None),
}


def _reducer(name):
    from mural_amd.summaries import SummarySink
    kw, k, fold = CASES[name]
    sink = SummarySink(None, genome=lambda chrom: "ACGT" * 40, **{key: io.StringIO(v) if v is BED12 else v for key, v in kw.items()})
    return sink._reducers[name], k, fold


def _states(spec):
    """Two states of random tables; in a limb table the lo limbs of `a` are the mask and those of `b` 1: every low sum carries."""
    from mural_amd.summaries import _KMER_LO_MASK
    rng = np.random.default_rng(3)
    a = [rng.integers(1, 1000, size=shape).astype(dtype) for _, shape, dtype, _ in spec]
    b = [rng.integers(1, 1000, size=shape).astype(dtype) for _, shape, dtype, _ in spec]
    for x, y, (_, shape, _, fold) in zip(a, b, spec):
        if fold is not None:
            lo = (slice(None), 2) if len(shape) == 3 and shape[1] == 3 else (slice(None), slice(None), 2)      # [names][3][k] or [tx][bins][3]
            x[lo], y[lo] = _KMER_LO_MASK, 1
    return a, b


@pytest.mark.parametrize("name", sorted(CASES))
def test_merge_adds_folds_skips_and_copies(name):
    from mural_amd import summaries
    r, k, fold = _reducer(name)
    spec = r._tables(k)
    assert [s[3] for s in spec] == [getattr(summaries, fold) if fold else None] + [None] * (len(spec) - 1)
    assert all(shape[0] == 2 and np.prod(shape) > 0 for _, shape, _, _ in spec)      # two transcripts or names
    a, b = _states(spec)
    state = (lambda t: t[0]) if len(spec) == 1 else tuple
    wrap = (lambda st: dict(table=st, index={})) if name == "simulation" else (lambda st: st)      # (its state carries the lists' index)
    table = (lambda st: st["table"]) if name == "simulation" else (lambda st: st)
    none = wrap(None) if name == "simulation" else None
    before = [t.copy() for t in a + b]

    got = table(r.merge([wrap(state(a)), none, wrap(state(b))], k))
    got = [got] if len(spec) == 1 else list(got)
    for have, x, y, (_, _, dtype, f) in zip(got, a, b, spec):
        want = x + y
        if f is not None:
            lo = (lambda t: t[:, 2]) if f is summaries._kmer_fold else (lambda t: t[:, :, 2])
            assert (lo(want) >> np.uint64(40) == 1).all()      # every low sum carries: a dropped fold shows
            f(want)
            assert not (lo(want) >> np.uint64(40)).any()
        assert have.dtype == dtype and have.tobytes() == want.tobytes()
    assert all(t.tobytes() == u.tobytes() for t, u in zip(a + b, before))

    assert table(r.merge([none, none], k)) is None
    one = table(r.merge([wrap(state(a))], k))
    one = [one] if len(spec) == 1 else list(one)
    for have, x in zip(one, a):
        assert have is not x and have.tobytes() == x.tobytes()
        have += have.dtype.type(1)
    assert all(t.tobytes() == u.tobytes() for t, u in zip(a, before))
