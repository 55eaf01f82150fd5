"""Host and device parts mixed in one SummarySink, for every reducer built on ``summaries._TableReducer``: the tables are integer sums
over the SET of rows, so a run fed entirely with host shards, a run whose first chromosome arrives on the device and a run after
``abort()`` all give the same ``result()`` and the same integer tables, exactly.  This is the read-back that adds host and device
tables, and ``reset``."""
import io

import numpy as np
import pytest
import torch

from tests import _conseq_data as D
from tests.test_gpu_summary_conseq import _dev, _up

pytestmark = pytest.mark.gpu

N_ROWS, LENGTH, N_REP = 100, 160, 5
# three transcripts on two chromosomes; chr3 has rows and no transcript or name
BED12 = "\n".join([D.bed12("chr1", "plus", "+", [(10, 40), (60, 90), (110, 140)], (20, 130)),
                   D.bed12("chr1", "minus", "-", [(30, 70), (100, 150)], (35, 120)),
                   D.bed12("chr2", "other", "+", [(5, 50), (80, 120)], (9, 99))]) + "\n"
ANNOTATIONS = {"chr1": [(0, 50, "a"), (40, 120, "b"), (130, 131, "c")], "chr2": [(20, 90, "b"), (0, 160, "c")]}

# reducer -> (the sink's keywords, INDEL rows?, the accessors of the integer tables)
CASES = {
    "annotations": (dict(annotations=ANNOTATIONS), False, ["annotation_sums"]),
    "consequences": (dict(transcripts=BED12), False, ["consequence_sums"]),
    "transcript_structure": (dict(transcripts=BED12, transcript_structure=True), False, ["consequence_sums", "structure_sums"]),
    "indel_structure": (dict(indel_transcripts=BED12, indel_kind="deletion_start"), True, ["indel_structure_sums"]),
    "simulation": (dict(annotations=ANNOTATIONS, simulate=N_REP, simulate_seed=7), False, ["annotation_sums", "simulation_counts"]),
    "consequence_simulation": (dict(transcripts=BED12, simulate=N_REP, simulate_seed=7, simulate_transcripts=True), False,
                               ["consequence_sums", "consequence_simulation_counts"]),
    "structure_simulation": (dict(transcripts=BED12, transcript_structure=True, simulate=N_REP, simulate_seed=7, simulate_transcripts=True,
                                  simulate_structure=True), False,
                             ["structure_sums", "consequence_simulation_counts", "structure_simulation_counts"]),
    "indel_structure_simulation": (dict(indel_transcripts=BED12, indel_kind="insertion", simulate=N_REP, simulate_seed=7,
                                        simulate_indel_structure=True), True,
                                   ["indel_structure_sums", "indel_structure_simulation_counts"]),
}


@pytest.fixture(scope="module")
def genomes():
    from mural_amd.data import PackedGenome
    rng = np.random.default_rng(5)
    return {name: PackedGenome.from_sequence("".join(rng.choice(list("ACGT"), size=LENGTH)), _dev()) for name in ("chr1", "chr2", "chr3")}


def _shards(k):
    """{chromosome: the shard of its N_ROWS rows on the host}, ascending in start with equal starts."""
    out = {}
    for j, name in enumerate(("chr1", "chr2", "chr3")):
        rng = np.random.default_rng(40 + j)
        start = np.sort(rng.integers(0, LENGTH - 1, size=N_ROWS)).astype(np.int64)
        out[name] = {"chrom": name, "start": start, "end": start + 1, "strand": rng.integers(0, 2, size=N_ROWS).astype(np.uint8),
                     "label": rng.integers(0, k, size=N_ROWS).astype(np.float32), "prob": rng.dirichlet(np.ones(k), size=N_ROWS).astype(np.float32),
                     "n_class": k, "calibrated": False, "aligned": True}
    return out


def _flat(x):
    """The arrays in a result or a table accessor's value, in order, as bytes; everything else as it is."""
    if isinstance(x, np.ndarray):
        return [(x.dtype.str, x.shape, x.tobytes())]
    if isinstance(x, dict):
        return [item for key in sorted(x, key=str) for item in [key] + _flat(x[key])]
    if isinstance(x, (list, tuple)):
        return [item for v in x for item in _flat(v)]
    return [x]


@pytest.mark.parametrize("reducer", sorted(CASES))
def test_host_and_device_parts_add_up_and_abort_starts_over(genomes, reducer):
    from mural_amd.predict import SummarySink
    kw, indel, accessors = CASES[reducer]
    shards = _shards(8 if indel else 4)
    on_device = {name: {key: _up(v) if isinstance(v, np.ndarray) else v for key, v in shard.items()} for name, shard in shards.items()}
    sink = SummarySink(None, genome=genomes.__getitem__, **{key: io.StringIO(v) if v is BED12 else v for key, v in kw.items()})
    assert reducer in sink._reducers
    mine = [name for name in sink._reducers if name != "windows"]      # (the window totals are floating-point sums)

    def run(device):
        for name in ("chr1", "chr2", "chr3"):
            sink((on_device if name in device else shards)[name])
        mixed = bool(sink._reducers[reducer].dev) and sink._reducers[reducer].host is not None
        sink.close()
        return _flat([sink.result()[name] for name in mine]) + [item for get in accessors for item in _flat(getattr(sink, get)())], mixed

    host, mixed = run(())
    assert not mixed and not sink._reducers[reducer].dev
    tables = getattr(sink, accessors[-1])()
    assert (tables[0] if isinstance(tables, tuple) else tables).any()
    sink.abort()
    both, mixed = run(("chr1", "chr3"))
    assert mixed and both == host
    sink.abort()
    assert sink._reducers[reducer].host is None and not sink._reducers[reducer].dev
    again, _ = run(())
    assert again == host
    torch.cuda.synchronize()
