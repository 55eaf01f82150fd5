"""One SummarySink asked for every summary at once against four sinks asked for one each, fed the same shards: the window tables and
totals, the k-mer tables, the motif tables and the calibration metrics of the one sink are exactly those of the four -- every array,
every sum, every file byte for byte -- on host shards and on device shards, and the integer sums of the device sink are those of the
host sink.  More than four window sizes and more than four k-mer lengths, so that each goes through more than one call of its entry
point; two chromosomes that arrive against their name order, each in several parts whose rows are shuffled.

Labels that are NaN ("no label") are rows that EVERY summary refuses (status bit 2, raised at close()): with them the sinks have no
result to compare.  So the NaN rows are fed first, to all five sinks, which must raise the same error and leave no file behind; the
equalities are then asserted on the same rows with those few labels set."""
import functools
import os

import numpy as np
import pytest
import torch

WINDOWS = (1000, 64, 500, 250, 128)
KMERS = (1, 3, 5, 7, 9)              # odd: the window of an SNV row around an even length is no k-mer (an empty table has no correlation to write)
MOTIFS = (3, 5)
BINS = 10
N_CLASS = 4
ONE_EACH = {"windows": dict(windows=WINDOWS), "kmers": dict(kmers=KMERS), "motifs": dict(motifs=MOTIFS),
            "calibration": dict(calibration=True, calibration_bins=BINS)}
EVERYTHING = {key: v for opts in ONE_EACH.values() for key, v in opts.items()}
CHROMS = (("chrT", 3100, 1050), ("chr2", 2900, 950))      # arrival order; by name chr2 sorts first


@functools.lru_cache(maxsize=None)
def _data():
    """({chromosome: sequence}, {chromosome: (prob float32 [n][4], start, end, strand uint8, label float32)} in a shuffled row order,
    {chromosome: rows whose label is NaN in the refused variant})."""
    rng = np.random.default_rng(20261019)
    seqs, rows, unlabelled = {}, {}, {}
    for name, length, n in CHROMS:
        seq = rng.choice(list("ACGT"), size=length)
        seq[[70, 71, 1500]] = "N"
        seqs[name] = "".join(seq)
        start = rng.permutation(np.sort(rng.choice(length, size=n, replace=False)).astype(np.int64))
        rest = (10.0 ** rng.uniform(-6, -0.8, size=(n, N_CLASS - 1)) / N_CLASS).astype(np.float32)
        prob = np.concatenate([(1.0 - rest.sum(axis=1, dtype=np.float64)).astype(np.float32)[:, None], rest], axis=1)
        rows[name] = (np.ascontiguousarray(prob), start, start + 1, rng.integers(0, 2, n).astype(np.uint8),
                      rng.integers(0, N_CLASS, n).astype(np.float32))
        unlabelled[name] = rng.choice(n, size=3, replace=False)
    assert sorted(seqs) != list(seqs) and all((p >= 0).all() and (p <= 1).all() for p, *_ in rows.values())
    return seqs, rows, unlabelled


def _shards(part_rows, with_nan=False, device=None):
    """The gathered (unsorted) shards of the data, a chromosome's rows in parts of `part_rows`, the parts not in their order."""
    _, rows, unlabelled = _data()
    up = (lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(device)) if device else (lambda a: a)      # noqa: E731
    for name, (prob, start, end, strand, label) in rows.items():
        if with_nan:
            label = label.copy()
            label[unlabelled[name]] = np.nan
        cuts = list(range(0, len(start), part_rows)) + [len(start)]
        parts = list(zip(cuts[:-1], cuts[1:]))
        assert len(parts) > 1
        for a, b in parts[1:] + parts[:1]:
            yield {"chrom": name, "start": up(start[a:b]), "end": up(end[a:b]), "strand": up(strand[a:b]), "label": up(label[a:b]),
                   "prob": up(prob[a:b]), "n_class": N_CLASS, "calibrated": False}


def _sink(prefix, genome, options, part_rows, with_nan=False, device=None):
    from mural_amd.predict import SummarySink
    sink = SummarySink(prefix, genome=genome, **options)
    for shard in _shards(part_rows, with_nan, device):
        sink(shard)
    return sink


def _files(prefix):
    d, stem = os.path.split(str(prefix))
    return {f[len(stem):]: open(os.path.join(d, f), "rb").read() for f in sorted(os.listdir(d)) if f.startswith(stem + ".")}


def _same_pair(got, want):
    assert got[0] == want[0] and np.array_equal(got[1], want[1])


def _same_metrics(got, want):
    assert set(got) == set(want)
    for key in want:
        if key == "per_chromosome":
            assert list(got[key]) == list(want[key])
            for name in want[key]:
                _same_metrics(got[key][name], want[key][name])
        else:
            assert got[key] == want[key], key


def _check_together(tmp_path, genome, part_rows, device=None):
    """The sink with every option against the four with one each; returns its result, the four sinks' integer sums and the four."""
    from mural_amd import tables
    # rows without a label: refused by all five at close(), and abort() leaves nothing
    for tag, options in dict(ONE_EACH, all=EVERYTHING).items():
        sink = _sink(tmp_path / ("nan_" + tag), genome, options, part_rows, with_nan=True, device=device)
        with pytest.raises(ValueError, match="summary: a mut_type outside 0 .. n_class - 1"):
            sink.close()
        sink.abort()
        assert os.listdir(tmp_path) == []
    one = {tag: _sink(tmp_path / tag, genome, options, part_rows, device=device) for tag, options in ONE_EACH.items()}
    every = _sink(tmp_path / "all", genome, EVERYTHING, part_rows, device=device)
    for sink in list(one.values()) + [every]:
        sink.close()
    res = every.result()
    assert set(res) == {"prob_sum", "n_sites", "windows", "kmers", "motifs", "calibration"}
    n = sum(len(r[1]) for r in _data()[1].values())
    for tag, sink in one.items():                          # the totals are every sink's
        assert sink.rows == every.rows == n
        assert sink.result()["prob_sum"] == res["prob_sum"] and sink.result()["n_sites"] == res["n_sites"] == n
    assert list(res["windows"]) == list(WINDOWS) and list(res["kmers"]) == list(KMERS) and list(res["motifs"]) == list(MOTIFS)
    for W in WINDOWS:
        _same_pair(res["windows"][W], one["windows"].result()["windows"][W])
        assert len(res["windows"][W][0]) > 2 and {c for c, _ in res["windows"][W][0]} == {"chrT", "chr2"}
    for k in KMERS:
        _same_pair(res["kmers"][k], one["kmers"].result()["kmers"][k])
        for a, b in zip(every.kmer_sums()[k], one["kmers"].kmer_sums()[k]):
            assert np.array_equal(a, b)
        assert len(res["kmers"][k][0]) == min(4 ** k, len(res["kmers"][k][0])) > 3
    for m in MOTIFS:
        _same_pair(res["motifs"][m], one["motifs"].result()["motifs"][m])
        for a, b in zip(every.motif_sums()[m], one["motifs"].motif_sums()[m]):
            assert np.array_equal(a, b)
    _same_metrics(res["calibration"], one["calibration"].result()["calibration"])
    assert res["calibration"]["rows"] == n and list(res["calibration"]["per_chromosome"]) == ["chr2", "chrT"]
    got, want = every.calibration_sums(), one["calibration"].calibration_sums()
    assert np.array_equal(got["all"], want["all"]) and list(got["per_chromosome"]) == list(want["per_chromosome"])
    assert all(np.array_equal(got["per_chromosome"][c], want["per_chromosome"][c]) for c in want["per_chromosome"])
    # the files: those of the one sink are those of the four, byte for byte
    files = _files(tmp_path / "all")
    names = [n for W in WINDOWS for n in tables.regional_output_names("", W)[:2]] + [n for k in KMERS for n in tables.kmer_output_names("", k)]
    names += [n for m in MOTIFS for n in tables.motif_output_names("", m)] + [".calibration.txt"]
    assert set(files) == set(names) and len(files) == 2 * (2 + len(KMERS) + len(MOTIFS)) + 1      # (the sizes below 1000 share the name 0Kb)
    singles = {}
    for tag in one:
        singles.update(_files(tmp_path / tag))
    assert files == singles
    # abort() on the closed sink removes every file it wrote (and no other sink's)
    every.abort()
    assert _files(tmp_path / "all") == {} and all(_files(tmp_path / tag) for tag in one)
    with pytest.raises(RuntimeError):
        every.result()
    return res, {"kmers": one["kmers"].kmer_sums(), "motifs": one["motifs"].motif_sums(), "calibration": want}, one


def test_host_sink_with_every_summary_equals_four_sinks(tmp_path):
    seqs, rows, _ = _data()
    assert all(len(r[1]) // 3 + 1 < len(r[1]) for r in rows.values())
    _check_together(tmp_path, seqs.__getitem__, 350)      # 3 shards per chromosome


@pytest.mark.gpu
def test_device_sink_with_every_summary_equals_four_sinks_and_the_host_sink(tmp_path):
    from mural_amd.data.genome import PackedGenome
    from tests.test_gpu_summary import RTOL, _same_tables, _sink_tables
    seqs, _, _ = _data()
    dev = torch.device("cuda", torch.cuda.current_device())
    packed = {name: PackedGenome.from_sequence(seq, dev) for name, seq in seqs.items()}
    res, sums, _ = _check_together(tmp_path, packed.__getitem__, 700, device=dev)
    host = _sink(None, seqs.__getitem__, EVERYTHING, 350)
    host.close()
    for k in KMERS:
        for a, b in zip(sums["kmers"][k], host.kmer_sums()[k]):
            assert np.array_equal(a, b), k
    for m in MOTIFS:
        for a, b in zip(sums["motifs"][m], host.motif_sums()[m]):
            assert np.array_equal(a, b), m
    want = host.calibration_sums()
    # the calibration sums: device and twin agree exactly in what no transcendental's last bit decides (rows, inf_rows, label counts);
    # the score sums go through log and exp of two math libraries (summary_calib_host's docstring: 8 of the 66 cells differ here, the
    # metrics by up to 5.1e-7), so they are held to the figure tests/test_gpu_summary_calib.py holds device and twin to, 2e-6 absolute
    head = 2 + N_CLASS
    for got_t, want_t in [(sums["calibration"]["all"], want["all"])] + [(sums["calibration"]["per_chromosome"][c], t)
                                                                         for c, t in want["per_chromosome"].items()]:
        assert np.array_equal(got_t[:head], want_t[:head])
    four = lambda m: np.array([m[key] for key in ("nll", "ece", "c_ece", "brier")])      # noqa: E731
    print("calibration cells that differ between device and host:", int((sums["calibration"]["all"] != want["all"]).sum()),
          "metrics", four(res["calibration"]), four(host.result()["calibration"]))
    assert np.abs(four(res["calibration"]) - four(host.result()["calibration"])).max() <= 2e-6
    href = host.result()
    assert res["n_sites"] == href["n_sites"] and abs(res["prob_sum"] - href["prob_sum"]) <= RTOL * href["prob_sum"]
    assert [keys for keys, _ in res["windows"].values()] == [keys for keys, _ in href["windows"].values()]
    _same_tables(_sink_tables(res, N_CLASS), _sink_tables(href, N_CLASS), N_CLASS)
