"""The numpy twin of the k-mer summary (mural_amd.predict.summary_kmer_host, the specification of csrc/summary_kmer.hip) and the host
path of SummarySink(kmers=...): against a row-by-row brute force with exact rational sums, against the table tools' key and order rule,
and across torch.distributed ranks (gloo).  No device."""
import os
import socket

import numpy as np
import pytest
import torch.distributed as dist
import torch.multiprocessing as mp

from tests import _summary_kmer_data as D

MODES = [(False, 0), (True, 1), (True, 2), (True, 3)]      # SNV rows by their own strand; INDEL rows '+', '-', both


@pytest.mark.parametrize("indel,mode", MODES)
@pytest.mark.parametrize("n_class,dtype", [(2, np.float32), (4, np.float64), (8, np.float32)])
def test_host_twin_equals_the_brute_force_exactly(n_class, dtype, indel, mode):
    from mural_amd.predict import summary_kmer_host
    for n, kind in D.CASES:
        if kind == "sites" and (indel or n_class != 4):
            continue
        prob, start, end, strand, label = D.case(n, kind, n_class, dtype, indel)
        got, status = summary_kmer_host(D.SEQ, prob, start, end, strand, label, n_class, D.KMERS, indel, mode, order_base=5 << 40)
        want = D.brute_force(prob, start, end, strand, label, n_class, D.KMERS, indel, mode, order_base=5 << 40)
        assert status == 0
        for k in D.KMERS:
            mine = D.sums_as_dict(*got[k], k)
            assert list(mine) == list(want[k]), (n, k)                 # names and their order
            assert mine == want[k], (n, k)                             # counts, exact sums, first appearance
            assert (got[k][0][:, 2] < (1 << 40)).all()                 # folded
        if kind == "sites":
            assert 1900 < len(start) < 2200 and len(want[7]) > 1000
        if n == 2049 and not indel:                                    # the fixture does what it promises
            assert D.brute_keys(0, 1, False, 3, False) is None and D.brute_keys(1, 2, False, 3, False) is not None
            assert D.brute_keys(D.L - 1, D.L, False, 3, False) is None and D.brute_keys(D.L - 2, D.L - 1, False, 3, False) is not None
            assert D.brute_keys(2, 3, False, 7, False) is None and D.brute_keys(2, 3, False, 5, False) is not None
            assert D.brute_keys(200, 201, False, 3, False) is None and D.brute_keys(300, 301, False, 3, False) is not None
            assert D.brute_keys(300, 301, False, 5, False) is None and D.brute_keys(400, 401, False, 5, False) is not None
            assert D.brute_keys(400, 401, False, 7, False) is None and D.brute_keys(499, 500, False, 1, False) is not None
            assert D.brute_keys(499, 500, False, 3, False) is None and (start == D.DUPLICATE).sum() == 3
            rows_of = {k: sum(sum(c[0]) for c in want[k].values()) for k in D.KMERS}
            assert n > rows_of[1] > rows_of[3] > rows_of[5] > rows_of[7] > 0      # a row without a key for one k counts for the others


def test_names_order_and_counts_follow_the_table_tools_rule():
    """tables.kmer_table orders the k-mers by the file row of their first appearance (key_a before key_b within a row) and names them
    with tables.kmer_name: the same from order_base + 2 * start + sub when the rows ascend in start."""
    from mural_amd import tables
    from mural_amd.predict import kmer_keys_host, kmer_table_from_sums, summary_kmer_host
    for indel, mode in MODES:
        prob, start, end, strand, label = D.rows(2049, 4, np.float32, indel)
        got, _ = summary_kmer_host(D.SEQ, prob, start, end, strand, label, 4, D.KMERS, indel, mode)
        for k in D.KMERS:
            names, table = kmer_table_from_sums(*got[k], k, 4)
            first, counts = {}, {}
            keys = kmer_keys_host(D.SEQ, start, end, strand, k, indel, mode)
            for row in range(len(start)):
                for sub in range(2):
                    key = int(keys[sub][row])
                    if key >= 0:
                        first.setdefault(key, 2 * row + sub)
                        counts.setdefault(key, np.zeros(4))[int(label[row])] += 1
            order = sorted(first, key=first.get)
            assert names == [tables.kmer_name(g, k) for g in order]
            assert np.array_equal(table[:, 1:5], np.array([counts[g] for g in order]))
            assert np.array_equal(table[:, 0], table[:, 1:5].sum(axis=1))
            # the key rule itself, against Python's slice
            for row in range(0, len(start), 7):
                want = D.brute_keys(start[row], end[row], mode == 2 or (mode == 0 and strand[row] != 0), k, indel)
                assert (tables.kmer_name(int(keys[0][row]), k) if keys[0][row] >= 0 else None) == want


def test_bad_rows_set_their_bit_and_stay_out():
    from mural_amd.predict import summary_kmer_host
    prob, start, end, strand, label = D.rows(65, 4, np.float64)
    clean, _ = summary_kmer_host(D.SEQ, prob[1:], start[1:], end[1:], strand[1:], label[1:], 4, (3,))
    for bit, spoil in ((1, lambda: start.__setitem__(0, -1)), (2, lambda: label.__setitem__(0, 4)), (2, lambda: label.__setitem__(0, 0.5)),
                       (8, lambda: prob.__setitem__((0, 1), np.nan)), (8, lambda: prob.__setitem__((0, 1), 1.0000001)),
                       (8, lambda: prob.__setitem__((0, 2), -1e-9))):
        prob, start, end, strand, label = D.rows(65, 4, np.float64)
        spoil()
        got, status = summary_kmer_host(D.SEQ, prob, start, end, strand, label, 4, (3,))
        assert status == bit and np.array_equal(got[3][0], clean[3][0]) and np.array_equal(got[3][1], clean[3][1])


def _host_shard(name, cols, rows=slice(None), aligned=True):
    prob, start, end, strand, label = cols
    shard = {"chrom": name, "start": start[rows], "end": end[rows], "strand": strand[rows], "label": label[rows], "prob": prob[rows],
             "n_class": 4, "calibrated": False}
    if aligned:
        shard["aligned"] = True
    return shard


GENOMES = {"chrK": D.SEQ, "chr2": D.SEQ[::-1]}


def _run_sink(parts, out_prefix=None):
    """Two chromosomes (chrK arrives first, chr2 sorts first) through a host-shard SummarySink."""
    from mural_amd.predict import SummarySink
    sink = SummarySink(out_prefix, kmers=(3, 5, 7), genome=GENOMES.__getitem__, parts=parts)
    cols = D.rows(2049, 4, np.float32)
    if parts:                          # a gathered shard: every rank has all rows and reduces its slice of the sorted ones
        perm = np.random.default_rng(1).permutation(2049)
        sink(_host_shard("chrK", [c[perm] for c in cols], aligned=False))
        sink(_host_shard("chr2", D.at_sites(4, np.float32), aligned=False))
    else:
        for a, b in ((0, 1), (1, 700), (700, 2049)):
            sink(_host_shard("chrK", cols, slice(a, b)))
        sink(_host_shard("chr2", D.at_sites(4, np.float32)))
    sink.close()
    return sink


def _worker(rank, world, port, q):
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
    dist.init_process_group("gloo", rank=rank, world_size=world)
    try:
        sink = _run_sink(parts=True)
        q.put((rank, {k: (t.tobytes(), f.tobytes()) for k, (t, f) in sink.kmer_sums().items()},
               {k: names for k, (names, _) in sink.result()["kmers"].items()}))
    finally:
        dist.destroy_process_group()


def test_host_shards_give_the_same_integers_at_world_1_2_and_3(tmp_path):
    from mural_amd import tables
    from mural_amd.predict import kmer_table_from_sums, summary_kmer_host
    one = _run_sink(parts=False, out_prefix=tmp_path / "k")
    want = {k: (t.tobytes(), f.tobytes()) for k, (t, f) in one.kmer_sums().items()}
    names = {k: v[0] for k, v in one.result()["kmers"].items()}
    # the sink against the twin on each chromosome: chr2 sorts before chrK, as in the written table
    a, _ = summary_kmer_host(GENOMES["chr2"], *D.at_sites(4, np.float32), 4, (3,), order_base=0)
    b, _ = summary_kmer_host(GENOMES["chrK"], *D.rows(2049, 4, np.float32), 4, (3,), order_base=1 << 40)
    both = (a[3][0] + b[3][0], np.minimum(a[3][1], b[3][1]))
    assert kmer_table_from_sums(*both, 3, 4)[0] == names[3]
    assert np.array_equal(one.kmer_sums()[3][0][:, 0], both[0][:, 0])
    for k in (3, 5, 7):                # the files of evaluate --kmer_only
        paths = tables.kmer_output_names(tmp_path / "k", k)
        assert all(os.path.exists(p) for p in paths)
        assert [ln.split("\t")[0] for ln in open(paths[0])][1:] == names[k]
    one.abort()
    assert os.listdir(tmp_path) == []
    ctx = mp.get_context("spawn")
    for world in (2, 3):
        q = ctx.Queue()
        with socket.socket() as s:
            s.bind(("127.0.0.1", 0))
            port = s.getsockname()[1]
        procs = [ctx.Process(target=_worker, args=(r, world, port, q)) for r in range(world)]
        for p in procs:
            p.start()
        res = [q.get(timeout=120) for _ in procs]
        for p in procs:
            p.join(timeout=60)
        for _, sums, order in res:
            assert sums == want and order == names, world


def test_the_sink_needs_a_genome_and_refuses_a_second_calibration():
    from mural_amd.predict import SummarySink
    with pytest.raises(ValueError, match="genome"):
        SummarySink(kmers=(3,))
    with pytest.raises(ValueError, match="kmer_length"):
        SummarySink(kmers=(11,), genome=GENOMES.get)
    with pytest.raises(ValueError, match="calibrated already"):
        SummarySink(poisson=True, kmers=(3,), genome=GENOMES.get)(dict(_host_shard("chrK", D.rows(10, 4, np.float64)), calibrated=True))
    assert "kmers" not in _closed(SummarySink()).result()


def _closed(sink):
    sink.close()
    return sink


def test_write_kmer_outputs_is_what_evaluate_writes(tmp_path):
    """run_kmer_corr_calc writes through write_kmer_outputs: the same bytes from the same table."""
    from mural_amd import tables
    from mural_amd.predict import kmer_table_from_sums, summary_kmer_host
    got, _ = summary_kmer_host(D.SEQ, *D.rows(2049, 4, np.float32), 4, (3,))
    names, table = kmer_table_from_sums(*got[3], 3, 4)
    corrs = tables.write_kmer_outputs(names, table, 4, 3, tmp_path / "a")
    rates, corr = (open(p).read() for p in tables.kmer_output_names(tmp_path / "a", 3))
    head = rates.split("\n")[0].split("\t")
    assert head[0] == "type" and head[-1] == "number_of_all" and len(head) == 1 + 3 * 3 + 1 and len(rates.split("\n")) == len(names) + 2
    assert corr.count("\n") == 3 and corr.startswith("3-mer\t1\t") and [c for c, _ in corrs] == [1, 2, 3]
    first = rates.split("\n")[1].split("\t")
    assert first[0] == names[0] and first[-1] == str(int(table[0, 0])) and float(first[4]) == table[0, 6] / table[0, 0]
