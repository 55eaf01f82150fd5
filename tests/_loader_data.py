"""The FASTA + BED fixture of the epoch-loader tests and the comparisons both library flavours run on it (tests/test_gpu_epoch_loader.py
on the debug flavour, tests/_product_loader_checks.py on the product library)."""
import numpy as np
import torch

R_LOCAL, ORDER, R_DISTAL = 4, 3, 110
SEGMENT, SAMPLED, BATCH = 400, 2, 7

# symbol -> dense column, written out independently of the kernels: the bases each MURAL_SYM_* code stands for (A C G T N R Y M S W K B D H V)
_MEMBERS = ["A", "C", "G", "T", "ACGT", "AG", "CT", "AC", "CG", "AT", "GT", "CGT", "AGT", "ACT", "ACG"]
ONEHOT = np.zeros((15, 4), np.float32)
for _s, _m in enumerate(_MEMBERS):
    for _b in _m:
        ONEHOT[_s, "ACGT".index(_b)] = {1: 1.0, 2: 0.5, 3: np.float32(1.0 / 3.0), 4: 0.25}[len(_m)]


def write_fixture(tmp):
    """Two chromosomes of about 3 kb.  chrA has sites within R_DISTAL of both ends (N fill beyond the record); chrB has an N run and three
    non-N IUPAC codes with sites on both strands whose windows hold them.  64 BED rows, segments of 400 bp: several (segment, strand)
    groups per chromosome, and a group of two segments that crosses the chromosome boundary.  Returns (fasta path, bed path)."""
    rng = np.random.default_rng(4242)
    a = rng.choice(np.frombuffer(b"ACGT", np.uint8), size=3011).tobytes().decode()
    b = list(rng.choice(np.frombuffer(b"ACGT", np.uint8), size=2897).tobytes().decode())
    b[1200:1240] = "N" * 40
    b[1500], b[1507], b[1519] = "R", "Y", "B"
    seqs = {"chrA": a, "chrB": "".join(b)}
    fa = tmp / "g.fa"
    fa.write_text("".join(f">{k}\n" + "\n".join(s[i:i + 60] for i in range(0, len(s), 60)) + "\n" for k, s in seqs.items()))
    pos = {"chrA": [0, 3, 57, 109, 110, 111, 3010, 3009, 2950, 2901, 2900, 2899] + list(rng.choice(np.arange(150, 2850), 20, replace=False)),
           "chrB": [2, 1190, 1215, 1245, 1450, 1499, 1500, 1503, 1510, 1519, 1560, 1625, 2896] + list(rng.choice(np.arange(150, 2850), 19, replace=False))}
    rows = []
    for name in ("chrA", "chrB"):
        for p in sorted(set(int(v) for v in pos[name])):
            rows.append((name, p, "+-"[int(rng.integers(0, 2))], int(rng.integers(0, 4))))
    bed = tmp / "s.bed"
    bed.write_text("".join(f"{c}\t{p}\t{p + 1}\t.\t{lab}\t{st}\n" for c, p, st, lab in rows))
    return fa, bed


def old_route(fa, bed, model_type, shuffle, seed):
    from mural_amd.data import ingest
    g = torch.Generator().manual_seed(seed) if shuffle else None
    return list(ingest.train_batches_from_files(fa, bed, BATCH, R_LOCAL, ORDER, R_DISTAL, segment_center=SEGMENT, sampled_segments=SAMPLED,
                                                shuffle=shuffle, generator=g, model_type=model_type))


def make_loader(fa, bed, model_type="snv", dense=False):
    from mural_amd.data import EpochLoader
    return EpochLoader(fa, bed, BATCH, R_LOCAL, ORDER, R_DISTAL, segment_center=SEGMENT, sampled_segments=SAMPLED, model_type=model_type,
                       dense=dense)


def new_route(loader, shuffle, seed):
    g = torch.Generator().manual_seed(seed) if shuffle else None
    return list(loader.epoch(shuffle=shuffle, generator=g))


def expand(sym):
    """uint8 (B, W) symbols -> float32 (B, 4, W) dense windows (numpy)."""
    return np.ascontiguousarray(ONEHOT[sym.cpu().numpy()].transpose(0, 2, 1))


def assert_batches_equal(new, old, dense):
    """Batch for batch: y and cat_x exactly; the distal member exactly (dense), or its one-hot expansion exactly (symbols)."""
    from mural_amd.data import SymbolWindows
    assert len(new) == len(old) and len(new) > 3
    for (y, cont, cat, dist), (y0, cont0, cat0, dist0) in zip(new, old):
        assert y.dtype == torch.float32 and y.shape == y0.shape and y.dim() == 2 and y.shape[1] == 1 and torch.equal(y.cpu(), y0.cpu())
        assert cont.dtype == torch.float64 and cont.shape == cont0.shape and not cont.any()
        assert cat.dtype == torch.int64 and cat.shape == cat0.shape and torch.equal(cat.cpu(), cat0.cpu())
        if dense:
            assert dist.dtype == torch.float32 and dist.shape == dist0.shape
            assert np.array_equal(dist.cpu().numpy().view(np.uint32), dist0.cpu().numpy().view(np.uint32))
        else:
            assert isinstance(dist, SymbolWindows) and dist.sym.dtype == torch.uint8 and dist.sym.shape == (y.shape[0], dist0.shape[2])
            assert int(dist.sym.max()) <= 14
            assert np.array_equal(expand(dist.sym).view(np.uint32), dist0.cpu().numpy().view(np.uint32))
