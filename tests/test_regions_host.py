"""Host logic of prediction over regions (mural_amd.predict.read_regions_arg and the ranks' slices of a chromosome's enumeration):
no device needed."""
import gzip

import numpy as np
import pytest

from mural_amd.predict import REGION_END, _region_pieces, read_regions_arg, shard_bounds


def test_region_specs_parse_merge_and_sort(tmp_path):
    assert read_regions_arg("chr7") == {"chr7": [(0, REGION_END)]}
    assert read_regions_arg("chr7:101-200") == {"chr7": [(100, 200)]}                  # 1-based inclusive -> 0-based half-open
    assert read_regions_arg("HLA-A*01:01:5-9") == {"HLA-A*01:01": [(4, 9)]}            # the LAST colon splits name and range
    # overlapping and touching regions merge, the rest is sorted; a list of arguments is one region set
    got = read_regions_arg(["chr2:501-600", "chr1:301-400", "chr1:1-100", "chr1:51-150", "chr1:151-200", "chr1:202-210"])
    assert got == {"chr2": [(500, 600)], "chr1": [(0, 200), (201, 210), (300, 400)]}
    assert read_regions_arg(["chr1:5-9", "chr1"]) == {"chr1": [(0, REGION_END)]}
    bed = tmp_path / "regions.bed"
    bed.write_text("# comment\ntrack name=x\nchrB\t100\t200\tname\t0\t+\nchrA\t50\t60\nchrB\t150\t300\nchrB\t300\t310\nchrB\t400\t400\n")
    want = {"chrB": [(100, 310)], "chrA": [(50, 60)]}
    assert read_regions_arg(str(bed)) == want and read_regions_arg(bed) == want
    with gzip.open(tmp_path / "regions.bed.gz", "wt") as fh:
        fh.write(bed.read_text())
    assert read_regions_arg(str(tmp_path / "regions.bed.gz")) == want
    assert read_regions_arg([str(bed), "chrA:1-55"]) == {"chrB": [(100, 310)], "chrA": [(0, 60)]}


@pytest.mark.parametrize("spec", ["chr:5-2", "chr:0-7", "chr:a-b", "chr:12-", "chr:-5", ":1-5", "chr:1-5x", "chr:1,000-2,000", ""])
def test_malformed_region_specs_name_the_spec(spec):
    with pytest.raises(ValueError) as e:
        read_regions_arg(spec)
    assert repr(spec) in str(e.value)


def test_malformed_region_files_name_the_file(tmp_path):
    empty = tmp_path / "empty.bed"
    empty.write_text("# nothing here\n\n")
    short = tmp_path / "short.bed"
    short.write_text("chr1\t5\n")
    text = tmp_path / "text.bed"
    text.write_text("chr1\tfive\t9\n")
    backwards = tmp_path / "backwards.bed"
    backwards.write_text("chr1\t9\t5\n")
    for path in (empty, short, text, backwards):
        with pytest.raises(ValueError) as e:
            read_regions_arg(str(path))
        assert str(path) in str(e.value), path


@pytest.mark.parametrize("world", [1, 3, 4])
def test_rank_slices_tile_every_region_of_a_chromosome(world):
    """Rank i of N takes shard_bounds(total, i, N) of a chromosome's enumeration, in parts: over all ranks and parts the pieces cover
    every region's enumeration exactly once, in order -- for totals of 0, 1, world - 1 and more, and regions without a site."""
    cases = [[0], [1], [world - 1], [world], [0, 0], [0, 1, 0], [2, 0, world - 1, 0, 5], [7, 1, 1, 9], [world - 1, 0, 1]]
    for totals in cases:
        cum = np.r_[0, np.cumsum(totals)].astype(np.int64)
        n = int(cum[-1])
        seen = [[] for _ in totals]
        for rank in range(world):
            b0, b1 = shard_bounds(n, rank, world)
            assert b1 - b0 in (n // world, n // world + 1)
            for parts in (1, 2):
                rows = 0
                for part in range(parts):
                    p0, p1 = shard_bounds(b1 - b0, part, parts)
                    pieces = _region_pieces(cum, b0 + p0, b0 + p1)
                    assert sum(m for _, _, m in pieces) == p1 - p0 and all(m > 0 for _, _, m in pieces)
                    assert [j for j, _, _ in pieces] == sorted(j for j, _, _ in pieces)
                    rows += p1 - p0
                    if parts == 2:
                        for j, first, m in pieces:
                            seen[j] += list(range(first, first + m))
                assert rows == b1 - b0
        assert seen == [list(range(t)) for t in totals], totals
    assert _region_pieces(np.array([0, 4, 9]), 3, 3) == []
    assert _region_pieces(np.array([0, 4, 9]), 3, 6) == [(0, 3, 1), (1, 0, 2)]
