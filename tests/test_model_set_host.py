"""Host-side rules of the model-set regions run (mural_amd.predict.ModelSetForward, focal "SET"): what is refused before anything
touches a device, and the C ABI's new declarations.  No GPU here."""
import importlib.util
import os
import re

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_SYMBOLS = ("mural_sites_classify", "mural_rows_split_workspace_bytes", "mural_rows_split", "mural_rows_scatter")


def test_set_keys_are_checked_before_the_members():
    from mural_amd.predict import ModelSetForward
    member = object()                                     # never looked at: the keys are wrong
    with pytest.raises(ValueError, match="unknown site class 'G'"):
        ModelSetForward({"A": member, "G": member})
    with pytest.raises(ValueError, match="unknown site class"):
        ModelSetForward({"cpg": member})
    for other in ("CpG", "nonCpG"):
        with pytest.raises(ValueError, match="'C' serves"):
            ModelSetForward({"C": member, other: member})
    with pytest.raises(ValueError, match="no member"):
        ModelSetForward({})
    with pytest.raises(ValueError, match="no HipShardForward"):
        ModelSetForward({"A": member})


def test_set_selection():
    from mural_amd.data.genome import FOCAL_SET, class_mask, site_selection
    assert site_selection("SET", classes=("A", "CpG")) == (FOCAL_SET, 5) == site_selection("set", classes=5)
    assert site_selection("SET", classes="C") == (FOCAL_SET, 6) and site_selection("SET", classes=["A", "C"]) == (FOCAL_SET, 7)
    assert [class_mask(m) for m in range(1, 8)] == list(range(1, 8)) and class_mask(("nonCpG", "CpG", "C")) == 6
    for kw in (dict(), dict(classes=()), dict(classes=0), dict(classes=8), dict(classes=("A", "T")), dict(classes="cpg"),
               dict(classes=("A",), context="CpG"), dict(classes=True)):
        with pytest.raises(ValueError):
            site_selection("SET", **kw)
    with pytest.raises(ValueError, match="classes= goes with focal 'SET'"):
        site_selection("C", "CpG", classes=4)
    # the single selections are what they were
    assert [site_selection(*s) for s in (("A",), ("C",), ("C", "CpG"), ("C", "nonCpG"), ("ANY",))] == [(0, 0), (1, 0), (1, 1), (1, 2), (2, 0)]


def test_set_and_focal_go_together():
    from mural_amd.predict import ModelSetForward, predict_regions_sharded

    class Plain:
        device = "cuda:0"

        def genome(self, chrom):
            raise AssertionError("refused before a chromosome is asked for")

    with pytest.raises(ValueError, match="focal 'SET'"):
        predict_regions_sharded(Plain(), {"chr1": [(0, 10)]}, "SET")
    a_set = ModelSetForward.__new__(ModelSetForward)      # (a real one needs a device; the driver looks at its type first)
    a_set.classes, a_set.device = 7, "cuda:0"
    for focal, context in (("A", "all"), ("C", "CpG"), ("ANY", "all")):
        with pytest.raises(ValueError, match="ModelSetForward"):
            predict_regions_sharded(a_set, {"chr1": [(0, 10)]}, focal, context)
    with pytest.raises(ValueError):
        predict_regions_sharded(a_set, {"chr1": [(0, 10)]}, "SET", model_type="indel")


@pytest.fixture(scope="module")
def cli():
    spec = importlib.util.spec_from_file_location("predict_files", os.path.join(ROOT, "tools", "predict_files.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def test_command_line_refusals(cli):
    pairs = ["A=/nowhere/a", "nonCpG=/nowhere/n", "CpG=/nowhere/c"]
    base = ["g.fa", "out.tsv", "--regions", "chr1", "--model_set"] + pairs
    for argv, msg in [
        (base + ["--summary", "pre", "--window_size", "1000"], "--summary"),
        (base + ["--genomewide_mu", "1e-8", "--m_proportion", "0.3"], "--summary"),
        (base + ["--scale_factor", "2"], "--scale_factors"),
        (["model"] + base, "MODEL"),
        (base + ["--model_path", "model"], "MODEL"),
        (["g.fa", "out.tsv", "--model_set"] + pairs, "--regions"),
        (["g.fa", "sites.bed", "out.tsv", "--model_set"] + pairs, "MODEL"),
        (base[:5] + ["A:/nowhere/a"], None),
        (base[:5] + ["T=/nowhere/t"], "CLASS=VALUE"),
        (base[:5] + ["A=/nowhere/a", "A=/nowhere/b"], "twice"),
        (base[:5] + ["A="], "CLASS=VALUE"),
        (base[:5] + ["C=/nowhere/c", "CpG=/nowhere/d"], "C serves"),
        (base + ["--focal", "A"], "--focal"),
        (base + ["--indel"], "--indel"),
        (base + ["--scale_factors", "C=2"], "no model"),
        (base + ["--scale_factors", "A=two"], "bad value"),
        (["model", "g.fa", "out.tsv", "--regions", "chr1", "--scale_factors", "A=2"], "--model_set"),
    ]:
        with pytest.raises(SystemExit) as e:
            cli.main(argv)
        assert e.value.code not in (None, 0), argv
        if msg is not None:
            assert msg in str(e.value.code), (argv, e.value.code)


def test_new_entry_points_are_declared_once_and_bound():
    from mural_amd import _lib
    header = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "mural_hip.h")).read(), flags=re.S)
    for name in NEW_SYMBOLS:
        assert len(re.findall(r"\b%s\s*\(" % name, header)) == 1, name
        assert name in _lib.PROTOTYPES
    for const in ("MURAL_FOCAL_SET = 3", "MURAL_CLASS_A = 1", "MURAL_CLASS_NONCPG = 2", "MURAL_CLASS_CPG = 4", "MURAL_ROW_CLASS_NONE = 255"):
        assert const in header, const
    assert "MURAL_FOCAL_A = 0, MURAL_FOCAL_C = 1, MURAL_FOCAL_ANY = 2" in header      # the existing codes keep their values
    sites = open(os.path.join(ROOT, "mural_amd", "csrc", "sites.hip")).read()
    for name in NEW_SYMBOLS:
        assert len(re.findall(r'extern "C" [a-z_0-9]+ %s\(' % name, sites)) == 1, name
    lib = _lib.lib()
    assert lib.mural_rows_split_workspace_bytes(0, 3) == 8 and lib.mural_rows_split_workspace_bytes(257, 3) == (4 * 2 + 1) * 8
    assert lib.mural_rows_split_workspace_bytes(10, 0) == 0 and lib.mural_rows_split_workspace_bytes(10, 9) == 0
