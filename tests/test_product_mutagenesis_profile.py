"""The mutagenesis-profile entry point in the PRODUCT library (the suite itself runs on the debug flavour, tests/conftest.py)."""
import os
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRIES = ("mural_mutagenesis_profile_window",)


def test_both_flavours_export_the_entry_and_declare_it_once():
    from mural_amd import _lib
    for path in (_lib.LIB_PATH, _lib.DEBUG_LIB_PATH):
        out = subprocess.run(["nm", "-D", "--defined-only", path], capture_output=True, text=True, check=True).stdout
        defined = {ln.split()[-1] for ln in out.splitlines() if ln.strip()}
        assert set(ENTRIES) <= defined, (path, set(ENTRIES) - defined)
    assert set(ENTRIES) <= set(_lib.PROTOTYPES)
    header = open(os.path.join(ROOT, "include", "mural_hip.h")).read()
    for name in ENTRIES:
        assert header.count(f"int {name}(") == 1


def test_the_python_surface_is_there():
    import inspect
    from mural_amd import mutagenesis as M
    want = ["model", "genome", "pos", "strand", "groups", "n_groups", "local_radius", "local_order", "chunk_windows", "distal_radius", "into",
            "timings"]
    assert list(inspect.signature(M.mutagenesis_profile).parameters) == want
    assert list(inspect.signature(M.mutagenesis_profile_host).parameters) == ["ref_logp", "var_logp", "ref_symbols", "group", "first", "table",
                                                                             "status"]
    for name in ("counts", "mean", "mean_abs", "rms", "by_distance", "offsets", "merge", "__iadd__", "all_reduce_", "save", "load"):
        assert callable(getattr(M.MutagenesisProfile, name))


@pytest.mark.gpu
def test_product_library_builds_a_profile():
    """Without MURAL_HIP_FLAVOR, and with stray development switches in the environment: the product library does not read them."""
    env = {k: v for k, v in os.environ.items() if k != "MURAL_HIP_FLAVOR"}
    env.update(MURAL_DEBUG_WS_GUARD="4096", MURAL_DEBUG_S1_ALIAS="1", MURAL_DEBUG_MLP="1")
    out = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "_product_mutagenesis_profile_checks.py")], capture_output=True, text=True,
                         timeout=600, env=env, cwd=ROOT)
    assert out.returncode == 0 and "PRODUCT_MUTAGENESIS_PROFILE_OK" in out.stdout, (out.stdout[-2000:], out.stderr[-4000:])
