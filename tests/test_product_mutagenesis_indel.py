"""The INDEL mutagenesis entry points in the PRODUCT library (the suite itself runs on the debug flavour, tests/conftest.py)."""
import os
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRIES = ("mural_indel_forward_symbols", "mural_encode_subst_symbols", "mural_mutagenesis_rows_window", "mural_mutagenesis_reduce_window",
           "mural_scores_log_softmax")


def test_both_flavours_export_the_entries_and_declare_them_once():
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
    from mural_amd.data import PackedGenome
    from mural_amd.model.model_indel import UNet_Small
    import inspect
    assert callable(getattr(UNet_Small, "forward_symbols", None))
    assert "model_type" in inspect.signature(PackedGenome.encode_subst_windows).parameters


@pytest.mark.gpu
def test_product_library_serves_forward_symbols_and_an_indel_map():
    """Without MURAL_HIP_FLAVOR, and with stray development switches in the environment: the product library does not read them."""
    env = {k: v for k, v in os.environ.items() if k != "MURAL_HIP_FLAVOR"}
    env.update(MURAL_DEBUG_WS_GUARD="4096", MURAL_INDEL_DENSE_SYMBOLS="0", MURAL_INDEL_CHUNK="256")
    out = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "_product_mutagenesis_indel_checks.py")], capture_output=True, text=True,
                         timeout=600, env=env, cwd=ROOT)
    assert out.returncode == 0 and "PRODUCT_MUTAGENESIS_INDEL_OK" in out.stdout, (out.stdout[-2000:], out.stderr[-4000:])


def test_symbols_instances_of_the_first_level_do_not_spill():
    """indel_enc0_kernel<13 | 7, .., BYTES, SYMS> (csrc/indel_level0_symbols.hip), the launches of mural_indel_forward_symbols: as the
    instances of the other entries (tests/test_build_resources.py) -- no spill, no scratch, at least four waves per SIMD."""
    from tests.test_build_resources import _kernels, _report
    ks = _kernels(_report("indel_level0_symbols"))
    run = [k for k in ks if "indel_enc0_kernel" in k]
    assert len(run) == 4 and all(k.split("indel_enc0_kernel")[1].startswith(("ILi13ELb0E", "ILi7ELb0E")) for k in run), sorted(ks)
    for k in run:
        r = ks[k]
        assert r["VGPRs Spill"] == 0 and r["SGPRs Spill"] == 0 and r["ScratchSize"] == 0 and r["Occupancy"] >= 4, (k, r)
