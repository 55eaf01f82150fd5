"""The allele entry points in the PRODUCT library (the suite itself runs on the debug flavour, tests/conftest.py)."""
import os
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRIES = ("mural_encode_allele_windows", "mural_allele_rows")


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
    import inspect
    from mural_amd import mutagenesis as M
    from mural_amd.data import PackedGenome
    assert list(inspect.signature(PackedGenome.encode_allele_windows).parameters)[1:] == [
        "pos", "strand", "allele", "alleles", "radius", "local_radius", "local_order", "model_type"]
    assert list(inspect.signature(M.allele_footprint).parameters)[:8] == [
        "model", "genome", "alleles", "strand", "local_radius", "local_order", "chunk_windows", "distal_radius"]
    for name in ("Alleles", "alternate_sequence", "encode_allele_windows_host", "allele_rows_host", "allele_footprint_offsets"):
        assert hasattr(M, name)


@pytest.mark.gpu
def test_product_library_serves_an_allele_footprint():
    """Without MURAL_HIP_FLAVOR, and with stray development switches in the environment: the product library does not read them."""
    env = {k: v for k, v in os.environ.items() if k != "MURAL_HIP_FLAVOR"}
    env.update(MURAL_DEBUG_WS_GUARD="4096", MURAL_INDEL_DENSE_SYMBOLS="0", MURAL_INDEL_CHUNK="256")
    out = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "_product_alleles_checks.py")], capture_output=True, text=True,
                         timeout=600, env=env, cwd=ROOT)
    assert out.returncode == 0 and "PRODUCT_ALLELES_OK" in out.stdout, (out.stdout[-2000:], out.stderr[-4000:])
