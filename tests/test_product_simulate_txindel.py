"""The INDEL structure simulation's entry points in the PRODUCT library (the suite itself runs on the debug flavour, tests/conftest.py)."""
import os
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRIES = ("mural_simulate_txindel_rows", "mural_simulate_txindel_workspace_bytes")


def test_both_flavours_export_the_entries_declared_once_and_the_source_is_linked():
    from mural_amd import _lib
    for path in (_lib.LIB_PATH, _lib.DEBUG_LIB_PATH):
        out = subprocess.run(["nm", "-D", "--defined-only", path], capture_output=True, text=True, check=True).stdout
        defined = {ln.split()[-1] for ln in out.splitlines() if ln.strip()}
        assert set(ENTRIES) <= defined, (path, set(ENTRIES) - defined)
    assert set(ENTRIES) <= set(_lib.PROTOTYPES)
    make = open(os.path.join(ROOT, "mural_amd", "csrc", "Makefile")).read()
    srcs = next(ln for ln in make.splitlines() if ln.startswith("SRCS"))
    reported = next(ln for ln in make.splitlines() if ln.startswith("REPORTED"))
    assert "simulate_txindel.hip" in srcs.split() and "simulate_txindel" in reported.split()
    header = open(os.path.join(ROOT, "include", "mural_hip.h")).read()
    assert header.count("int mural_simulate_txindel_rows(") == 1 and header.count("size_t mural_simulate_txindel_workspace_bytes(") == 1
    # the bin rule lives in one header that both kernel files include
    for name in ("summary_txindel.hip", "simulate_txindel.hip"):
        text = open(os.path.join(ROOT, "mural_amd", "csrc", name)).read()
        assert '#include "txindel_bins.h"' in text and "struct TiItem" not in text


@pytest.mark.gpu
def test_product_library_simulates_the_indel_structure_table():
    """Without MURAL_HIP_FLAVOR, and with stray development switches in the environment: the product library does not read them."""
    env = {k: v for k, v in os.environ.items() if k != "MURAL_HIP_FLAVOR"}
    env.update(MURAL_DEBUG_WS_GUARD="4096", MURAL_DEBUG_NO_SMALL_BATCH="1", STI_UNIT_BLOCKS="1")
    out = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "_product_simulate_txindel_checks.py")], capture_output=True, text=True,
                         timeout=600, env=env, cwd=ROOT)
    assert out.returncode == 0 and "PRODUCT_SIMULATE_TXINDEL_OK" in out.stdout, (out.stdout[-2000:], out.stderr[-4000:])
