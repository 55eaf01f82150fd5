"""The mutagenesis entry points in the PRODUCT library (the suite itself runs on the debug flavour, tests/conftest.py)."""
import os
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRIES = ("mural_encode_subst_windows", "mural_mutagenesis_rows", "mural_mutagenesis_reduce")


def test_both_flavours_export_the_mutagenesis_entries_and_the_source_is_linked():
    from mural_amd import _lib
    for path in (_lib.LIB_PATH, _lib.DEBUG_LIB_PATH):
        out = subprocess.run(["nm", "-D", "--defined-only", path], capture_output=True, text=True, check=True).stdout
        defined = {ln.split()[-1] for ln in out.splitlines() if ln.strip()}
        assert set(ENTRIES) <= defined, (path, set(ENTRIES) - defined)
    assert set(ENTRIES) <= set(_lib.PROTOTYPES)
    make = open(os.path.join(ROOT, "mural_amd", "csrc", "Makefile")).read()
    srcs = next(ln for ln in make.splitlines() if ln.startswith("SRCS"))
    assert "mutagenesis.hip" in srcs.split()
    header = open(os.path.join(ROOT, "include", "mural_hip.h")).read()
    for name in ENTRIES:
        assert header.count(f"int {name}(") == 1                                       # declared once
    # the window rules live in ONE place: both encoders read columns through csrc/encode_window.h
    for src in ("encode.hip", "mutagenesis.hip"):
        assert '#include "encode_window.h"' in open(os.path.join(ROOT, "mural_amd", "csrc", src)).read()


@pytest.mark.gpu
def test_product_library_encodes_substitutions_and_builds_a_map():
    """Without MURAL_HIP_FLAVOR, and with stray development switches in the environment: the product library does not read them."""
    env = {k: v for k, v in os.environ.items() if k != "MURAL_HIP_FLAVOR"}
    env.update(MURAL_DEBUG_WS_GUARD="4096", MURAL_DEBUG_S1_ALIAS="1", MURAL_DEBUG_MLP="1")
    out = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "_product_mutagenesis_checks.py")], capture_output=True, text=True,
                         timeout=600, env=env, cwd=ROOT)
    assert out.returncode == 0 and "PRODUCT_MUTAGENESIS_OK" in out.stdout, (out.stdout[-2000:], out.stderr[-4000:])
