"""The device step state's entry points in the PRODUCT library (the suite itself runs on the debug flavour, tests/conftest.py)."""
import os
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRIES = ("mural_op_train_state_tick", "mural_op_adam_flat_state")


def test_both_flavours_export_the_step_state_entries_and_link_closed():
    from mural_amd import _lib
    for path in (_lib.LIB_PATH, _lib.DEBUG_LIB_PATH):
        out = subprocess.run(["nm", "-D", "--defined-only", path], capture_output=True, text=True, check=True).stdout
        defined = {ln.split()[-1] for ln in out.splitlines() if ln.strip()}
        assert set(ENTRIES) <= defined, (path, set(ENTRIES) - defined)
    assert set(ENTRIES) <= set(_lib.PROTOTYPES)
    # both link lines refuse undefined symbols, and the new source is one of the objects they link
    make = open(os.path.join(ROOT, "mural_amd", "csrc", "Makefile")).read()
    links = [ln for ln in make.splitlines() if "-shared" in ln]
    assert len(links) == 2 and all("-Wl,--no-undefined" in ln for ln in links)
    srcs = next(ln for ln in make.splitlines() if ln.startswith("SRCS"))
    assert "train_state.hip" in srcs.split()


@pytest.mark.gpu
def test_product_library_steps_adam_on_the_device_state():
    env = {k: v for k, v in os.environ.items() if k != "MURAL_HIP_FLAVOR"}
    out = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "_product_train_state_checks.py")], capture_output=True, text=True,
                         timeout=600, env=env, cwd=ROOT)
    assert out.returncode == 0 and "PRODUCT_TRAIN_STATE_OK" in out.stdout, (out.stdout[-2000:], out.stderr[-4000:])
