"""The INDEL symbol-window training entries in the PRODUCT library (the suite itself runs on the debug flavour, tests/conftest.py)."""
import os
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRIES = ("mural_indel_train_symbols_workspace_bytes", "mural_indel_train_forward_symbols", "mural_indel_train_backward_symbols",
           "mural_op_indel_first_scratch", "mural_op_indel_first_fwd", "mural_op_indel_first_bwd", "mural_op_symbols_to_dense")


def test_both_flavours_export_the_symbol_entries():
    from mural_amd import _lib
    for path in (_lib.LIB_PATH, _lib.DEBUG_LIB_PATH):
        out = subprocess.run(["nm", "-D", "--defined-only", path], capture_output=True, text=True, check=True).stdout
        names = {ln.split()[-1] for ln in out.splitlines() if ln.strip()}
        assert set(ENTRIES) <= names, (path, set(ENTRIES) - names)
    assert set(ENTRIES) <= set(_lib.PROTOTYPES)


def test_epoch_loader_takes_symbols_for_indel_models():
    import inspect
    from mural_amd.data import EpochLoader
    assert "symbols" in inspect.signature(EpochLoader.__init__).parameters


@pytest.mark.gpu
def test_product_library_trains_from_symbol_windows():
    env = {k: v for k, v in os.environ.items() if k != "MURAL_HIP_FLAVOR"}
    out = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "_product_indel_symbols_checks.py")], capture_output=True, text=True,
                         timeout=600, env=env, cwd=ROOT)
    assert out.returncode == 0 and "PRODUCT_INDEL_SYMBOLS_OK" in out.stdout, (out.stdout[-2000:], out.stderr[-4000:])
