"""The epoch loader's entry point in the PRODUCT library (the suite itself runs on the debug flavour, tests/conftest.py)."""
import os
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_both_flavours_export_the_batch_encoder():
    from mural_amd import _lib
    for path in (_lib.LIB_PATH, _lib.DEBUG_LIB_PATH):
        out = subprocess.run(["nm", "-D", "--defined-only", path], capture_output=True, text=True, check=True).stdout
        assert any(ln.split()[-1] == "mural_train_batch_encode" for ln in out.splitlines() if ln.strip()), path
    assert "mural_train_batch_encode" in _lib.PROTOTYPES


@pytest.mark.gpu
def test_product_library_loader_equals_the_old_route():
    env = {k: v for k, v in os.environ.items() if k != "MURAL_HIP_FLAVOR"}
    out = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "_product_loader_checks.py")], capture_output=True, text=True,
                         timeout=600, env=env, cwd=ROOT)
    assert out.returncode == 0 and "PRODUCT_LOADER_OK" in out.stdout, (out.stdout[-2000:], out.stderr[-4000:])
