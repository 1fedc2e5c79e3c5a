"""checkWitnesses of the Node.js shim (ntru-circom_amd/js): golden witnesses, mutations and malformed input (tests/js/shim_check.mjs)."""
import os
import shutil
import subprocess

import pytest

import __graft_entry__ as ge

NODE = shutil.which("node")


@pytest.mark.gpu
@pytest.mark.skipif(NODE is None, reason="node is not installed")
def test_shim_check_witnesses():
    ge.build()
    r = subprocess.run([NODE, os.path.join(ge.ROOT, "tests", "js", "shim_check.mjs")], cwd=ge.ROOT, capture_output=True, text=True,
                       timeout=600)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    assert "shim_check: 178 golden witnesses accepted" in r.stdout
