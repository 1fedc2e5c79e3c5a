"""reencryptBatch of the Node.js shim (tests/js/shim_mix.mjs, a fresh process): composed from encryptBatch on a zero message and addBatch,
which need the engine and so a GPU, it reproduces every round of tests/golden/mix_cases.json."""
import os
import shutil
import subprocess

import pytest

import __graft_entry__ as ge

NODE = shutil.which("node")


@pytest.mark.gpu
@pytest.mark.skipif(NODE is None, reason="node is not installed")
def test_shim_mix():
    ge.build()
    r = subprocess.run([NODE, os.path.join(ge.ROOT, "tests", "js", "shim_mix.mjs")], cwd=ge.ROOT, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    assert "shim_mix: 18 rounds of 6 cases" in r.stdout
