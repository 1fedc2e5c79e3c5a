"""Combinations of ciphertexts through the Node.js shim (tests/js/shim_combine.mjs, a fresh process): the reference-captured cases of
tests/golden/combine_cases.json through combineCiphertexts and ntru.combineBatch."""
import os
import shutil
import subprocess

import pytest

import __graft_entry__ as ge

NODE = shutil.which("node")


@pytest.mark.gpu
@pytest.mark.skipif(NODE is None, reason="node is not installed")
def test_shim_combine():
    ge.build()
    r = subprocess.run([NODE, os.path.join(ge.ROOT, "tests", "js", "shim_combine.mjs")], cwd=ge.ROOT, capture_output=True, text=True,
                       timeout=600)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    assert "shim_combine: 2 sets, 12 combinations" in r.stdout
