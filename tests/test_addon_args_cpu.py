"""The native interface of ntru_addon.node, export by export: names, argument counts, what is refused as a TypeError and that a valid
call without an engine says so (tests/js/addon_args.mjs).  No engine is ever used, so the test needs no GPU."""
import os
import shutil
import subprocess

import pytest

import __graft_entry__ as ge

NODE = shutil.which("node")
SCRIPT = os.path.join(ge.ROOT, "tests", "js", "addon_args.mjs")


@pytest.mark.skipif(NODE is None, reason="node is not installed")
def test_addon_argument_checks_without_an_engine():
    ge.build()
    r = subprocess.run([NODE, SCRIPT], cwd=ge.ROOT, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    assert "addon_args: 53 exports" in r.stdout

