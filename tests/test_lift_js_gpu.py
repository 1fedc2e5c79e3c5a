"""The option lift: 'centred' of the Node.js shim (ntru-circom_amd/js/index.mjs), in a fresh node process: tests/js/shim_lift.mjs."""
import json
import os
import shutil
import subprocess

import pytest

import __graft_entry__ as ge
import lift_ref as ref

NODE = shutil.which("node")


@pytest.mark.gpu
@pytest.mark.skipif(NODE is None, reason="node is not installed")
def test_shim_centred_lift(tmp_path):
    ge.build()
    c = ref.tally_case(7, 6)
    assert abs(c["T"]).max() < c["q"] // 2              # room to count: a correct lift must return the sums
    with open(tmp_path / "tally.json", "w") as fh:
        json.dump({k: (v.tolist() if hasattr(v, "tolist") else v) for k, v in c.items() if k != "T"}, fh)
    r = subprocess.run([NODE, os.path.join(ge.ROOT, "tests", "js", "shim_lift.mjs"), str(tmp_path)], cwd=ge.ROOT, capture_output=True,
                       text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    assert "shim_lift:" in r.stdout
