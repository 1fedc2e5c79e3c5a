"""Encrypt / decrypt with one key pair per item through the Node.js shim (tests/js/shim_peritem.mjs, a fresh process): its arrays equal the
Python engine's on the same keys and inputs."""
import json
import os
import shutil
import subprocess

import numpy as np
import pytest

import __graft_entry__ as ge

NODE = shutil.which("node")
pkg = ge.load_package()


@pytest.mark.gpu
@pytest.mark.skipif(NODE is None, reason="node is not installed")
@pytest.mark.parametrize("name,B", [("n167_q128", 600), ("n821_q4096", 300)])
def test_shim_batch_per_key(tmp_path, name, B):
    ge.build()
    r = subprocess.run([NODE, os.path.join(ge.ROOT, "tests", "js", "shim_peritem.mjs"), name, str(B), str(tmp_path)], cwd=ge.ROOT,
                       capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    assert "shim_peritem: %d items" % B in r.stdout
    meta = json.load(open(os.path.join(str(tmp_path), "peritem.json")))
    N, q, p = meta["N"], meta["q"], meta["p"]
    load = lambda n, dt: np.fromfile(os.path.join(str(tmp_path), n + ".bin"), dtype=dt).reshape(B, N)
    with open(os.path.join(ge.ROOT, "tests", "golden", "scheme_%s.json" % name)) as fh:
        o = json.load(fh)["options"]
    eng = pkg.Engine(0)
    keys = eng.keygen_batch(N, q, p, o["df"], o["dg"], np.array(meta["key"], np.uint32), B)
    assert not keys["flags"].any()
    rr, m = load("r", np.uint8), load("m", np.uint8)
    e, quot = eng.encrypt_peritem_batch(N, q, keys["h"], rr, m)
    value, q1, r1, q2 = eng.decrypt_peritem_batch(N, q, p, keys["f"], keys["fp"], e)
    for got, want, what in ((load("e", np.uint16), e, "e"), (load("quotientE", np.uint16), quot, "quotientE"),
                            (load("value", np.uint8), value, "value"), (load("quotient1", np.uint16), q1, "quotient1"),
                            (load("remainder1", np.uint16), r1, "remainder1"), (load("quotient2", np.uint8), q2, "quotient2")):
        assert np.array_equal(got, want), what
