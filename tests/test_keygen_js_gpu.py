"""Batched key generation of the Node.js shim (tests/js/shim_keygen.mjs): the arrays it dumps are replayed on the CPU oracle, and its
loadKeyFromBatch(...).verifyKeysInputs() equals the Python shim's."""
import json
import os
import shutil
import subprocess

import numpy as np
import pytest

import __graft_entry__ as ge
from test_keygen_gpu import check_against_replay, options, replay

NODE = shutil.which("node")
pkg = ge.load_package()


@pytest.mark.gpu
@pytest.mark.skipif(NODE is None, reason="node is not installed")
@pytest.mark.parametrize("name,B", [("n17_q32", 3000), ("n509_q2048", 700)])
def test_shim_generate_keys_batch(tmp_path, name, B):
    ge.build()
    r = subprocess.run([NODE, os.path.join(ge.ROOT, "tests", "js", "shim_keygen.mjs"), name, str(B), str(tmp_path)], cwd=ge.ROOT,
                       capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    assert "shim_keygen: %d key pairs" % B in r.stdout
    meta = json.load(open(os.path.join(str(tmp_path), "keys.json")))
    N, q = meta["N"], meta["q"]
    load = lambda n, dt, shape: np.fromfile(os.path.join(str(tmp_path), n + ".bin"), dtype=dt).reshape(shape)
    out = {"f": load("f", np.int8, (B, N)), "g": load("g", np.int8, (B, N)), "fq": load("fq", np.uint16, (B, N)),
           "fp": load("fp", np.uint8, (B, N)), "h": load("h", np.uint16, (B, N)), "tries": load("tries", np.uint8, (B,)),
           "flags": load("flags", np.uint8, (B,))}
    o = options(name)
    key = np.array(meta["key"], np.uint32)
    check_against_replay(N, q, out, replay(N, o["df"], o["dg"], key, meta["firstItem"], B, 100))
    from oracle import ntru_oracle as orc
    packed = load("packedH", np.uint64, (B, meta["outputSize"], 4))
    assert np.array_equal(packed, orc.pack_batch(q - 1, N, out["h"]))
    eng = pkg.Engine(0)
    py = pkg.ntru.NTRU(dict(o), engine=eng)
    keys = py.generateKeysBatch(B, key, firstItem=meta["firstItem"])
    for name_ in out:
        assert np.array_equal(keys[name_], out[name_]), name_
    for rec in meta["inputs"]:
        assert py.loadKeyFromBatch(keys, rec["item"]).verifyKeysInputs() == rec["witnesses"]
