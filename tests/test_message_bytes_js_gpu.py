"""Byte messages through the Node.js shim (tests/js/shim_bytes.mjs, a fresh process): the reference-captured messages with the recorded r,
and one batch whose ciphertexts, bytes and flags equal the Python engine's for the same inputs."""
import json
import os
import shutil
import subprocess

import numpy as np
import pytest

import __graft_entry__ as ge
import message_bytes_ref as ref

NODE = shutil.which("node")
pkg = ge.load_package()


@pytest.mark.gpu
@pytest.mark.skipif(NODE is None, reason="node is not installed")
def test_shim_bytes(tmp_path):
    ge.build()
    s = [x for x in ref.load_sets() if x["set"] == "n509_q2048"][0]
    N, q, p, W, h, f, fp = ref.set_key(s)
    g = np.random.default_rng(21)
    length = 40 * W - 5
    blocks = 40
    data = g.integers(0, 256, length, dtype=np.uint8)
    dr = s["options"]["dr"]
    r = np.zeros((blocks, N), np.uint8)
    r[:, :dr], r[:, dr:2 * dr] = 1, 2
    r = g.permuted(r, axis=1)
    eng = pkg.Engine(0)
    ntru = pkg.NTRU(dict(s["options"], f=s["key"]["f"], fp=s["key"]["fp"], h=s["key"]["h"]), engine=eng)
    e = ntru.encryptBytes(data.tobytes(), r=r)
    e_mixed = e.copy()
    e_mixed[::9] = g.integers(0, q, e_mixed[::9].shape, dtype=np.uint16)          # rows of noise: flagged blocks
    out, flags = eng.decrypt_bytes_batch(N, q, p, W, f, fp, e_mixed)
    assert flags[::9].all() and not np.delete(flags, np.arange(0, blocks, 9)).any()
    assert ntru.decryptBytes(e, length=length)[0] == data.tobytes()
    for name, a in (("data", data), ("r", r), ("h", h), ("f", f), ("fp", fp), ("e", e), ("e_mixed", e_mixed), ("out", out), ("flags", flags)):
        np.ascontiguousarray(a).tofile(os.path.join(str(tmp_path), name + ".bin"))
    with open(os.path.join(str(tmp_path), "bytes.json"), "w") as fh:
        json.dump({"options": s["options"], "blocks": blocks, "length": length}, fh)
    del ntru, eng
    r_ = subprocess.run([NODE, os.path.join(ge.ROOT, "tests", "js", "shim_bytes.mjs"), str(tmp_path)], cwd=ge.ROOT, capture_output=True,
                        text=True, timeout=600)
    assert r_.returncode == 0, r_.stdout[-3000:] + r_.stderr[-3000:]
    assert "shim_bytes: " in r_.stdout and "batch of %d blocks" % blocks in r_.stdout
