"""Sums of ciphertexts and tallies through the Node.js shim (tests/js/shim_tally.mjs, a fresh process): the reference-captured cases, and
one ragged weighted batch whose results equal the Python engine's."""
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
def test_shim_tally(tmp_path):
    ge.build()
    N, q, p, B = 509, 2048, 3, 5000
    g = np.random.default_rng(12)
    rows = g.integers(0, q, (B, N), dtype=np.uint16)
    weights = g.integers(0, q, B, dtype=np.uint16)
    offsets = np.array([1, 1, 2, 40, 40, 3000, 3001, 4990, 4990], np.int64)
    f, fp = g.integers(-1, 2, N).astype(np.int8), g.integers(0, 3, N).astype(np.uint8)
    eng = pkg.Engine(0)
    total, value, q1, r1, q2 = eng.tally_decrypt_batch(N, q, p, f, fp, rows, offsets=offsets, weights=weights)
    for name, a in (("rows", rows), ("weights", weights), ("offsets", offsets), ("f", f), ("fp", fp), ("sum", total), ("value", value),
                    ("quotient1", q1), ("remainder1", r1), ("quotient2", q2)):
        a.tofile(os.path.join(str(tmp_path), name + ".bin"))
    with open(os.path.join(str(tmp_path), "tally.json"), "w") as fh:
        json.dump({"N": N, "q": q, "p": p, "B": B, "G": offsets.size - 1}, fh)
    del eng
    r = subprocess.run([NODE, os.path.join(ge.ROOT, "tests", "js", "shim_tally.mjs"), str(tmp_path)], cwd=ge.ROOT, capture_output=True,
                       text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    assert "shim_tally: " in r.stdout and "ragged batch of %d rows" % B in r.stdout
