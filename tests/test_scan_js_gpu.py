"""scanBytes of the Node.js shim (tests/js/shim_scan.mjs, a fresh process): composed from decryptBytes per key and a filter in JavaScript,
which need the engine and so a GPU, it reproduces tests/golden/scan_cases.json and agrees with the Python side on an engine-made
batch (expected: decrypt_bytes_batch per key plus tests/scan_ref.py's filter, written to a file the Node process reads)."""
import base64
import json
import os
import shutil
import subprocess

import numpy as np
import pytest

import __graft_entry__ as ge
import scan_ref as ref

NODE = shutil.which("node")


@pytest.mark.gpu
@pytest.mark.skipif(NODE is None, reason="node is not installed")
def test_shim_scan(tmp_path):
    pkg = ge.build()
    eng = pkg.Engine(0)
    c = ref.load_cases()[1]
    o = c["options"]
    N, q, p, W, B, tag, off, max_hits = o["N"], o["q"], o["p"], c["W"], 150, b"NTRU", 9, 20
    g = np.random.default_rng(150)
    owner = g.integers(0, 4, B)                         # keys 0 .. 2, 3: arbitrary values
    data = g.integers(0, 256, (B, W), dtype=np.uint8)
    data[:, off:off + 4] = np.frombuffer(tag, np.uint8)
    e = g.integers(0, q, (B, N)).astype(np.uint16)
    for k in range(3):
        idx = np.flatnonzero(owner == k)
        r = np.zeros((idx.size, N), np.uint8)
        r[:, :o["dr"]], r[:, o["dr"]:2 * o["dr"]] = 1, 2
        e[idx] = eng.encrypt_bytes_batch(N, q, W, c["h"][k], g.permuted(r, axis=1), data[idx], want_quot=False)[0]
    want = []
    for k in range(3):
        count, rows, kept = ref.select(*eng.decrypt_bytes_batch(N, q, p, W, c["f"][k], c["fp"][k], e), tag, off, max_hits)
        assert count > max_hits == rows.size
        want.append({"count": int(count), "rows": rows.tolist(), "bytes": base64.b64encode(kept.tobytes()).decode()})
    got = pkg.scan_bytes_batch(eng, N, q, p, W, c["f"], c["fp"], e, tag, off, max_hits)
    assert [int(x) for x in got[0]] == [w["count"] for w in want] and [r.tolist() for r in got[1]] == [w["rows"] for w in want]
    path = os.path.join(str(tmp_path), "scan_expected.json")
    with open(path, "w") as fh:
        json.dump({"options": o, "B": B, "tag": list(tag), "tagOffset": off, "maxHits": max_hits,
                   "e": base64.b64encode(e.tobytes()).decode(),
                   "keys": [{"f": c["f"][k].tolist(), "fp": c["fp"][k].tolist()} for k in range(3)], "want": want}, fh)
    eng.close()
    r = subprocess.run([NODE, os.path.join(ge.ROOT, "tests", "js", "shim_scan.mjs"), path], cwd=ge.ROOT, capture_output=True, text=True,
                       timeout=600)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    assert "shim_scan: 12 key results of 3 cases and one batch" in r.stdout
