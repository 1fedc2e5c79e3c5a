"""sumPackedCiphertexts and tallyPackedBatch of the Node.js shim (tests/js/shim_packed.mjs, a fresh process): the shim composes them from
unpackBatch, sumGroups and tallyDecryptBatch, which need the engine and so a GPU; their results equal the restatement
(tests/packed_ref.py) and the Python engine's packed calls."""
import json
import os
import shutil
import subprocess

import numpy as np
import pytest

import __graft_entry__ as ge
import packed_ref as ref

NODE = shutil.which("node")
pkg = ge.load_package()


@pytest.mark.gpu
@pytest.mark.skipif(NODE is None, reason="node is not installed")
def test_shim_packed(tmp_path):
    ge.build()
    N, q, p, B = 821, 4096, 3, 300
    g = np.random.default_rng(21)
    rows = g.integers(0, q, (B, N), dtype=np.uint16)
    packed = ref.set_ignored_bits(q, N, ref.pack_rows(q, rows))
    weights = g.integers(0, q, B, dtype=np.uint16)
    offsets = np.array([1, 1, 2, 40, 40, 250, 251, 290, 290], np.int64)
    f, fp = g.integers(-1, 2, N).astype(np.int8), g.integers(0, 3, N).astype(np.uint8)
    eng = pkg.Engine(0)
    total, value, q1, r1, q2 = pkg.tally_decrypt_packed_batch(eng, N, q, p, f, fp, packed, offsets=offsets, weights=weights)
    assert np.array_equal(total, ref.np_sum_packed(q, N, packed, offsets=offsets, weights=weights))
    for name, a in (("packed", packed), ("weights", weights), ("offsets", offsets), ("f", f), ("fp", fp), ("sum", total), ("value", value),
                    ("quotient1", q1), ("remainder1", r1), ("quotient2", q2),
                    ("sum_plain", ref.np_sum_packed(q, N, packed, offsets=offsets)), ("sum_all", ref.np_sum_packed(q, N, packed, K=B))):
        np.ascontiguousarray(a).tofile(os.path.join(str(tmp_path), name + ".bin"))
    with open(os.path.join(str(tmp_path), "packed.json"), "w") as fh:
        json.dump({"N": N, "q": q, "p": p, "B": B, "G": offsets.size - 1}, fh)
    del eng
    r = subprocess.run([NODE, os.path.join(ge.ROOT, "tests", "js", "shim_packed.mjs"), str(tmp_path)], cwd=ge.ROOT, capture_output=True,
                       text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    assert "shim_packed: %d packed rows" % B in r.stdout
