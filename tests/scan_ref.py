"""Restatement of the scan (include/ntru_engine.h "scanning") without the engine, and the scan fixture: decryptBits through the oracle
under either lift (tests/lift_ref.py), the byte codec and its flags from tests/message_bytes_ref.py, the predicate in numpy.  The checker
of tests/test_scan_gpu.py, tied to the reference by tests/test_scan_cpu.py.  Not a test module."""
import base64
import json
import os

import numpy as np

import lift_ref
import message_bytes_ref as mb

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "scan_cases.json")


def unpack(a):
    """{bits, n, off, b64} of tests/golden/gen_scan_cases.mjs -> int64 array."""
    bits = np.unpackbits(np.frombuffer(base64.b64decode(a["b64"]), np.uint8), bitorder="little")[:a["n"] * a["bits"]]
    vals = bits.reshape(a["n"], a["bits"]).astype(np.int64) @ (1 << np.arange(a["bits"], dtype=np.int64))
    return vals + a["off"]


def load_cases():
    """The fixture with every packed array expanded: f [K][N] int8, fp [K][N] uint8, h [K][N] uint16, e [B][N] uint16, value [K][B][N]
    uint8, hit [K][B], tag as bytes; hits[k] = (rows int64 [.], bytes uint8 [.][W])."""
    with open(GOLDEN) as fh:
        cases = json.load(fh)["cases"]
    for c in cases:
        N, W, K = c["options"]["N"], c["W"], len(c["keys"])
        for name, dt in (("f", np.int8), ("fp", np.uint8), ("h", np.uint16)):
            c[name] = np.array([unpack(k[name]) for k in c["keys"]]).astype(dt)
        c["e"] = unpack(c["e"]).reshape(-1, N).astype(np.uint16)
        B = c["e"].shape[0]
        c["value"] = unpack(c["value"]).reshape(K, B, N).astype(np.uint8)
        c["hit"] = unpack(c["hit"]).reshape(K, B)
        c["tag"] = bytes(c["tag"])
        c["hits"] = [(np.array([h["row"] for h in l], np.int64), np.array([h["bytes"] for h in l], np.uint8).reshape(-1, W))
                     for l in c["hits"]]
    return cases


def select(data, flags, tag=b"", tag_off=0, max_hits=None):
    """The predicate and the compaction on what decrypt_bytes_batch returns for ONE key: data [B][nbytes], flags [B] ->
    (count, rows int64 [stored], bytes uint8 [stored][nbytes]), stored = min(count, max_hits), ascending rows."""
    data = np.asarray(data, np.uint8)
    tag = np.frombuffer(bytes(tag), np.uint8)
    assert 0 <= tag_off and tag_off + tag.size <= data.shape[1] and tag.size <= 32
    hit = (np.asarray(flags) == 0) & (data[:, tag_off:tag_off + tag.size] == tag).all(axis=1)
    rows = np.flatnonzero(hit).astype(np.int64)
    count = rows.size
    if max_hits is not None:
        rows = rows[:max_hits]
    return count, rows, data[rows]


def scan_values(value, nbytes, tag=b"", tag_off=0, max_hits=None):
    """select on decrypted coefficient rows value [B][N]."""
    data, flags = mb.np_rows_to_bytes(value, nbytes)
    return select(data, flags, tag, tag_off, max_hits)


def scan(N, q, p, nbytes, f, fp, e, tag=b"", tag_off=0, max_hits=None, mode=lift_ref.REFERENCE):
    """The definition: per key k of f [K][N], fp [K][N], decryptBits of every row of e under the lift `mode`, then the predicate.
    Returns (count [K] int64, [rows per key], [bytes per key])."""
    f, fp = np.asarray(f).reshape(-1, N), np.asarray(fp).reshape(-1, N)
    res = [scan_values(lift_ref.decrypt(N, q, p, f[k].astype(np.int8), fp[k].astype(np.uint8), e, mode)[0], nbytes, tag, tag_off, max_hits)
           for k in range(f.shape[0])]
    return np.array([r[0] for r in res], np.int64), [r[1] for r in res], [r[2] for r in res]


def same(got, want):
    """Do two (count, rows, bytes) results agree?"""
    return (np.array_equal(np.asarray(got[0]), np.asarray(want[0])) and len(got[1]) == len(want[1]) == len(got[2]) == len(want[2]) and
            all(np.array_equal(a, b) for a, b in zip(got[1], want[1])) and all(np.array_equal(a, b) for a, b in zip(got[2], want[2])))
