"""numpy restatement of ntru_sum_groups (np.add.reduceat on widened integers, then mod) and the tally fixture: the checker the GPU tests
of the ciphertext sums use, tied to the reference by tests/test_ciphertext_sum_cpu.py."""
import base64
import json
import os

import numpy as np

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "tally_cases.json")


def unpack(a):
    """{bits, n, off, b64} of tests/golden/gen_tally_cases.mjs -> list of ints."""
    bits = np.unpackbits(np.frombuffer(base64.b64decode(a["b64"]), np.uint8), bitorder="little")[:a["n"] * a["bits"]]
    vals = bits.reshape(a["n"], a["bits"]).astype(np.int64) @ (1 << np.arange(a["bits"], dtype=np.int64))
    return (vals + a["off"]).tolist()


def load_cases():
    """The fixture with every packed array expanded: m, e as [K][N] lists, everything else as the reference returned it."""
    with open(GOLDEN) as fh:
        cases = json.load(fh)["cases"]
    for c in cases:
        N = c["options"]["N"]
        rows = lambda flat: [flat[k * N:(k + 1) * N] for k in range(c["K"])]
        c["key"] = {k: unpack(v) for k, v in c["key"].items()}
        c["m"], c["e"] = rows(unpack(c["m"])), rows(unpack(c["e"]))
        c["sum"], c["expected"] = unpack(c["sum"]), unpack(c["expected"])
        d = c["decrypt"]
        d["value"] = unpack(d["value"])
        d["inputs"] = {k: unpack(v) for k, v in d["inputs"].items()}
    return cases


def np_sum(rows, mod, offsets=None, K=None, weights=None, chunk=16384):
    """out[g] = (sum of weights[r] * rows[r] for r in group g) % mod, exact in int64 (w x < 2^32, at most 2^31 rows)."""
    rows = np.asarray(rows)
    B, N = rows.shape
    offsets = np.arange(0, B + 1, K, dtype=np.int64) if offsets is None else np.asarray(offsets, dtype=np.int64)
    G = offsets.size - 1
    out = np.zeros((G, N), np.int64)
    for a in range(int(offsets[0]), int(offsets[-1]), chunk):
        b = min(a + chunk, int(offsets[-1]))
        x = rows[a:b].astype(np.int64)
        if weights is not None:
            x *= np.asarray(weights[a:b]).astype(np.int64)[:, None]
        g_lo = int(np.searchsorted(offsets, a, side="right")) - 1       # the last group that starts at or before a
        g_hi = int(np.searchsorted(offsets, b, side="left")) - 1        # the last group that starts before b
        loc = np.clip(offsets[g_lo:g_hi + 2], a, b) - a
        nonempty = loc[1:] > loc[:-1]
        idx = loc[:-1][nonempty]                                        # contiguous groups: the segments tile [0, b - a)
        view = out[g_lo:g_hi + 1]
        view[nonempty] += np.add.reduceat(x, idx, axis=0)
    return (out % mod).astype(np.uint16)


def pad(a, N, dt):
    return np.array(list(a) + [0] * (N - len(a)), dtype=dt)


def case_arrays(c):
    """(N, q, p, f, fp, rows [K][N], weights or None, sum [N]) of a fixture case."""
    o = c["options"]
    N, q, p = o["N"], o["q"], o["p"]
    w = None if c["weights"] is None else np.array(c["weights"], np.uint16)
    return (N, q, p, pad(c["key"]["f"], N, np.int8), pad(c["key"]["fp"], N, np.uint8), np.array(c["e"], np.uint16).reshape(-1, N), w,
            np.array(c["sum"], np.uint16))
