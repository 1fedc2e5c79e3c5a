"""numpy restatement of ntru_reencrypt_batch (include/ntru_engine.h "re-randomising and shuffling") and the mix fixture: the checker the
GPU tests of the re-encrypt kernels use, tied to the reference by tests/test_mix_cpu.py.  Not a test module."""
import base64
import json
import os

import numpy as np

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "mix_cases.json")


def unpack(a):
    """{bits, n, off, b64} of tests/golden/gen_mix_cases.mjs -> int64 array."""
    bits = np.unpackbits(np.frombuffer(base64.b64decode(a["b64"]), np.uint8), bitorder="little")[:a["n"] * a["bits"]]
    vals = bits.reshape(a["n"], a["bits"]).astype(np.int64) @ (1 << np.arange(a["bits"], dtype=np.int64))
    return vals + a["off"]


def load_cases():
    """The fixture with every packed array expanded to numpy: key rows (N,), m / e [6][N], per round r, remainder, quotient, value
    [B][N], src and recovered [B]."""
    with open(GOLDEN) as fh:
        cases = json.load(fh)["cases"]
    for c in cases:
        N = c["options"]["N"]
        c["key"] = {k: np.pad(unpack(v), (0, N - v["n"])) for k, v in c["key"].items()}          # fp is trimmed: padded to N
        c["m"], c["e"] = unpack(c["m"]).reshape(-1, N), unpack(c["e"]).reshape(-1, N)
        for rd in c["rounds"]:
            rd["src"] = np.array(rd["src"], np.int64)
            for k in ("r", "remainder", "quotient", "value"):
                rd[k] = unpack(rd[k]).reshape(-1, N)
            rd["recovered"] = unpack(rd["recovered"])
    return cases


def gather_rows(e_in, src, B, q):
    """The addend of every output row, reduced mod q: row src[i] (i without src) of e_in, zeros for an index outside [0, B_in)."""
    e_in = np.asarray(e_in).astype(np.int64) % q
    s = np.arange(B, dtype=np.int64) if src is None else np.asarray(src, np.int64)
    ok = (s >= 0) & (s < e_in.shape[0])
    out = np.zeros((B, e_in.shape[1]), np.int64)
    out[ok] = e_in[s[ok]]
    return out


def reencrypt(N, q, h, r, e_in, src=None):
    """(e_out, quotE) [B][N] uint16: (r[i] * h + e_in[s]) mod q split by 1 - x^N.  With lin = r[i] * h as a linear product, low its
    coefficients 0..N-1 and high its coefficients N..2N-2: e_out = (low + high + e_in[s]) mod q, quotE = -high mod q -- the addend
    only touches the low N coefficients, so the quotient is that of Enc(0; r[i])."""
    h = np.asarray(h).astype(np.int64).reshape(N) % q
    r = np.asarray(r).astype(np.int64).reshape(-1, N)
    B = r.shape[0]
    add = gather_rows(np.asarray(e_in).reshape(-1, N), src, B, q)
    e_out, quot = np.empty((B, N), np.uint16), np.empty((B, N), np.uint16)
    for i in range(B):
        lin = np.convolve(r[i], h)                       # exact: below 3 * 65535 * N
        high = np.zeros(N, np.int64)
        high[:N - 1] = lin[N:]
        e_out[i] = (lin[:N] + high + add[i]) % q
        quot[i] = (-high) % q
    return e_out, quot
