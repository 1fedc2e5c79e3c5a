"""numpy restatement of the byte-message codec (np.unpackbits / np.packbits, most significant bit first) and the bytes fixture: the
checker the GPU tests of message_bytes.hip use, tied to the reference by tests/test_message_bytes_cpu.py."""
import base64
import json
import os

import numpy as np

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "bytes_cases.json")
FLAG_NOT_BITS, FLAG_PAD_NONZERO = 32, 64


def unpack(a):
    """{bits, n, off, b64} of tests/golden/gen_bytes_cases.mjs -> list of ints."""
    bits = np.unpackbits(np.frombuffer(base64.b64decode(a["b64"]), np.uint8), bitorder="little")[:a["n"] * a["bits"]]
    vals = bits.reshape(a["n"], a["bits"]).astype(np.int64) @ (1 << np.arange(a["bits"], dtype=np.int64))
    return (vals + a["off"]).tolist()


def load_sets():
    """The fixture with every packed array expanded to a list of ints."""
    with open(GOLDEN) as fh:
        sets = json.load(fh)["sets"]
    for s in sets:
        s["key"] = {k: unpack(v) for k, v in s["key"].items()}
        for m in s["messages"]:
            m["blocks"] = [{k: unpack(v) for k, v in b.items()} for b in m["blocks"]]
            m["data"] = bytes(x for b in m["blocks"] for x in b["chunk"])
    return sets


def pad(a, N, dt):
    return np.array(list(a) + [0] * (N - len(a)), dtype=dt)


def set_key(s):
    """(N, q, p, W, h, f, fp) of a fixture set as padded arrays."""
    o = s["options"]
    N = o["N"]
    return (N, o["q"], o["p"], s["W"], pad(s["key"]["h"], N, np.uint16), pad(s["key"]["f"], N, np.int8),
            pad(s["key"]["fp"], N, np.uint8))


def block_arrays(s):
    """Every block of a set: (chunks zero padded to [n][W], r [n][N], value [n][N] uint16, decrypted [n][N])."""
    N, W = s["options"]["N"], s["W"]
    blocks = [b for m in s["messages"] for b in m["blocks"]]
    chunks = np.array([b["chunk"] + [0] * (W - len(b["chunk"])) for b in blocks], np.uint8)
    return (chunks, np.array([b["r"] for b in blocks], np.uint8), np.array([b["value"] for b in blocks], np.uint16),
            np.array([b["decrypted"] for b in blocks], np.uint8))


def np_bytes_to_rows(data, N):
    """[B][nbytes] bytes -> [B][N] rows: coefficient 8 i + j = bit 7 - j of byte i, the pad 0."""
    data = np.asarray(data, np.uint8)
    B, nbytes = data.shape
    m = np.zeros((B, N), np.uint8)
    m[:, :8 * nbytes] = np.unpackbits(data, axis=1, bitorder="big")
    return m


def np_rows_to_bytes(value, nbytes):
    """[B][N] rows -> ([B][nbytes] bytes of the low bits, [B] flags)."""
    value = np.asarray(value, np.uint8)
    msg = value[:, :8 * nbytes]
    out = np.packbits(msg & 1, axis=1, bitorder="big")
    flags = (np.where((msg > 1).any(axis=1), FLAG_NOT_BITS, 0) |
             np.where((value[:, 8 * nbytes:] != 0).any(axis=1), FLAG_PAD_NONZERO, 0)).astype(np.uint8)
    return out, flags
