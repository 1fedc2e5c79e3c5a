"""What the tests of ntru_combine_batch check against: the exact integer matrix product in numpy, the digit-plane arithmetic of
k_combine_m restated with wrapping int32 accumulators, the launcher's rule (which kernel for which modulus and kernel path), and the
fixture of the unmodified reference (tests/golden/gen_combine_cases.mjs)."""
import json
import os

import numpy as np

from ciphertext_sum_ref import pad, unpack

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "combine_cases.json")
MAX_G = 4096


def np_combine(rows, weights, mod):
    """out [G][N] = (weights^T . rows) % mod, exact in int64: at most 65535^2 * 2^31 < 2^63."""
    rows, weights = np.asarray(rows).astype(np.int64), np.asarray(weights).astype(np.int64)
    return ((weights.T @ rows) % mod).astype(np.uint16)


# ---- the digit planes of k_combine_m ----------------------------------------------------------------------------------------------
def planes_of(mod):
    """Planes per operand: the low byte alone carries everything modulo a modulus whose values have at most 8 bits (mod <= 256 divides 256)."""
    return 1 if (int(mod) - 1).bit_length() <= 8 else 2


def digits(x):
    """x = lo + 256 hi (mod 2^16): lo the low byte read as int8, hi = (x + 128) >> 8 read as int8 (by wrap)."""
    x = np.asarray(x).astype(np.int64)
    lo = (x & 0xFF).astype(np.uint8).view(np.int8)
    hi = (((x + 128) >> 8) & 0xFF).astype(np.uint8).view(np.int8)
    return lo.astype(np.int64), hi.astype(np.int64)


def wrap32(x):
    """What an int32 accumulator holds after sums that wrap: the value modulo 2^32, signed."""
    return ((np.asarray(x, dtype=np.int64) + (1 << 31)) % (1 << 32)) - (1 << 31)


def plane_model(rows, weights, mod, block=1 << 15):
    """k_combine_m in numpy: lo.lo into one wrapping int32 accumulator, lo.hi + hi.lo into a second that counts 256-fold, hi.hi
    dropped; mod a power of two.  The contraction runs in blocks so that the int64 stand-in never overflows."""
    assert mod & (mod - 1) == 0
    rlo, rhi = digits(rows)
    wlo, whi = digits(weights)
    G, N = wlo.shape[1], rlo.shape[1]
    acc0, acc1 = np.zeros((G, N), np.int64), np.zeros((G, N), np.int64)
    for a in range(0, rlo.shape[0], block):
        s = slice(a, a + block)
        acc0 = wrap32(acc0 + wlo[s].T @ rlo[s])
        if planes_of(mod) == 2:
            acc1 = wrap32(acc1 + wlo[s].T @ rhi[s] + whi[s].T @ rlo[s])
    v = (acc0 + (acc1 << 8)) % (1 << 32)
    return (v & (mod - 1)).astype(np.uint16)


# ---- the launcher's rule ------------------------------------------------------------------------------------------------------------
def kernel_of(mod, path, G):
    """The name ntru_engine_last_kernel reports after a combine call of G outputs: k_combine_m<digit planes, output tiles of 32 per
    workgroup> or k_combine_v<power of two?>."""
    pow2 = mod & (mod - 1) == 0
    if pow2 and path in (0, 4, 5):
        return "k_combine_m<%d,%d>" % (planes_of(mod), 1 if G <= 32 else 2)
    return "k_combine_v<%d>" % int(pow2)


# ---- the fixture --------------------------------------------------------------------------------------------------------------------
def load_sets():
    """The fixture with every packed array expanded.  Per set: options, key, m and e as [B][N] lists, and cases of {kind, G, weights
    [B][G], outputs: G of {sum, expected, recovered, decrypt as the reference returned it}}."""
    with open(GOLDEN) as fh:
        sets = json.load(fh)["sets"]
    for s in sets:
        N = s["options"]["N"]
        rows = lambda flat: [flat[k * N:(k + 1) * N] for k in range(s["B"])]
        s["key"] = {k: unpack(v) for k, v in s["key"].items()}
        s["m"], s["e"] = rows(unpack(s["m"])), rows(unpack(s["e"]))
        for c in s["cases"]:
            for o in c["outputs"]:
                o["sum"], o["expected"] = unpack(o["sum"]), unpack(o["expected"])
                d = o["decrypt"]
                d["value"] = unpack(d["value"])
                d["inputs"] = {k: unpack(v) for k, v in d["inputs"].items()}
    return sets


def set_arrays(s):
    """(N, q, p, f, fp, rows [B][N] uint16) of a fixture set."""
    o = s["options"]
    N = o["N"]
    return (N, o["q"], o["p"], pad(s["key"]["f"], N, np.int8), pad(s["key"]["fp"], N, np.uint8),
            np.array(s["e"], np.uint16).reshape(-1, N))


def case_arrays(s, c):
    """(weights [B][G] uint16, sums [G][N] uint16) of a case of set s."""
    N = s["options"]["N"]
    return np.array(c["weights"], np.uint16).reshape(s["B"], c["G"]), np.array([pad(o["sum"], N, np.uint16) for o in c["outputs"]])
