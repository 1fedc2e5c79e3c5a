"""What the tests of ntru_noise_batch share: the plain numpy reduction of a remainder row to (peak, energy), the expected values from
the oracle's decrypt_batch rem1, the launcher's rule, the operand builders (random rows, honest ciphertexts from the oracle's keygen
and encrypt, a monomial key against rows that put one chosen coefficient into a), and the fixture captured from the unmodified
reference.  Not a test module."""
import functools
import json
import os

import numpy as np

import __graft_entry__ as ge
import keygen_ref
from oracle import ntru_oracle as orc

GOLDEN = os.path.join(ge.ROOT, "tests", "golden", "noise_cases.json")
PASS = 65536                                  # rows per pass of the slow route: pinned to csrc/matrix_noise.hip by test_noise_cpu.py
MAX_STRIPS = 8


def centred(a, q):
    """c_k = a_k > q/2 ? a_k - q : a_k (strict: q/2 stays +q/2)."""
    a = np.asarray(a, np.int64)
    return np.where(a > q // 2, a - q, a)


def reduce_rows(a, q):
    """(peak [B] uint16, energy [B] uint64) of remainder rows a [B][N] with entries in [0, q)."""
    c = centred(np.asarray(a).reshape(len(a), -1), q)
    return np.abs(c).max(axis=1).astype(np.uint16), (c * c).sum(axis=1).astype(np.uint64)


def rem1(N, q, f, e):
    """The oracle's remainder1 of decryptBits for every row (p = 3 against a zero fp: product 1 does not depend on either)."""
    return orc.decrypt_batch(N, q, 3, f, np.zeros(N, np.uint8), np.ascontiguousarray(e, np.uint16).reshape(-1, N))[2]


def want(N, q, f, e):
    return reduce_rows(rem1(N, q, f, e), q)


def matrix_range(N, q, path):
    """Whether k_noise_m takes (N, q) on kernel path `path`: make_mgeom with ld = N."""
    return q <= 8192 and N <= 1024 and path in (0, 4, 5) and N >= (2 if path >= 4 else 64)


def kernel_of(N, q, path):
    """ntru_engine_last_kernel after the call: the matrix kernel, or the slow route around the product's kernel."""
    return "k_noise_m" if matrix_range(N, q, path) else "noise_rows("


# ---- operands ----------------------------------------------------------------------------------------------------------------------------
def ternary(rng, N):
    return rng.integers(-1, 2, N).astype(np.int8)


@functools.lru_cache(maxsize=None)
def honest_key(N, q):
    """A key pair of the oracle's keygen with weights that scale with N (f: df ones and df - 1 minus ones; g: dg of each)."""
    df, dg = max(1, N // 8), max(1, N // 16)
    k = keygen_ref.key_pairs(N, q, df, dg, np.arange(8, dtype=np.uint32) + N, 0, 1, 32)
    assert not k["flags"].any(), (N, q)
    return k["f"][0].copy(), k["g"][0].copy(), k["h"][0].copy()


def honest(N, q, B, seed=0):
    """(f, e): B encryptions of random bits under honest_key(N, q), r with dr ones and dr entries p - 1 from the oracle's sampler."""
    f, _, h = honest_key(N, q)
    dr = max(1, N // 32)
    r = orc.sample_ternary_batch(N, dr, dr, 2, np.arange(8, dtype=np.uint32) + 100 + seed, 0, B)
    m = np.random.default_rng(seed + N).integers(0, 2, (B, N)).astype(np.uint8)
    return f, orc.encrypt_batch(N, q, h, r, m, want_quot=False)[0]


def monomial(N, j, sign):
    f = np.zeros(N, np.int8)
    f[j % N] = sign
    return f


def spike_rows(N, q, j, sign, cols, values):
    """Rows whose a under f = sign x^j is zero except a_k = v: one row per (k, v) of cols x values; (rows, the a they give)."""
    rows = np.zeros((len(cols) * len(values), N), np.uint16)
    a = np.zeros_like(rows)
    b = 0
    for k in cols:
        for v in values:
            rows[b, (k - j) % N] = (sign * v) % q
            a[b, k] = v % q
            b += 1
    return rows, a


def edge_values(q):
    """1, q/2 - 1, q/2, q/2 + 1 and q - 1, reduced modulo q (they collapse for the smallest q)."""
    return sorted({v % q for v in (1, q // 2 - 1, q // 2, q // 2 + 1, q - 1)})


def border_columns(N):
    """Every tile border, the column in front of it, and the ends of the row."""
    return sorted({k for k in list(range(0, N, 32)) + list(range(31, N, 32)) + [1, N - 2, N - 1] if 0 <= k < N})


# ---- the fixture ---------------------------------------------------------------------------------------------------------------------------
def load_sets():
    """The fixture with every packed array expanded.  Per set: options, f and g [N], r and m [B][N], and cases of {K, inside, e,
    remainder1, A} for the sum of the first K ciphertexts."""
    from ciphertext_sum_ref import unpack
    with open(GOLDEN) as fh:
        sets = json.load(fh)["sets"]
    for s in sets:
        N = s["options"]["N"]
        rows = lambda flat: [flat[k * N:(k + 1) * N] for k in range(s["B"])]
        s["f"], s["g"] = unpack(s["key"]["f"]), unpack(s["key"]["g"])
        s["r"], s["m"] = rows(unpack(s["r"])), rows(unpack(s["m"]))
        for c in s["cases"]:
            for name in ("e", "remainder1", "A"):
                c[name] = unpack(c[name])
    return sets


def plain_A(N, p, f, g, rs, ms):
    """A = p sum(r * g) + f * sum(m) modulo x^N - 1 over the integers; r as encryptBits multiplies it, in {0, 1, p - 1} (index.js:89)."""
    cyc = lambda x, y: np.array([sum(int(x[i]) * int(y[(k - i) % N]) for i in range(N)) for k in range(N)], np.int64)
    rsum = sum(np.asarray(r, np.int64) for r in rs)
    msum = sum(np.asarray(m, np.int64) for m in ms)
    return p * cyc(rsum, np.asarray(g, np.int64)) + cyc(np.asarray(f, np.int64), msum)
