"""What the tests of ntru_mul_shared_batch share: the numpy model of k_mul_shared_m's three plane products (rows = e_lo + 128 e_hi against
s = s0 + 128 s1, pass B shifted by 6 in a wrapping int32, pass A on top), the oracle's answer (polymul_split_batch on s repeated per row),
the launcher's rule, the operands that sit on the digits' edges, and the fixture captured from the unmodified reference."""
import json
import os

import numpy as np

import __graft_entry__ as ge
from oracle import ntru_oracle as orc

GOLDEN = os.path.join(ge.ROOT, "tests", "golden", "mulshared_cases.json")
RADIX, HALF, S1_MASK, CARRY_SHIFT = 128, 64, 0x3F, 6       # pinned to csrc/matrix_mulshared.hip by test_mulshared_cpu.py
FALLBACK_PASS = 65536


def want(N, mod, s, rows):
    """(quot, rem) of the oracle: polymul_split_batch(a = rows, b = s repeated per row)."""
    rows = np.ascontiguousarray(rows, np.uint16).reshape(-1, N)
    return orc.polymul_split_batch(N, mod, rows, np.tile(np.asarray(s, np.uint16), (rows.shape[0], 1)))


def s_planes(s, q):
    s = np.asarray(s, np.int64) & (q - 1)
    s0 = ((s + HALF) & (RADIX - 1)) - HALF
    return s0, 2 * (((s - s0) >> 7) & S1_MASK)


def row_planes(rows, q):
    e = np.asarray(rows, np.int64) & (q - 1)
    return e & (RADIX - 1), 2 * (e >> 7)


def _low_high(x, y, N):
    """Coefficients 0 .. N-1 and N .. 2N-1 of the linear products of the rows of x with y, exact."""
    lin = np.zeros((x.shape[0], 2 * N), np.int64)
    for b in range(x.shape[0]):
        lin[b, :2 * N - 1] = np.convolve(x[b], y)
    return lin[:, :N], lin[:, N:]


def _i32(x):
    return ((x + 2 ** 31) % 2 ** 32) - 2 ** 31


def plane_model(N, q, s, rows):
    """(quot, rem) as k_mul_shared_m computes them: int8 planes, int32 accumulators, the shift by 6 between the passes."""
    rows = np.asarray(rows).reshape(-1, N)
    e_lo, e_hi2 = row_planes(rows, q)
    s0, s1x2 = s_planes(s, q)
    for plane in (e_lo, e_hi2, s0, s1x2):
        assert plane.min() >= -128 and plane.max() <= 127
    acc = []
    for part in range(2):                                               # low, high
        b = _low_high(e_lo, s1x2, N)[part] + _low_high(e_hi2, s0, N)[part]
        a = _low_high(e_lo, s0, N)[part]
        assert np.abs(a).max() < 2 ** 31 and np.abs(b).max() < 2 ** 31     # every partial sum is inside an int32 before the shift
        acc.append(_i32(_i32(b << CARRY_SHIFT) + a))
    low, high = acc
    return ((-high) & (q - 1)).astype(np.uint16), ((low + high) & (q - 1)).astype(np.uint16)


def matrix_range(N, mod, path):
    """Whether k_mul_shared_m takes (N, mod) on kernel path `path` (make_mgeom with ld = N, and a power-of-two modulus)."""
    pow2 = mod & (mod - 1) == 0
    return pow2 and mod <= 8192 and N <= 1024 and path in (0, 4, 5) and N >= (2 if path >= 4 else 64)


def kernel_of(N, mod, path):
    """ntru_engine_last_kernel after the call: the matrix kernel, or the replicated route around a per-item kernel."""
    return "k_mul_shared_m" if matrix_range(N, mod, path) else "mul_shared_replicated("


def edge_s(N, q, rng):
    """Random s with {0, 63, 64, 65, 127, 128, q - 64, q - 1} (reduced modulo q) planted: every edge of both digits."""
    s = rng.integers(0, q, N).astype(np.uint16)
    edges = np.array([0, 63, 64, 65, 127, 128, q - 64, q - 1]) % q
    at = rng.permutation(N)[:min(N, len(edges))]
    s[at] = edges[:len(at)]
    return s


def operand_sets(N, q, B, rng):
    """(label, s, rows) of the operand kinds the kernel is checked on; unreduced values only for a power-of-two q."""
    rnd = lambda shape: rng.integers(0, q, shape).astype(np.uint16)
    spike = lambda i: np.eye(1, N, i, dtype=np.uint16)[0] * (q - 1)
    sets = [("random", rnd(N), rnd((B, N))),
            ("all_max", np.full(N, q - 1, np.uint16), np.full((B, N), q - 1, np.uint16)),
            ("edges", edge_s(N, q, rng), rnd((B, N))),
            ("spike_0", spike(0), rnd((B, N))),
            ("spike_last", spike(N - 1), rnd((B, N)))]
    if q & (q - 1) == 0:
        sets.append(("unreduced", np.full(N, 0xFFFF, np.uint16), np.full((B, N), 0xFFFF, np.uint16)))
    return sets


def load_sets():
    with open(GOLDEN) as fh:
        return json.load(fh)["sets"]


def pad(a, n):
    return list(a) + [0] * (n - len(a))
