"""The per-item scheme's CPU reference, built from oracle.ntru_oracle.polymul_split_batch (one key pair per row), and the edge operands
the GPU tests of matrix_peritem_scheme.hip feed it.  Not a test module: imported by tests/test_peritem_scheme_gpu.py and
tests/variant_runners.py (the runners of tests/test_kernel_variants_gpu.py)."""
import numpy as np

from oracle import ntru_oracle as orc


def oracle_encrypt(N, q, h, r, m):
    """r * h split by 1 - x^N modulo q, m added to the remainder (index.js:90-92)."""
    quot, rem = orc.polymul_split_batch(N, q, r.astype(np.uint16), h)
    return ((rem.astype(np.int64) + m) % q).astype(np.uint16), quot


def oracle_decrypt(N, q, p, f, fp, e):
    """f * e modulo q, the centred lift of index.js:117, then fp * a modulo p."""
    q1, r1 = orc.polymul_split_batch(N, q, (f.astype(np.int64) % q).astype(np.uint16), e)
    x = r1.astype(np.int64)
    a = np.where(2 * x > q, (x + 1) % p, x % p).astype(np.uint16)
    q2, r2 = orc.polymul_split_batch(N, p, fp.astype(np.uint16), a)
    return r2.astype(np.uint8), q1, r1, q2.astype(np.uint8)


def rows_cycle(B, makers):
    return np.stack([makers[b % len(makers)](b) for b in range(B)])


def monomial(N, k, sign):
    f = np.zeros(N, np.int64)
    f[k % N] = sign
    return f


def lift_edge_row(N, q):
    """0, q/2, q/2 + 1, q - 1 in sequence: under f = x^k, rem1 is a rotation of this row, so the strict `>` of the lift meets q/2 and
    q/2 + 1."""
    return np.resize(np.array([0, q // 2, q // 2 + 1, q - 1]), N)


def encrypt_operands(rng, N, q, B, variant=0):
    """h rows: all q-1, zero, random; r rows: all 2, all 1, zero, random ternary; m rows: all 255, all 0, random bytes.  `variant`
    shifts which kinds meet in one row."""
    h = rows_cycle(B, [lambda b: np.full(N, q - 1), lambda b: np.zeros(N), lambda b: rng.integers(0, q, N)]).astype(np.uint16)
    r = rows_cycle(B + variant, [lambda b: np.full(N, 2), lambda b: np.ones(N), lambda b: np.zeros(N),
                                 lambda b: rng.integers(0, 3, N)])[variant:].astype(np.uint8)
    m = rows_cycle(B + 2 * variant, [lambda b: np.full(N, 255), lambda b: np.zeros(N),
                                     lambda b: rng.integers(0, 256, N)])[2 * variant:].astype(np.uint8)
    return h, r, m


def decrypt_operands(rng, N, q, p, B, variant=0):
    """f rows: all -1, all +1, a single +-1 at index k (k = 0, N-1, 3b mod N), random ternary; e rows: all q-1, zero, all q/2, all
    q/2+1, random, a random mix of the four extremes, and the lift-edge row; fp rows: all p-1, a single 1, random.  The rows are cycled
    with different periods (f 6, e 7, fp 3) and `variant` shifts fp against them.  Row 0 holds the extremes, row 1 pairs f = x^(N-1)
    with the lift-edge row, row 2 is random."""
    fm = [lambda b: np.full(N, -1), lambda b: monomial(N, N - 1, 1), lambda b: rng.integers(-1, 2, N), lambda b: np.ones(N),
          lambda b: monomial(N, 0, -1), lambda b: monomial(N, 3 * b, 1 if b % 2 else -1)]
    em = [lambda b: np.full(N, q - 1), lambda b: lift_edge_row(N, q), lambda b: rng.integers(0, q, N), lambda b: np.full(N, q // 2),
          lambda b: np.full(N, q // 2 + 1), lambda b: np.zeros(N), lambda b: rng.choice([0, q - 1, q // 2, q // 2 + 1], N)]
    pm = [lambda b: np.full(N, p - 1), lambda b: monomial(N, b, 1), lambda b: rng.integers(0, p, N)]
    f = rows_cycle(B, fm).astype(np.int8)
    e = rows_cycle(B, em).astype(np.uint16)
    fp = rows_cycle(B + variant, pm)[variant:].astype(np.uint8)
    return f, fp, e


def assert_lift_edges_met(N, q, f, rem1):
    """A condition on the inputs, checked on the oracle's rem1: some row with a monomial f has rem1 at q/2 and at q/2 + 1 (B >= 2 and
    N >= 4, so that the lift-edge row holds all four of its values)."""
    if N < 4 or len(f) < 2:
        return
    mono = np.nonzero((f != 0).sum(axis=1) == 1)[0]
    hit = [b for b in mono if (rem1[b] == q // 2).any() and (rem1[b] == q // 2 + 1).any()]
    assert hit, ("no monomial row puts rem1 at q/2 and q/2 + 1", N, q, mono.tolist())
