"""An exact reference for k_invert_key (csrc/key_inversion.hip) that uses neither the kernel nor the oracle's poly_inv, the facts the
kernel and its launcher derive from N, and the rows of tests/test_key_inversion_geometry_gpu.py.

Plain data and plain arithmetic, imported by tests/test_key_inversion_geometry_cpu.py (the restatement against the source, what N_LIST
reaches, the promises of rows(N), the coverage conditions) and tests/test_key_inversion_geometry_gpu.py (four calls per N).  Not a
test module.

  is_unit(f, N, P)         gcd(f mod P, x^N - 1) over GF(P) is a constant: Euclid on Python integers used as bit planes
  check_inverse(...)       f inv = 1 modulo `mod` and x^N - 1 through the oracle's product; inverses are unique, so on units this is
                           a complete check of an inverse
  geometry(N, P)           NW, the register-plane class launch_invert<P> picks (0: planes in LDS), N & 31, whether a 16-element piece
                           of a whole block can cross into the next row
  whole_block(...)         whether a block of 64 rows goes through the whole-block input or output stage
  N_LIST                   the N of the sweep, derived from geometry()
  rows(N)                  B = 135 int8 rows (two whole blocks and a partial one) in ten families, interleaved over the three waves;
                           rows(N, order="sorted") has them grouped by family
  units(N)                 {2: ..., 3: ...}: which rows of rows(N) are units, promised by construction or computed by is_unit; cached"""
from collections import namedtuple

import numpy as np

from oracle import ntru_oracle as orc
from peritem_geometry import gf2_is_unit

FLAG_NOT_UNIT_MOD2, FLAG_NOT_UNIT_MODP = 8, 16
MIN_N, MAX_N = 2, 1920            # ntru_engine_supports
BLOCK = 64                        # keys per block: one per lane
PIECE = 16                        # elements per piece of the whole-block stages (16 bytes in, 16 or 32 bytes out)
WHOLE_MIN_N = 32                  # `N >= 32` of whole_in and whole
CLASSES = (2, 6, 12, 16, 22, 26)  # INV_CASE(W) of launch_invert<P>, both fields
CLASSES_GF2 = (32,)               # ... `if constexpr (P == 2)`
FIRST_BAND = 96                   # the band 96..127: class 6, NW = 4, registers for both fields
QS = (32, 128, 2048, 4096, 8192, 65536)


# ---- units and inverses ----------------------------------------------------------------------------------------------------------------

def _bits(mask):
    return int.from_bytes(np.packbits(mask, bitorder="little").tobytes(), "little")


def gf3_is_unit(f_row, N):
    """f is a unit modulo 3 and x^N - 1 iff gcd(f mod 3, x^N - 1) is a constant over GF(3).  A polynomial is two Python integers:
    bit i of the first says coefficient i is 1, of the second that it is 2 (negation swaps them)."""
    r = np.asarray(f_row, np.int64) % 3
    a1, a2 = 1 << N, 1                                            # x^N - 1
    b1, b2 = _bits(r == 1), _bits(r == 2)
    while b1 | b2:
        nb = b1 | b2
        db = nb.bit_length() - 1
        lb = 1 if b1 >> db & 1 else 2
        while True:
            na = a1 | a2
            da = na.bit_length() - 1
            if da < db:
                break
            la = 1 if a1 >> da & 1 else 2
            s = da - db
            # a -= (la / lb) x^s b; 1 / lb = lb in GF(3): subtract b where la == lb, add it otherwise
            t1, t2 = (b2 << s, b1 << s) if la == lb else (b1 << s, b2 << s)
            nt = t1 | t2
            a1, a2 = (a1 & ~nt) | (t1 & ~na) | (a2 & t2), (a2 & ~nt) | (t2 & ~na) | (a1 & t1)
        a1, a2, b1, b2 = b1, b2, a1, a2
    return (a1 | a2).bit_length() == 1


def is_unit(f, N, P):
    """True iff the int8 (or any integer) row f is invertible in Z_P[x] / (x^N - 1), P = 2 or 3."""
    assert P in (2, 3) and len(f) == N
    return gf2_is_unit(f, N) if P == 2 else gf3_is_unit(f, N)


def check_inverse(f, inv, N, mod):
    """Per row of f (B x N integers) and inv (B x N, unsigned): inv < mod everywhere and f inv = 1 modulo `mod` and x^N - 1."""
    f, inv = np.asarray(f).reshape(-1, N), np.asarray(inv).reshape(-1, N)
    if not len(f):
        return np.zeros(0, bool)
    a = (f.astype(np.int64) % mod).astype(np.uint16)
    rem = orc.polymul_split_batch(N, mod, a, inv.astype(np.uint16))[1]
    one = np.zeros(N, np.uint16); one[0] = 1
    return (rem == one).all(axis=1) & (inv.astype(np.int64) < mod).all(axis=1)


# ---- the kernel's own facts --------------------------------------------------------------------------------------------------------------

Geometry = namedtuple("Geometry", "N P NW cls planes top straddles")


def geometry(N, P):
    """NW = words per bit plane (N + 1 coefficients: the reversed modulus has degree N); cls = the NWC launch_invert<P> instantiates
    (`nw = (N + 32) / 32` against the cases, 0 = planes in LDS); top = N & 31, the bit of coefficient N of 1 - x^N in its word;
    straddles = a 16-element piece of a whole block's run can cross into the next row (16 does not divide N)."""
    assert MIN_N <= N <= MAX_N and P in (2, 3)
    nw = (N + 32) // 32
    cases = CLASSES + (CLASSES_GF2 if P == 2 else ())
    cls = next((W for W in cases if nw <= W), 0)
    return Geometry(N, P, (N + 1 + 31) >> 5, cls, "registers" if cls else "LDS", N & 31, N % PIECE != 0)


def whole_block(N, B, k0, aligned):
    """A block of 64 rows from row k0 on takes a whole-block stage: `k0 + 64 <= B && N >= 32` and the stage's pointers (f for the
    input stage, the outputs asked for for the output stage) on 16-byte boundaries."""
    return bool(aligned) and N >= WHOLE_MIN_N and k0 + BLOCK <= B


def regime(N):
    """(planes of GF(3), planes of GF(2))"""
    return geometry(N, 3).planes, geometry(N, 2).planes


REGIMES = (("registers", "registers"), ("LDS", "registers"), ("LDS", "LDS"))


def class_boundaries():
    """The N at which either field's class differs from that of N - 1."""
    return [N for N in range(MIN_N + 1, MAX_N + 1) if any(geometry(N, P).cls != geometry(N - 1, P).cls for P in (2, 3))]


def bands():
    """32 consecutive N from a multiple of 32 on, one band per regime: from FIRST_BAND, and from the first N of the two later regimes."""
    starts = [FIRST_BAND] + [next(N for N in range(MIN_N, MAX_N + 1) if regime(N) == r) for r in REGIMES[1:]]
    assert all(s % 32 == 0 for s in starts), starts
    return [range(s, s + 32) for s in starts]


def _n_list():
    ns = {MIN_N, MIN_N + 1, PIECE - 1, PIECE, PIECE + 1, WHOLE_MIN_N - 1, WHOLE_MIN_N, WHOLE_MIN_N + 1, MAX_N - 1, MAX_N}
    for N in class_boundaries():
        ns |= {N - 1, N}
    for band in bands():
        ns |= set(band)
    return sorted(ns)


N_LIST = _n_list()


def q_of(N):
    """q cycles through QS along N_LIST."""
    return QS[N_LIST.index(N) % len(QS)]


def slices(budget=1.6e7, most=16):
    """N_LIST cut into runs whose reference work stays small: the gcds of rows(N) cost about N^2 (0.3 s at N = 1920), a run holds at
    most `budget` of it and at most `most` N (the times are in tests/test_key_inversion_geometry_gpu.py)."""
    out, cost = [[]], 0
    for N in N_LIST:
        if out[-1] and (cost + N * N > budget or len(out[-1]) == most):
            out.append([])
            cost = 0
        out[-1].append(N)
        cost += N * N
    return out


# ---- the rows -----------------------------------------------------------------------------------------------------------------------------

B = 2 * BLOCK + 7                 # two whole blocks and a partial one
# (the grouped order ends with the random rows: from row 64 on its waves hold generic keys alone, whose |delta| stays small, so the
# shared word bounds are as tight there as they get, while every wave of the interleaved order has a zero row that loosens them)
FAMILIES = ("monomial", "zero", "ones", "times_x_minus_1", "factor", "dense_low", "dense_high", "sign_magnitude", "ternary", "int8")
MONOMIAL_K = (0, 1, 15, 16, 31, 32, -2, -1)
DENSE_D = (1, 2, 33, 0)           # 0: N / 2
EDGE_BYTES = (-128, -127, -3, -2, -1, 0, 1, 2, 3, 126, 127)
N_INT8 = 24
TAIL = ("zero", "monomial", "dense_low", "dense_high", "ternary", "int8", "sign_magnitude")     # the partial block's rows
SEED = 20

Rows = namedtuple("Rows", "f family promise perm")
_rows, _units = {}, {}


def cyclic_product(a, b, N):
    """a b modulo x^N - 1 over the integers."""
    full = np.convolve(np.asarray(a, np.int64), np.asarray(b, np.int64))
    out = np.zeros(N, np.int64)
    for at in range(0, len(full), N):
        part = full[at:at + N]
        out[:len(part)] += part
    return out


def ternary_row(rng, N):
    """The scheme's weights: N / 3 ones and N / 3 - 1 minus-ones (one 1 where N / 3 is 0)."""
    n1, n2 = max(N // 3, 1), max(N // 3 - 1, 0)
    f, perm = np.zeros(N, np.int64), rng.permutation(N)
    f[perm[:n1]], f[perm[n1:n1 + n2]] = 1, -1
    return f


def _build(N):
    """[(family, row, promise)] grouped by family; promise: True = a unit in both fields, False = in neither, None = is_unit says,
    ("as", j) = the status of row j of this list (a monomial times it)."""
    rng = np.random.default_rng([SEED, N])
    out = []

    def add(family, row, promise):
        row = np.asarray(row, np.int64)
        assert row.shape == (N,) and row.min() >= -128 and row.max() <= 127, (family, N)
        out.append((family, row, promise))

    for k in sorted({k % N for k in MONOMIAL_K if -N <= k < N}):
        for s in (1, -1):
            add("monomial", s * np.eye(1, N, k, dtype=np.int64)[0], True)
    for _ in range(3):
        add("zero", np.zeros(N), False)
    add("ones", np.ones(N), False)
    add("ones", -np.ones(N), False)
    for _ in range(4):                                            # a (x - 1): coefficients in -2..2, f(1) = 0
        a = rng.integers(-1, 2, N)
        add("times_x_minus_1", np.roll(a, 1) - a, False)
    divisors = [m for m in range(2, N) if N % m == 0]
    for m in sorted({divisors[0], divisors[-1]}) if divisors else ():
        phi = np.zeros(N, np.int64); phi[::m] = 1                 # 1 + x^m + ... + x^(N-m): phi (x^m - 1) = x^N - 1
        a = np.zeros(N, np.int64); a[:m] = rng.integers(-1, 2, m)
        add("factor", phi, False)
        add("factor", cyclic_product(a, phi, N), False)            # a repeated N / m times: ternary again
    low = []
    for d in DENSE_D:
        d = min(max(d or N // 2, 1), N)
        for _ in range(2):
            row = np.zeros(N, np.int64)
            row[:d] = rng.integers(-1, 2, d)
            row[d - 1] = rng.choice([-1, 1])                      # degree d - 1 exactly: rev(f) starts with N - d zeros
            low.append((len(out), d))
            add("dense_low", row, None)
    for j, d in low:
        add("dense_high", np.roll(out[j][1], N - d), ("as", j))   # x^(N-d) times the dense low row
    for s in range(len(EDGE_BYTES)):                              # every edge byte in every column, so in every lane of a 16-byte piece
        add("sign_magnitude", [EDGE_BYTES[(j + s) % len(EDGE_BYTES)] for j in range(N)], None)
    for _ in range(N_INT8):
        add("int8", rng.integers(-128, 128, N), None)
    while len(out) < B:
        add("ternary", ternary_row(rng, N), None)
    order = {name: i for i, name in enumerate(FAMILIES)}
    index = sorted(range(B), key=lambda i: order[out[i][0]])      # (stable: grouped by family, in the order of FAMILIES)
    where = {i: t for t, i in enumerate(index)}
    return [(out[i][0], out[i][1], ("as", where[out[i][2][1]]) if isinstance(out[i][2], tuple) else out[i][2]) for i in index]


def _interleave(N, family):
    """The permutation that spreads the sorted rows over the waves: the last row of each family of TAIL makes the partial block; of
    the other 128, neighbours in the sorted order go to different waves (so every family with two rows left is in both), and each
    wave is shuffled."""
    rng = np.random.default_rng([SEED + 1, N])
    tail = [max(i for i in range(B) if family[i] == name) for name in TAIL]
    rest = [i for i in range(B) if i not in tail]
    waves = [rest[0::2], rest[1::2]]
    return np.array([waves[w][t] for w in (0, 1) for t in rng.permutation(BLOCK)] + tail)


def rows(N, order="interleaved"):
    """Rows(f, family, promise, perm): f is B x N int8; family and promise per row; perm[i] = the row of the sorted order that row i
    is (so rows(N).f == rows(N, "sorted").f[rows(N).perm], and the sorted order's own perm is the identity)."""
    if N not in _rows:
        built = _build(N)
        f = np.array([r for _, r, _ in built]).astype(np.int8)
        family, promise = [b[0] for b in built], [b[2] for b in built]
        perm = _interleave(N, family)
        back = {int(j): i for i, j in enumerate(perm)}
        _rows[N] = {
            "sorted": Rows(f, family, promise, np.arange(B)),
            "interleaved": Rows(f[perm], [family[j] for j in perm],
                                [("as", back[promise[j][1]]) if isinstance(promise[j], tuple) else promise[j] for j in perm], perm)}
    return _rows[N][order]


def units(N, order="interleaved"):
    """{P: which rows of rows(N, order) are units modulo P}: the promise where there is one, is_unit elsewhere."""
    if N not in _units:
        r = rows(N, "sorted")
        got = {}
        for P in (2, 3):
            u = [p if isinstance(p, bool) else None for p in r.promise]
            for i, p in enumerate(r.promise):
                if p is None:
                    u[i] = is_unit(r.f[i], N, P)
            for i, p in enumerate(r.promise):
                if isinstance(p, tuple):
                    u[i] = u[p[1]]
            got[P] = np.array(u, bool)
        _units[N] = got
    perm = rows(N, order).perm
    return {P: u[perm] for P, u in _units[N].items()}
