"""The geometry that the per-item matrix kernels of csrc/matrix_peritem.hip (k_verify_keys_m, k_polymul_m, k_product_tern_m,
k_newton_round_m) derive from N, and the edge operands of tests/test_peritem_geometry_gpu.py.

Plain data, imported by tests/test_peritem_geometry_cpu.py (the restatement against the constants of the source, what the sweep
N = 64..1024 reaches, the promises of the operand builders) and tests/test_peritem_geometry_gpu.py (every output of the sweep against
the oracle).  Not a test module.

A Python restatement of the host and lane arithmetic of csrc/peritem_common.h and csrc/matrix_peritem.hip:
  make_pgeom           NT = ceil(N / 32) tiles, tpitch dwords per copy of a reversed array; P = 32 NT - N places that the moved copy of
                       the products modulo x^N - 1 is moved up by
  pi_product_plan      the split product's loop: trips in pairs, a single trip behind them iff NT is even
  pi_product_cyc       trips in pairs, then `trip, last` (NT odd) or `last` alone (NT even; at NT = 2 nothing else runs)
  pi_build_array_half  the period stored once, the margins by other lanes: chunks 0..2 behind it, the chunks that hold coefficients
                       N - 36 .. N - 1 in front of it (3 or 4 of them); one store for both from N = 160, two below
  pi_nat_bytes         three periods + 64 bytes, rounded up to 16, but 2304 at the least; pi_wave_bytes adds the reversed arrays
  k_verify_keys_m      the set of coefficients that a lane compares with h: lane l holds 16 l .. 16 l + 15, those below N count
  peritem_applies      a power of two <= 8192, N <= 1024, N >= 64 at kernel path 4 and >= 128 at kernel path 0

The operand builders are seeded by N alone (values are then reduced to the call's modulus), so every module sees the same rows."""
import numpy as np

from oracle import ntru_oracle as orc

NS = range(64, 1025)
PI_HALF_BASE = 64                 # byte offset of the period in the natural-order area
PI_IMG = 1152                     # bytes between the images of two planes
PI_WAVES = 2
HALF_ONE_STORE_N = 160            # pi_build_array_half: behind and front margins in ONE store instruction from this N
FRONT_MARGIN = 36                 # ... the front margin: the chunks that reach coefficient N - 36 or beyond
NAT_MIN_BYTES = 2304
MIN_N = {0: 128, 4: 64}           # kernel path -> smallest N the family takes
MAX_N, MAX_Q = 1024, 8192
FLAG_INVALID_FQ, FLAG_INVALID_FP, FLAG_INVALID_H, FLAG_NOT_UNIT_MOD2 = 1, 2, 4, 8


# ---- host and lane geometry -----------------------------------------------------------------------------------------------------------

def pgeom(N):
    """(NT, tpitch) of make_pgeom."""
    NT = (N + 31) // 32
    return NT, ((16 * NT + 31) // 32) * 32 + 8


def moved_by(N):
    """P = 32 NT - N: 0 .. 31."""
    return 32 * pgeom(N)[0] - N


def split_loop(N):
    """(pairs of trips, single trips behind them) of pi_product_plan and of k_polymul_m<false>'s written-out loop."""
    NT, j, pairs = pgeom(N)[0], 1, 0
    while j + 1 < NT:
        pairs, j = pairs + 1, j + 2
    return pairs, int(j < NT)


def cyc_tail(N):
    """(pairs of trips, tail) of pi_product_cyc; the tail is "trip+last" or "last"."""
    NT, j, pairs = pgeom(N)[0], 1, 0
    while j + 1 <= NT - 2:
        pairs, j = pairs + 1, j + 2
    return pairs, "trip+last" if j <= NT - 2 else "last"


def cyc_tail_shape(N):
    """The three shapes of that tail: "last alone" (NT = 2), "trip+last" (NT odd), "pairs, last" (NT even and above 2)."""
    pairs, tail = cyc_tail(N)
    return tail if tail == "trip+last" else ("pairs, last" if pairs else "last alone")


def cyc_keep_bytes(N, lane):
    """Bytes of each of the lane's four dwords that the last distance of pi_product_cyc CUTS (pi_cyc_keep): rows <= NT - 2 lose
    their bytes 16 hh + j < P."""
    NT = pgeom(N)[0]
    u = moved_by(N) - 16 * (lane >> 5) if (lane & 31) <= NT - 2 else 0
    return [min(max(u - 4 * c, 0), 4) for c in range(4)]


def half_array_stores(N):
    """pi_build_array_half: (one store for both margins?, the chunks stored in front of the period, the chunks stored behind it)."""
    front = [ch for ch in range(64) if 16 * ch < N and 16 * ch + 15 >= N - FRONT_MARGIN]
    behind = [ch for ch in range(3)]
    return N >= HALF_ONE_STORE_N, front, behind


def nat_bytes(N):
    periods = (3 * N + 64 + 15) & ~15
    return max(periods, NAT_MIN_BYTES)


def wave_bytes(N, arrays):
    return nat_bytes(N) + arrays * 16 * pgeom(N)[1]


def h_valid(N, lane):
    """The lane's `valid` set of k_verify_keys_m's comparison with h, in its split layout: coefficient 16 lane + 2 c in bit c,
    16 lane + 2 c + 1 in bit 16 + c; and `left`, the coefficients of the lane's chunk that exist (None where i0 < 32 NT gates it)."""
    i0 = 16 * lane
    if i0 >= 32 * pgeom(N)[0]:
        return 0, None
    left = N - i0
    if left <= 0:                                                 # (the kernel's `valid` is 0 there whatever ne and no are)
        return 0, left
    ne = 0xFF if left >= 16 else (1 << ((left + 1) >> 1)) - 1
    no = 0xFF if left >= 16 else (1 << (left >> 1)) - 1
    return (0 if left <= 0 else ne | no << 16), left


def last_lane_left(N):
    """`left` of the last lane that holds a coefficient: 1 .. 16."""
    return N - 16 * ((N - 1) // 16)


def applies(N, q, path):
    """peritem_applies at kernel path 0 or 4."""
    return path in MIN_N and q & (q - 1) == 0 and 2 <= q <= MAX_Q and MIN_N[path] <= N <= MAX_N


def paths(N):
    """The kernel paths of the sweep at this N: 4, and 0 where the automatic choice takes the family."""
    return [path for path in (4, 0) if N >= MIN_N[path]]


# ---- edge operands ----------------------------------------------------------------------------------------------------------------------

def spikes(N):
    """S of the sweep, clipped to [0, N): the first places, both sides of the 16-coefficient chunk and the 32-coefficient tile edges
    at either end, P, and the last two indices."""
    P = moved_by(N)
    S = {0, 1, 15, 16, 17, 31, 32, P, N - 33, N - 32, N - 17, N - 16, N - 15, N - 2, N - 1}
    return sorted(k for k in S if 0 <= k < N)


def spike_pairs(N):
    """(i, j), both from spikes(N): every pair with i + j = N - 1 (the last index), N (pure wrap to index 0) or 2 N - 2, every spike
    against P both ways round, and (0, 0)."""
    S, P = spikes(N), moved_by(N)
    pairs = [(i, j) for i in S for j in S if i + j in (N - 1, N, 2 * N - 2)]
    pairs += [(i, P) for i in S] + [(P, j) for j in S] + [(0, 0)]
    return list(dict.fromkeys(pairs))


def _rng(tag, N):
    return np.random.default_rng([tag, N])


def _ternary(rng, shape):
    return rng.integers(-1, 2, shape)


def public_key_rows(N, q):
    """(fq, g): (q - 1) x^i against +-x^j for the spike pairs; all q - 1 against all +1 and all -1; two random rows."""
    pairs, rng = spike_pairs(N), _rng(1, N)
    B = len(pairs) + 4
    fq, g = np.zeros((B, N), np.int64), np.zeros((B, N), np.int64)
    for t, (i, j) in enumerate(pairs):
        fq[t, i], g[t, j] = q - 1, (1 if t % 2 else -1)
    t = len(pairs)
    fq[t:t + 2] = q - 1
    g[t], g[t + 1] = 1, -1
    fq[t + 2:] = rng.integers(0, 65536, (2, N)) % q
    g[t + 2:] = _ternary(rng, (2, N))
    return fq.astype(np.uint16), g.astype(np.int8)


def polymul_rows(N, mod):
    """(a, b): (mod - 1) x^i against (mod - 1) x^j for the spike pairs; two random rows; all mod - 1; all 65535 (unreduced)."""
    pairs, rng = spike_pairs(N), _rng(2, N)
    B = len(pairs) + 4
    a, b = np.zeros((B, N), np.int64), np.zeros((B, N), np.int64)
    for t, (i, j) in enumerate(pairs):
        a[t, i], b[t, j] = mod - 1, mod - 1
    t = len(pairs)
    a[t:t + 2] = rng.integers(0, 65536, (2, N)) % mod
    b[t:t + 2] = rng.integers(0, 65536, (2, N)) % mod
    a[t + 2], b[t + 2] = mod - 1, mod - 1
    a[t + 3], b[t + 3] = 65535, 65535
    return a.astype(np.uint16), b.astype(np.uint16)


H_KINDS = 4                       # per cut: cut; cut and one coefficient changed below it; one changed at min(c, N - 1); a lone one above


def h_cuts(N):
    return sorted({0, N - 17, N - 16, N - 15, N - 2, N - 1, N})


def verify_rows(N, q):
    """The operands of the verify_keys sweep at p = 3 and the rows of each class:
      "pairs"      variant_runners.key_pairs with its seven kinds: all five flag values
      "true"       f = +-x^k for k in spikes(N) with its inverses and h = p fq g: flags 0
      "one_plus"   the same with x^(N-1-k) added to fq and to fp: both remainders are 1 + x^(N-1).  The constant coefficient is 1, so
                   neither is flagged (index.js:159 wants length != 1 AND [0] != 1)
      "last_only"  ... with fq and fp = +-x^(N-1-k) alone: both remainders are x^(N-1), the LAST valid index is the only non-zero one
                   and the constant coefficient is not 1: INVALID_FQ | INVALID_FP hang on index N - 1 alone
      "index_1"    remainder 2 + x of fq (first row) and of fp (second row)
      "constant"   fq and fp twice the inverse, at two k: both remainders are the constant 2, of length 1 and so not flagged -- while
                   the accumulators hold that 2 again as "coefficient N" (the low half's full cyclic sum) where N is no multiple
                   of 32: junk that must not count
      "h"          h cut at h_cuts(N), four kinds per cut, then the zero polynomial; fp arrives unreduced (bytes 0..255)
    h of every row but "pairs" and "h" is the oracle's p fq g of that row's own fq, so that INVALID_H stays clear there.
    Returns ((f, g, fq, fp, h), {class: row indices})."""
    from variant_runners import key_pairs
    p, S, rng = 3, spikes(N), _rng(3, N)
    base = [a.astype(np.int64) for a in key_pairs(rng, N, q, p, 7)]
    cuts = h_cuts(N)
    n_edge, n_h = 3 * len(S) + 4, H_KINDS * len(cuts) + 1
    B = n_edge + n_h
    f, fq, fp = (np.zeros((B, N), np.int64) for _ in range(3))
    g = _ternary(rng, (B, N))
    rows = {"pairs": list(range(7)), "true": [], "one_plus": [], "last_only": [], "index_1": [n_edge - 4, n_edge - 3],
            "constant": [n_edge - 2, n_edge - 1], "h": list(range(n_edge, B))}
    for t, k in enumerate(S):
        s, inv, nxt = (1 if t % 2 else -1), (N - k) % N, (N - 1 - k) % N
        for kind, name in enumerate(("true", "one_plus", "last_only")):
            b = 3 * t + kind
            rows[name].append(b)
            f[b, k] = s
            for arr, mod in ((fq, q), (fp, p)):
                if kind < 2:
                    arr[b, inv] = s % mod
                if kind > 0:
                    arr[b, nxt] = s % mod
    for i, b in enumerate(rows["index_1"]):                       # remainder 2 + x of fq, then of fp; the other inverse is the true one
        k, s = S[len(S) // 2], 1
        inv, up = (N - k) % N, (N - k + 1) % N
        f[b, k] = s
        fq[b, inv], fp[b, inv] = (2 if i == 0 else 1), (2 if i == 1 else 1)
        (fq if i == 0 else fp)[b, up] = 1
    for i, b in enumerate(rows["constant"]):                      # remainder 2 of both inverses
        k, s = (0, S[len(S) // 2 + 1])[i], (1 if i else -1)
        f[b, k] = s
        fq[b, (N - k) % N], fp[b, (N - k) % N] = (2 * s) % q, (2 * s) % p
    for i, b in enumerate(rows["h"]):                             # true keys, g without zeros: p fq g is non-zero at every index
        k, s = S[i % len(S)], (1 if i % 2 else -1)
        f[b, k] = s
        fq[b, (N - k) % N] = s % q
        g[b] = rng.choice([-1, 1], N)
        fp[b] = rng.integers(0, 256, N)
    h = orc.public_key_batch(N, q, p, fq, g).astype(np.int64)     # "h": the remainder every cut is made from
    at = n_edge
    for c in cuts:
        h[at, c:] = 0
        h[at + 1, c:] = 0
        if c > 0:
            h[at + 1, rng.integers(0, c)] ^= 1
        h[at + 2, min(c, N - 1)] = (h[at + 2, min(c, N - 1)] + 1) % q
        h[at + 3, c:] = 0
        if c < N:
            h[at + 3, rng.integers(c, N)] = 1
        at += H_KINDS
    h[at] = 0
    rows = {name: [7 + b for b in idx] if name != "pairs" else idx for name, idx in rows.items()}
    rows["h_cut"] = rows["h"][0:-1:H_KINDS]
    out = [np.concatenate([x, y]) for x, y in zip(base, (f, g, fq, fp, h))]
    dts = (np.int8, np.int8, np.uint16, np.uint8, np.uint16)
    return tuple(a.astype(dt) for a, dt in zip(out, dts)), rows


INVERT_B = 32
INVERT_MIN_UNITS = 4


def inversion_rows(N):
    """INVERT_B ternary f with N // 3 ones and N // 3 - 1 minus-ones."""
    rng, d = _rng(4, N), N // 3
    f = np.zeros((INVERT_B, N), np.int8)
    for b in range(INVERT_B):
        perm = rng.permutation(N)
        f[b, perm[:d]], f[b, perm[d:2 * d - 1]] = 1, -1
    return f


def gf2_is_unit(f_row, N):
    """f is a unit modulo 2 and x^N - 1 iff gcd(f mod 2, x^N + 1) = 1 over GF(2): polynomials as Python integers, bit i = x^i."""
    a = (1 << N) | 1
    b = int.from_bytes(np.packbits(np.asarray(f_row, np.int64) & 1, bitorder="little").tobytes(), "little")
    while b:
        nb = b.bit_length()
        while a.bit_length() >= nb:
            a ^= b << (a.bit_length() - nb)
        a, b = b, a
    return a == 1


_units = {}


def inversion_units(N):
    """Which rows of inversion_rows(N) are units modulo 2."""
    if N not in _units:
        _units[N] = np.array([gf2_is_unit(r, N) for r in inversion_rows(N)])
    return _units[N]
