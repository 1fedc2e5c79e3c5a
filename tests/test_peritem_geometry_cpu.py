"""tests/peritem_geometry.py without a GPU: its restatement of the per-item matrix kernels' geometry against the constants of
csrc/matrix_peritem.hip and csrc/peritem_common.h, what the sweep N = 64..1024 of tests/test_peritem_geometry_gpu.py reaches, and the
promises of its operand builders at every N."""
import os
import re

import numpy as np

import peritem_geometry as pg

CSRC = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "ntru-circom_amd", "csrc")


def source(name):
    with open(os.path.join(CSRC, name)) as fh:
        return fh.read()


def function_text(text, head):
    """The text of the function whose definition starts with `head`, up to the next line that starts a top-level definition."""
    at = text.index(head)
    end = re.search(r"\n}\n", text[at:])
    return text[at:at + end.end()]


def ints(pattern, text, count=1):
    found = re.findall(pattern, text)
    assert len(found) == count, (pattern, found)
    return [int(x) for x in (found[0] if isinstance(found[0], tuple) else found)]


def test_constants_are_the_source():
    kern, common = source("matrix_peritem.hip"), source("peritem_common.h")
    assert ints(r"constexpr int PI_HALF_BASE = (\d+);", kern) == [pg.PI_HALF_BASE]
    assert ints(r"constexpr int PI_IMG = (\d+);", kern) == [pg.PI_IMG]
    assert ints(r"constexpr int PI_WAVES = (\d+);", common) == [pg.PI_WAVES]
    half = function_text(kern, "static __device__ __forceinline__ void pi_build_array_half(")
    assert ints(r"if \(N >= (\d+)\) \{", half) == [pg.HALF_ONE_STORE_N]
    assert ints(r"behind = ch < (\d+), front = holds && 16 \* ch \+ 15 >= N - (\d+);", half) == [3, pg.FRONT_MARGIN]
    nat = function_text(common, "static __host__ __device__ inline size_t pi_nat_bytes(")
    assert ints(r"\(\(size_t\)(\d+) \* g\.N \+ (\d+) \+ 15\) & ~\(size_t\)15;", nat) == [3, 64]
    assert ints(r"return periods > (\d+) \? periods : (\d+);", nat) == [pg.NAT_MIN_BYTES, pg.NAT_MIN_BYTES]
    wave = function_text(common, "static __host__ __device__ inline size_t pi_wave_bytes(")
    assert "return pi_nat_bytes(g) + (size_t)arrays * 16 * g.tpitch;" in wave
    applies = function_text(common, "static inline bool peritem_applies(")
    assert ints(r"q <= (\d+) && N <= (\d+) && N >= \(eng->path >= (\d+) \? (\d+) : (\d+)\);", applies) == [
        pg.MAX_Q, pg.MAX_N, 4, pg.MIN_N[4], pg.MIN_N[0]]
    geom = function_text(common, "static inline PGeom make_pgeom(")
    assert "pg.NT = (N + 31) / 32; pg.tpitch = ((16 * pg.NT + 31) / 32) * 32 + 8;" in geom
    # the images of two planes do not overlap, and the second one ends inside the natural-order area (P + 32 NT <= 1055)
    assert max(pg.moved_by(N) + 32 * pg.pgeom(N)[0] for N in pg.NS) + 16 <= pg.PI_IMG
    assert all(2 * pg.PI_IMG <= pg.nat_bytes(N) for N in pg.NS)


def test_geometry_holds_at_every_n():
    for N in pg.NS:
        NT, tpitch = pg.pgeom(N)
        P = pg.moved_by(N)
        assert 2 <= NT <= 32 and 32 * (NT - 1) < N <= 32 * NT and 0 <= P <= 31, N
        assert tpitch % 4 == 0 and tpitch >= 8 * NT + 8, N           # pi_build_array_half writes words below 8 NT + 8 of a copy
        pairs, single = pg.split_loop(N)
        assert 2 * pairs + single == NT - 1 and single == (NT % 2 == 0), N
        pairs, tail = pg.cyc_tail(N)
        assert 2 * pairs + (2 if tail == "trip+last" else 1) == NT - 1, N
        one, front, behind = pg.half_array_stores(N)
        assert behind == [0, 1, 2] and len(front) in (3, 4), (N, front)
        assert front == list(range(front[0], (N + 15) // 16)) and 16 * front[0] <= max(N - pg.FRONT_MARGIN, 0), (N, front)
        assert not one or not set(front) & set(behind), N             # one store per lane: a chunk is front or behind there
        assert pg.PI_HALF_BASE - N + 16 * front[0] >= 0, N            # the first front chunk lands inside the area
        assert pg.nat_bytes(N) % 16 == 0 and pg.nat_bytes(N) >= pg.PI_HALF_BASE + 2 * N + 48, N
        assert pg.wave_bytes(N, 2) - pg.wave_bytes(N, 1) == 16 * tpitch, N
        # the comparison with h: the lanes' sets are exactly the coefficients below N
        seen = []
        for lane in range(64):
            valid, left = pg.h_valid(N, lane)
            seen += [16 * lane + 2 * c for c in range(8) if valid >> c & 1] + [16 * lane + 2 * c + 1 for c in range(8) if valid >> (16 + c) & 1]
            assert valid >> 8 & 0xFF == 0 and valid >> 24 == 0, (N, lane)
        assert sorted(seen) == list(range(N)), N
        assert pg.h_valid(N, (N - 1) // 16)[1] == pg.last_lane_left(N), N
        # the last distance cuts P bytes of every row but the last one
        for lane in range(64):
            cut = sum(pg.cyc_keep_bytes(N, lane))
            want = min(max(P - 16 * (lane >> 5), 0), 16) if (lane & 31) <= NT - 2 else 0
            assert cut == want, (N, lane)
        for path in (0, 4):
            assert pg.applies(N, 256, path) == pg.applies(N, 8192, path) == (path in pg.paths(N)), (N, path)
    assert not pg.applies(63, 256, 4) and not pg.applies(127, 256, 0) and not pg.applies(1025, 256, 4)
    assert not pg.applies(512, 16384, 4) and not pg.applies(512, 3, 4) and not pg.applies(512, 256, 1)
    assert pg.paths(127) == [4] and pg.paths(128) == [4, 0]


def test_sweep_reaches_every_class():
    ns = list(pg.NS)
    assert ns[0] == 64 and ns[-1] == 1024 and len(ns) == 961
    # every (NT, P) pair that exists: NT = 2 has N = 64 alone, every other NT all 32 P
    pairs = {(pg.pgeom(N)[0], pg.moved_by(N)) for N in ns}
    assert pairs == {(2, 0)} | {(NT, P) for NT in range(3, 33) for P in range(32)}, len(pairs)
    assert {pg.pgeom(N)[0] % 2 for N in ns} == {0, 1}
    # both branches of pi_build_array_half, both counts of front chunks on each side
    assert {(one, len(front)) for one, front, _ in map(pg.half_array_stores, ns)} == {(False, 3), (False, 4), (True, 3), (True, 4)}
    assert pg.half_array_stores(pg.HALF_ONE_STORE_N - 1)[0] is False and pg.half_array_stores(pg.HALF_ONE_STORE_N)[0] is True
    # below 160 a chunk can be front AND behind (two stores); N = 64 has chunks 1 and 2 in both
    assert set(pg.half_array_stores(64)[1]) & set(pg.half_array_stores(64)[2]) == {1, 2}
    # every `left` from 1 to 16 in the last occupied lane of the h comparison, even non-zero ones among them
    assert {pg.last_lane_left(N) for N in ns} == set(range(1, 17))
    # both sides of the pi_nat_bytes switch
    small = [N for N in ns if pg.nat_bytes(N) == pg.NAT_MIN_BYTES]
    assert small == list(range(64, 747)) and pg.nat_bytes(747) == 2320 and pg.nat_bytes(1024) == 3136
    # the three tail shapes of pi_product_cyc, and the split loop with and without its single trip
    assert {pg.cyc_tail_shape(N) for N in ns} == {"last alone", "trip+last", "pairs, last"}
    assert [N for N in ns if pg.cyc_tail_shape(N) == "last alone"] == [64]
    assert {pg.split_loop(N)[1] for N in ns} == {0, 1} and pg.split_loop(64) == (0, 1)
    # kernel path 0 joins at 128
    assert [N for N in ns if 0 not in pg.paths(N)] == list(range(64, 128))


def test_spikes_keep_their_promises():
    for N in pg.NS:
        S = pg.spikes(N)
        assert all(0 <= k < N for k in S) and len(S) == len(set(S)) >= 8, (N, S)
        assert {0, 1, N - 2, N - 1, pg.moved_by(N)} <= set(S), (N, S)
        pairs = pg.spike_pairs(N)
        assert all(i in S and j in S for i, j in pairs) and len(pairs) == len(set(pairs)), N
        sums = {i + j for i, j in pairs}
        assert {N - 1, N, 2 * N - 2} <= sums, (N, sorted(sums))
        assert any(i + j < N - 1 for i, j in pairs) and sum(i + j >= N for i, j in pairs) >= 4, N
        assert 7 == len(pg.h_cuts(N)) and pg.h_cuts(N)[0] == 0 and pg.h_cuts(N)[-1] == N, N


def test_product_rows_keep_their_promises():
    for N in (64, 65, 127, 160, 747, 1024):
        for q in (2, 256, 8192):
            n = len(pg.spike_pairs(N))
            fq, g = pg.public_key_rows(N, q)
            a, b = pg.polymul_rows(N, q)
            assert fq.shape == g.shape == a.shape == b.shape == (n + 4, N)
            assert fq.max() == q - 1 and set(np.unique(g)) == {-1, 0, 1}
            assert all((fq[t] != 0).sum() == 1 and abs(int(g[t].sum())) == 1 and (g[t] != 0).sum() == 1 for t in range(n))
            assert (fq[n:n + 2] == q - 1).all() and (g[n] == 1).all() and (g[n + 1] == -1).all()
            assert all(a[t, i] == q - 1 == b[t, j] for t, (i, j) in enumerate(pg.spike_pairs(N)))
            assert (a[n + 2] == q - 1).all() and (a[n + 3] == 65535).all() and (b[n + 3] == 65535).all() and a[:n + 3].max() < q
            if q > 2:
                assert len(np.unique(fq[n + 2:])) > 2 and len(np.unique(a[n:n + 2])) > 2
            again = pg.public_key_rows(N, q)
            assert np.array_equal(fq, again[0]) and np.array_equal(g, again[1])


def test_inversion_rows_keep_their_promises():
    """INVERT_B ternary f per N with N // 3 ones and N // 3 - 1 minus-ones, of which at least INVERT_MIN_UNITS are units modulo 2."""
    for N in pg.NS:
        f = pg.inversion_rows(N)
        assert f.shape == (pg.INVERT_B, N) and f.dtype == np.int8, N
        assert ((f == 1).sum(axis=1) == N // 3).all() and ((f == -1).sum(axis=1) == N // 3 - 1).all(), N
        units = int(pg.inversion_units(N).sum())
        assert units >= pg.INVERT_MIN_UNITS, (N, units)
    assert pg.INVERT_MIN_UNITS == 4 and pg.INVERT_B == 32
    # the gcd against the definition on a size where it can be enumerated: f is a unit iff some g has f g = 1 modulo (2, x^7 - 1)
    N = 7
    for a in range(1, 1 << N):
        row = np.array([a >> i & 1 for i in range(N)])
        has_inverse = False
        for b in range(1, 1 << N):
            prod = 0
            for i in range(N):
                if a >> i & 1:
                    prod ^= ((b << i) | (b >> (N - i))) & ((1 << N) - 1)
            if prod == 1:
                has_inverse = True
                break
        assert pg.gf2_is_unit(row, N) == has_inverse, a
