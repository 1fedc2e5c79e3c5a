"""tests/inversion_ref.py without a GPU: its restatement of launch_invert<P> and of k_invert_key's N-dependent facts against
csrc/key_inversion.hip and the variant table, what N_LIST reaches, is_unit against the oracle's Euclid and against the definition, the
promises and the coverage conditions of rows(N) at every N of the sweep, and the plain-Python division steps of
tests/test_divstep_bounds_cpu.py on the hard rows (so that a bound that is wrong in principle is told from a kernel that applies it
wrongly)."""
import itertools
import os
import re

import numpy as np
import pytest

import inversion_ref as ir
import kernel_variants as kv
from oracle import ntru_keygen as kg
from test_divstep_bounds_cpu import deg, run

SOURCE = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "ntru-circom_amd", "csrc", "key_inversion.hip")
HEADER = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "ntru_engine.h")
MIN_UNITS, MIN_NON_UNITS = 4, 2   # among the random rows (ternary and int8) of every N, in each field
RANDOM = ("ternary", "int8")


def text_of(path):
    with open(path) as fh:
        return fh.read()


def test_classes_and_stage_conditions_are_the_source():
    text = text_of(SOURCE)
    body = text[text.index("static int launch_invert(ntru_engine *eng"):]
    body = body[:body.index("#undef INV_CASE")]
    assert "const int nw = (N + 32) / 32;" in body
    assert "#define INV_CASE(W) if (nw <= W) return launch_invert_nw<P, W>(" in body
    cases = [int(w) for w in re.findall(r"INV_CASE\((\d+)\)", body)]
    extra = re.findall(r"if constexpr \(P == 2\) \{((?: *INV_CASE\(\d+\))+) *\}", body)
    assert len(extra) == 1, extra
    gf2_only = [int(w) for w in re.findall(r"\d+", extra[0])]
    assert tuple(gf2_only) == ir.CLASSES_GF2 and tuple(cases) == ir.CLASSES + ir.CLASSES_GF2, (cases, gf2_only)
    assert cases == sorted(cases)                                 # the first case that fits is the smallest
    assert "return launch_invert_nw<P, 0>(" in text[text.index("#undef INV_CASE"):]
    assert "const int NW = NWC ? NWC : (N + 1 + 31) >> 5;" in text
    assert "const bool whole_in = k0 + 64 <= B && N >= 32 && (((unsigned long long)f & 15) == 0);" in text
    assert ("const bool whole = k0 + 64 <= B && N >= 32 && ((((unsigned long long)out16 | (unsigned long long)out8) & 15) == 0);"
            in text)
    assert (ir.BLOCK, ir.WHOLE_MIN_N, ir.PIECE) == (64, 32, 16)
    assert len(re.findall(r"for \(u32 e = 16u \* \(u32\)lane[^;]*; e < total; e \+= 1024u", text)) == 2      # 64 lanes x 16 elements
    assert "? 1u << (N & 31) : 0u;" in text
    assert "for (int step = 0; step < 2 * N - 1; step++)" in text and "if ((step & 15) == 0) {" in text
    assert "vw_top = word_of((step + mx + 34) >> 1);" in text and "fg_top = word_of((2 * N - 1 - step + mx) >> 1);" in text
    header = text_of(HEADER)
    assert re.search(r"#define NTRU_FLAG_NOT_UNIT_MOD2 %d\b" % ir.FLAG_NOT_UNIT_MOD2, header)
    assert re.search(r"#define NTRU_FLAG_NOT_UNIT_MODP %d\b" % ir.FLAG_NOT_UNIT_MODP, header)
    assert re.search(r"#define NTRU_MAX_N %d\b" % ir.MAX_N, header)


def test_geometry_is_the_launcher_and_the_variant_table():
    for N in range(ir.MIN_N, ir.MAX_N + 1):
        for P in (2, 3):
            g = ir.geometry(N, P)
            assert 32 * (g.NW - 1) <= N < 32 * g.NW and g.top == N - 32 * (g.NW - 1), (N, P)      # coefficient N is in the last word
            if g.cls:
                assert g.NW <= g.cls and g.planes == "registers", (N, P)
                smaller = [W for W in ir.CLASSES + ir.CLASSES_GF2 if W < g.cls]
                assert not smaller or g.NW > smaller[-1], (N, P)
            else:
                assert g.NW > (32 if P == 2 else 26) and g.planes == "LDS", (N, P)
            assert g.straddles == any(e % N + 16 > N for e in range(0, 64 * N, 16)), N         # a piece that ends in the next row
    rows = [r for r in kv.ROWS if r["kernel"].startswith("k_invert_key<")]
    assert len(rows) == 2 * len(ir.CLASSES) + len(ir.CLASSES_GF2) + 2, len(rows)
    for r in rows:
        P, W = (int(x) for x in re.fullmatch(r"k_invert_key<(\d+), (\d+)>", r["kernel"]).groups())
        assert r["shapes"] and all(ir.geometry(s["N"], P).cls == W for s in r["shapes"]), r["kernel"]
    assert ir.whole_block(32, 135, 64, True) and not ir.whole_block(31, 135, 0, True)
    assert not ir.whole_block(32, 135, 128, True) and not ir.whole_block(32, 135, 0, False) and ir.whole_block(32, 128, 64, True)


def test_n_list_reaches_every_class_word_position_and_boundary():
    ns = ir.N_LIST
    assert ns == sorted(set(ns)) and ir.MIN_N == ns[0] and ns[-1] == ir.MAX_N
    assert {2, 3, 15, 16, 17, 31} == {N for N in ns if N < ir.WHOLE_MIN_N} and {32, 33, 1919, 1920} <= set(ns)
    assert ir.class_boundaries() == [64, 192, 384, 512, 704, 832, 1024]
    for N in ir.class_boundaries():
        assert {N - 1, N} <= set(ns), N
        assert any(ir.geometry(N - 1, P).cls != ir.geometry(N, P).cls for P in (2, 3)), N
    assert ir.regime(831) == ir.REGIMES[0] and ir.regime(832) == ir.REGIMES[1] == ir.regime(1023) and ir.regime(1024) == ir.REGIMES[2]
    # every instantiation of the kernel
    assert {(P, ir.geometry(N, P).cls) for N in ns for P in (2, 3)} == (
        {(P, W) for P in (2, 3) for W in ir.CLASSES + (0,)} | {(2, W) for W in ir.CLASSES_GF2})
    # every N mod 32 -- the bit of the top coefficient, and with it every (nf - 16) & 31 of the pieces -- in each regime, on whole blocks
    assert [b[0] for b in ir.bands()] == [96, 832, 1024]
    for r in ir.REGIMES:
        assert {N & 31 for N in ns if ir.regime(N) == r and N >= ir.WHOLE_MIN_N} == set(range(32)), r
        assert {N % ir.PIECE for N in ns if ir.regime(N) == r} == set(range(16)), r
    # each q of the cycle in each regime, and on both sides of N = 128 where the Newton rounds change kernels at kernel path 0
    for r in ir.REGIMES:
        assert {ir.q_of(N) for N in ns if ir.regime(N) == r} == set(ir.QS), r
    assert [N for s in ir.slices() for N in s] == ns and max(len(s) for s in ir.slices()) <= 16
    assert len(ns) == 118


def gf3_has_inverse(f, N):
    one = np.eye(1, N, dtype=np.int64)[0]
    return any(np.array_equal(ir.cyclic_product(f, g, N) % 3, one) for g in itertools.product(range(3), repeat=N))


def test_is_unit_is_the_oracles_and_the_definition():
    rng = np.random.default_rng(5)
    seen = set()
    for t in range(400):
        N = int(rng.integers(2, 41))
        f = rng.integers(-128, 128, N) if t % 4 == 0 else rng.integers(-1, 2, N)
        for P in (2, 3):
            u = ir.is_unit(f, N, P)
            assert u == kg.is_unit(f, N, P), (N, P, f.tolist())
            seen.add((P, u))
    assert len(seen) == 4
    for N in (4, 5):                                              # GF(3) against the definition: some g has f g = 1
        for f in itertools.product((-1, 0, 1), repeat=N):
            assert ir.is_unit(np.array(f), N, 3) == gf3_has_inverse(np.array(f), N), f


def test_rows_keep_their_promises():
    for N in [N for N in ir.N_LIST if N < 200]:
        r, s = ir.rows(N), ir.rows(N, order="sorted")
        assert r.f.shape == s.f.shape == (ir.B, N) and r.f.dtype == np.int8 and ir.B == 135, N
        assert sorted(r.perm.tolist()) == list(range(ir.B)) and np.array_equal(s.perm, np.arange(ir.B)), N
        assert np.array_equal(r.f, s.f[r.perm]) and r.family == [s.family[j] for j in r.perm], N
        assert s.family == sorted(s.family, key=ir.FAMILIES.index), N
        u, us = ir.units(N), ir.units(N, order="sorted")
        for P in (2, 3):
            assert np.array_equal(u[P], us[P][r.perm]), (N, P)
            for i in range(ir.B):
                if s.promise[i] is not None:                      # by construction: True, False, or the status of another row
                    assert us[P][i] == ir.is_unit(s.f[i], N, P), (N, P, i, s.family[i])
        rows_of = lambda name: [s.f[i].astype(np.int64) for i in range(ir.B) if s.family[i] == name]
        mono = rows_of("monomial")
        assert all((m != 0).sum() == 1 and abs(int(m.sum())) == 1 for m in mono), N
        want_k = {k % N for k in (0, 1, 15, 16, 31, 32, N - 2, N - 1) if k < N}
        assert {(int(np.nonzero(m)[0][0]), int(m.sum())) for m in mono} == {(k, sgn) for k in want_k for sgn in (1, -1)}, N
        assert len(rows_of("zero")) == 3 and not any(z.any() for z in rows_of("zero")), N
        assert [int(o[0]) for o in rows_of("ones")] == [1, -1] and all((o == o[0]).all() for o in rows_of("ones")), N
        assert all(t.sum() == 0 and np.abs(t).max() <= 2 for t in rows_of("times_x_minus_1")) and len(rows_of("times_x_minus_1")) == 4, N
        assert bool(rows_of("factor")) == any(N % m == 0 for m in range(2, N)), N
        for t in rows_of("factor"):
            m = next(m for m in range(2, N) if N % m == 0 and np.array_equal(np.roll(t, m), t))
            assert np.abs(t).max() <= 1 and m < N, N             # periodic with a proper divisor: a multiple of 1 + x^m + ...
        low, high = rows_of("dense_low"), rows_of("dense_high")
        ds = [min(max(d or N // 2, 1), N) for d in ir.DENSE_D for _ in range(2)]
        assert len(low) == len(high) == 8, N
        for lo, hi, d in zip(low, high, ds):
            assert lo[d - 1] != 0 and not lo[d:].any() and np.abs(lo).max() == 1, (N, d)
            assert np.array_equal(hi, np.roll(lo, N - d)), (N, d)
        sm = np.array(rows_of("sign_magnitude"))
        assert sm.shape == (len(ir.EDGE_BYTES), N) and all(sorted(sm[:, j].tolist()) == sorted(ir.EDGE_BYTES) for j in range(N)), N
        i8 = np.array(rows_of("int8"))
        assert len(i8) == ir.N_INT8 and (N < 100 or (i8.min() < -120 and i8.max() > 120)), N
        tern = np.array(rows_of("ternary"))
        assert ((tern == 1).sum(axis=1) == max(N // 3, 1)).all() and ((tern == -1).sum(axis=1) == max(N // 3 - 1, 0)).all(), N
        assert len(tern) >= 55, N
        again = ir._build(N)
        assert all(np.array_equal(a[1], b) for a, b in zip(again, s.f)), N


@pytest.mark.parametrize("ns", ir.slices(), ids=["%d-%d" % (s[0], s[-1]) for s in ir.slices()])
def test_every_wave_holds_the_hard_rows_and_the_random_rows_cover_both_outcomes(ns):
    """For every N of the sweep: each of the three waves (rows 0..63, 64..127, 128..134) holds a zero row (delta runs to 2N), a
    monomial and dense rows of both kinds; among the random rows at least MIN_UNITS are units and MIN_NON_UNITS are not, in each
    field.  Where N is a power of two, x^N - 1 = (x - 1)^N modulo 2 and the ternary rows' odd weight makes every one of them a unit
    there: the count is exact."""
    for N in ns:
        r, u = ir.rows(N), ir.units(N)
        for w in range(3):
            fam = set(r.family[64 * w:64 * w + 64])
            assert {"zero", "monomial", "dense_low", "dense_high", "ternary", "int8"} <= fam, (N, w, sorted(fam))
        # ... and the last two waves of the grouped order hold random rows alone: no wave-mate with a large |delta| loosens their bounds
        assert set(ir.rows(N, order="sorted").family[64:]) == set(RANDOM), N
        rnd = np.array([name in RANDOM for name in r.family])
        tern = np.array([name == "ternary" for name in r.family])
        for P in (2, 3):
            assert int((u[P] & rnd).sum()) >= MIN_UNITS and int((~u[P] & rnd).sum()) >= MIN_NON_UNITS, (N, P)
            by_family = {name: u[P][[f == name for f in r.family]] for name in ir.FAMILIES if name in r.family}
            assert by_family["monomial"].all() and not by_family["zero"].any() and not by_family["ones"].any(), (N, P)
            assert not by_family["times_x_minus_1"].any() and not by_family.get("factor", np.zeros(1, bool)).any(), (N, P)
        if N & (N - 1) == 0:
            assert u[2][tern].all() and int(tern.sum()) >= 55, N
            i8 = np.array([name == "int8" for name in r.family])
            assert np.array_equal(u[2][i8], r.f[i8].astype(np.int64).sum(axis=1) % 2 == 1), N


@pytest.mark.parametrize("N,P", [(N, P) for N in (31, 32, 33, 65) for P in (2, 3)])
def test_division_steps_on_the_hard_rows(N, P):
    """The degree bounds at every step, the sampled word bounds with the key's OWN |delta| (the wave's maximum is no smaller, and a
    larger one only loosens them), the final bound that `rest` is collected under, the unit verdict and the inverse as the kernel
    extracts it, on every row of rows(N)."""
    r, u = ir.rows(N), ir.units(N)[P]
    inverses = np.zeros((ir.B, N), np.uint16)
    for b in range(ir.B):
        seen = {}

        def check(n, f, g, v, w, delta):
            assert 2 * deg(f) <= 2 * N - 1 - n + delta and 2 * deg(g) <= 2 * N - 1 - n - delta, (b, r.family[b], n, delta)
            assert 2 * deg(v) <= n - 1 + delta and 2 * deg(w) <= n + 1 - delta, (b, r.family[b], n, delta)
            seen[n] = (abs(delta), max(deg(f), deg(g)), max(deg(v), deg(w)))

        f, v, delta = run(r.f[b].astype(np.int64), N, P, check)
        for n0 in range(0, 2 * N - 1, 16):
            mx = seen[n0][0]
            for n in range(n0, min(n0 + 16, 2 * N - 1)):
                assert seen[n][1] <= (2 * N - 1 - n0 + mx) >> 1, (b, r.family[b], n)
                assert max(seen[n][2], seen[n + 1][2]) <= (n0 + mx + 34) >> 1, (b, r.family[b], n)
        assert max(deg(f), 0) <= abs(delta) >> 1, (b, r.family[b])
        assert (deg(f) == 0 and f[0] != 0) == u[b], (b, r.family[b])
        if r.family[b] == "zero":
            assert delta == 2 * N                                 # the largest |delta| there is: the word bounds of its wave are widest
        if u[b]:
            inverses[b] = (int(f[0]) * v[:N][::-1]) % P
    assert ir.check_inverse(r.f[u], inverses[u], N, P).all()
    assert not ir.check_inverse(r.f[~u][:4], inverses[~u][:4], N, P).any()
