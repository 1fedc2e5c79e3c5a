"""k_invert_key<P, NWC> (csrc/key_inversion.hip) in both fields at every word geometry, on hard keys: the 118 N of inversion_ref.N_LIST
(N < 32; both sides of every register-plane class boundary and of the moves to LDS planes; 1919 and 1920; every N mod 32 with register
planes for both fields, with GF(3) in LDS, with both in LDS), each on the 135 rows of inversion_ref.rows(N) -- two whole blocks and a
partial one, every wave with a zero row (|delta| up to 2N), monomials and dense rows next to random ones, so that the shared word
bounds are set by one lane and needed by another -- with q cycling through 32, 128, 2048, 4096, 8192, 65536 along the list.

Four calls of invert_key_batch_dev per N, outputs between guard bytes:
  1  fq and fp together, every pointer on a 16-byte boundary: blocks 0 and 1 through the whole-block stages, the last 7 rows per coefficient
  2  f one byte off, fq and fp one element off: every block per coefficient
  3  fp alone (d_fq = NULL: k_invert_key<3> on the caller's stream), then fq alone (d_fp = NULL)
  4  the rows grouped by family (other wave-mates set the bounds), the result put back into the order of call 1
Every call names k_invert_key and leaves its guards; NOT_UNIT_MOD2 / NOT_UNIT_MODP are set exactly on the non-units of the reference's
gcd (inversion_ref.is_unit: Python integers as bit planes, neither the kernel's division steps nor the oracle's poly_inv) and no other bit is; units have f fp = 1
modulo 3 and f fq = 1 modulo q by the oracle's product with fp < 3 and fq < q; flagged rows are zero; calls 2 to 4 equal call 1 byte
for byte.  A call that fails is noted and the sweep goes on, so that a failure lists every N it concerns.  What the sweep reaches and
what the rows promise is asserted without a GPU by tests/test_key_inversion_geometry_cpu.py.

Reference work on the CPU per test id, measured on one core (the gcds of about 100 rows per N in both fields, cached per N, and the
oracle's products of one call; calls whose outputs equal an earlier call's reuse its products, the regrouped call pays them again):
    N 2-101     gcds 0.24 s, products 0.02 s        N 845-860    gcds 2.11 s, products 0.59 s
    N 102-117   gcds 0.43 s, products 0.04 s        N 861-1035   gcds 2.47 s, products 0.97 s
    N 118-512   gcds 0.68 s, products 0.07 s        N 1036-1049  gcds 2.20 s, products 0.77 s
    N 703-844   gcds 1.96 s, products 0.67 s        N 1050-1920  gcds 1.86 s, products 0.63 s
(N = 1920 alone: gcds 0.31 s, products 0.26 s.)  On an MI355X host the slowest test id took 2.8 s in all."""
import numpy as np
import pytest

import inversion_ref as ir
from variant_runners import Dev, once, pkg

pytestmark = pytest.mark.gpu

SLICES = ir.slices()
IDS = ["%d-%d" % (s[0], s[-1]) for s in SLICES]
SMALL_QS = (2, 4, 65536)          # no Newton round, one, four
SMALL_NS = (17, 33, 127, 1055)
BOTH = ir.FLAG_NOT_UNIT_MOD2 | ir.FLAG_NOT_UNIT_MODP


@pytest.fixture(scope="module")
def eng():
    assert (pkg.engine.FLAG_NOT_UNIT_MOD2, pkg.engine.FLAG_NOT_UNIT_MODP) == (ir.FLAG_NOT_UNIT_MOD2, ir.FLAG_NOT_UNIT_MODP)
    e = pkg.Engine(0)
    yield e
    e.close()


def runs_of(ns):
    """"64-66 69 72-80" of a set of N."""
    ns, out = sorted(ns), []
    for n in ns:
        if out and out[-1][1] == n - 1:
            out[-1][1] = n
        else:
            out.append([n, n])
    return " ".join("%d" % a if a == b else "%d-%d" % (a, b) for a, b in out)


def invert(eng, ctx, N, q, f, fq=True, fp=True, off=0):
    """One call; `off` = 1 puts f one byte and the outputs one element off a 16-byte boundary.  -> {"fq", "fp", "flags"}"""
    B = f.shape[0]
    with Dev(eng, guard=True) as d:
        df = d.up(f, shift=off)
        dq = d.out((B, N), np.uint16, shift=2 * off) if fq else None
        dp = d.out((B, N), np.uint8, shift=off) if fp else None
        dfl = d.out((B,), np.uint8)
        for ptr in (df, dq, dp):
            assert ptr is None or (ptr % 16 == 0) == (off == 0), (ctx, "alignment", ptr % 16)
        eng.invert_key_batch_dev(N, q, 3, df, B, dq, dp, dfl)
        name = eng.last_kernel()
        got = {"fq": d.get(dq, (B, N), np.uint16) if fq else None, "fp": d.get(dp, (B, N), np.uint8) if fp else None,
               "flags": d.get(dfl, (B,), np.uint8)}
        d.guards_intact(ctx)
    assert name == "k_invert_key", ("launched", name)
    return got


def verify(memo, N, q, f, units, got):
    """The assertions on one call's outputs (of the fields it ran)."""
    flags = got["flags"]
    ran = (ir.FLAG_NOT_UNIT_MOD2 if got["fq"] is not None else 0) | (ir.FLAG_NOT_UNIT_MODP if got["fp"] is not None else 0)
    assert not (flags & (255 ^ ran)).any(), ("flag bits outside", ran, np.nonzero(flags & (255 ^ ran))[0][:8].tolist())
    for P, bit, name, mod in ((2, ir.FLAG_NOT_UNIT_MOD2, "fq", q), (3, ir.FLAG_NOT_UNIT_MODP, "fp", 3)):
        inv = got[name]
        if inv is None:
            continue
        u = units[P]
        wrong = np.nonzero((flags & bit == 0) != u)[0]
        assert not len(wrong), ("units modulo %d" % P, "rows", wrong[:8].tolist(), "flags", flags[wrong[:8]].tolist())
        ok = once(memo, ("inverse", N, mod), lambda: ir.check_inverse(f[u], inv[u], N, mod), f[u], inv[u])
        assert ok.all(), ("f %s != 1 modulo %d" % (name, mod), "rows", np.nonzero(u)[0][~ok][:8].tolist())
        dirty = np.nonzero(inv[~u].any(axis=1))[0]
        assert not len(dirty), ("flagged rows of %s not zero" % name, np.nonzero(~u)[0][dirty][:8].tolist())


def same(base, got, what):
    for name in ("fq", "fp", "flags"):
        if got[name] is not None:
            rows = np.nonzero((got[name] != base[name]).reshape(len(base["flags"]), -1).any(axis=1))[0]
            assert not len(rows), ("%s: %s differs from call 1" % (what, name), "rows", rows[:8].tolist())


def cases(eng, memo, N, q):
    """(ctx, run) for the calls at one (N, q); the later ones compare with what call 1 left in `base`."""
    r, s = ir.rows(N), ir.rows(N, order="sorted")
    u, us = ir.units(N), ir.units(N, order="sorted")
    base = {}

    def call_1(ctx):
        got = invert(eng, ctx, N, q, r.f)
        base.update(got)                                          # (kept even where an assertion fails: the comparisons still say something)
        verify(memo, N, q, r.f, u, got)

    def call_2(ctx):
        got = invert(eng, ctx, N, q, r.f, off=1)
        verify(memo, N, q, r.f, u, got)
        assert base, "call 1 did not return"
        same(base, got, "per coefficient")

    def call_3(ctx):
        got_p = invert(eng, ctx + ("fp alone",), N, q, r.f, fq=False)
        got_q = invert(eng, ctx + ("fq alone",), N, q, r.f, fp=False)
        verify(memo, N, q, r.f, u, got_p)
        verify(memo, N, q, r.f, u, got_q)
        assert base, "call 1 did not return"
        same(base, {"fq": got_q["fq"], "fp": got_p["fp"], "flags": got_p["flags"] | got_q["flags"]}, "one field at a time")
        assert not (got_p["flags"] & got_q["flags"]).any()

    def call_4(ctx):
        got = invert(eng, ctx, N, q, s.f)
        verify(memo, N, q, s.f, us, got)
        assert base, "call 1 did not return"
        same(base, {k: v[r.perm] for k, v in got.items()}, "grouped by family")

    for i, fn in enumerate((call_1, call_2, call_3, call_4)):
        ctx = ("invert_key", N, q, "call %d" % (i + 1))
        yield ctx, (lambda fn=fn, ctx=ctx: fn(ctx))


def sweep(eng, pairs):
    """Every call of every (N, q); failures are collected over the range."""
    failures, count, memo = [], 0, {}
    for N, q in pairs:
        for ctx, run in cases(eng, memo, N, q):
            count += 1
            try:
                run()
            except AssertionError as exc:
                failures.append((ctx, str(exc)[:300]))
    assert count == 4 * len(pairs)
    assert not failures, "%d of %d calls; N: %s; the first: %r" % (len(failures), count, runs_of({f[0][1] for f in failures}), failures[:4])


@pytest.mark.parametrize("ns", SLICES, ids=IDS)
def test_invert_key_both_fields_at_every_word_geometry(eng, ns):
    sweep(eng, [(N, ir.q_of(N)) for N in ns])


@pytest.mark.parametrize("N", SMALL_NS)
def test_invert_key_with_no_one_and_four_newton_rounds(eng, N):
    """q = 2 (the inverse modulo 2 is the result), q = 4 (one round) and q = 65536 (four), per coefficient only (17), on the first
    whole-block N that is odd (33), at the end of the first band (127) and at the last N of the sweep below the largest (1055)."""
    assert N in ir.N_LIST
    sweep(eng, [(N, q) for q in SMALL_QS])
