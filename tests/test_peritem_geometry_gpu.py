"""The per-item matrix kernels of csrc/matrix_peritem.hip (k_verify_keys_m, k_polymul_m<ONE>, k_product_tern_m<ONE>,
k_newton_round_m) at EVERY N from 64 to 1024, on the edge operands of tests/peritem_geometry.py: kernel path 4 at every N and kernel
path 0 from N = 128, one digit plane (q = 256; polymul_split also modulus 2) and two (q = 8192).

Every call must name its kernel, leave the GUARD bytes around every output untouched (outputs start as FILL bytes) and equal
oracle.ntru_oracle bit for bit in every output array.  A call that does not is noted and the range goes on, so that a failure lists
every N it concerns.  What the sweep reaches is asserted without a GPU by tests/test_peritem_geometry_cpu.py."""
import numpy as np
import pytest

import peritem_geometry as pg
from oracle import ntru_oracle as orc
from variant_runners import VK_OUT, Dev, assert_equal, pkg

pytestmark = pytest.mark.gpu

EVERY_N = [r.tolist() for r in np.array_split(np.arange(64, 1025), 20)]
IDS = ["%d-%d" % (r[0], r[-1]) for r in EVERY_N]
QS = (256, 8192)                  # one digit plane, two
INVERT_QS = (8192, 2048, 256)     # Newton schedules (kb -> m): 1, 2, 4, 7, 13; 1, 2, 3, 6, 11; 1, 2, 4, 8


@pytest.fixture(scope="module")
def eng():
    e = pkg.Engine(0)
    yield e
    e.close()


def call(eng, ctx, fn, head, ins, outs):
    """fn(*head, inputs, B, guarded outputs) -> (the kernel it named, the outputs); outs: (shape, dtype) each, B = ins[0].shape[0]."""
    with Dev(eng, guard=True) as d:
        ptrs = [None if o is None else d.out(*o) for o in outs]
        fn(*head, *[d.up(x) for x in ins], ins[0].shape[0], *ptrs)
        name = eng.last_kernel()
        got = [d.get(p, *o) for p, o in zip(ptrs, outs) if p]
        d.guards_intact(ctx)
    return name, got


def runs_of(ns):
    """"64-66 69 72-80" of a set of N."""
    ns, out = sorted(ns), []
    for n in ns:
        if out and out[-1][1] == n - 1:
            out[-1][1] = n
        else:
            out.append([n, n])
    return " ".join("%d" % a if a == b else "%d-%d" % (a, b) for a, b in out)


def sweep(eng, ns, cases):
    """cases(N) yields (ctx, kernel path, run) with run() asserting one call.  Failures are collected over the range."""
    failures, count = [], 0
    try:
        for N in ns:
            for ctx, path, run in cases(N):
                eng.set_kernel_path(path)
                count += 1
                try:
                    run()
                except AssertionError as exc:
                    failures.append((ctx, "path %d" % path, str(exc)[:300]))
    finally:
        eng.set_kernel_path(0)
    assert count >= len(ns)
    assert not failures, "%d of %d calls; N: %s; the first: %r" % (len(failures), count, runs_of({f[0][1] for f in failures}), failures[:4])


@pytest.mark.parametrize("ns", EVERY_N, ids=IDS)
def test_public_key_every_n(eng, ns):
    """k_product_tern_m<ONE> / <false> behind public_key (pi_product_cyc on one and two planes), p = 3 and p = 8: (q - 1) x^i against
    +-x^j over the spike pairs (i + j = N - 1, N, 2 N - 2 among them), all q - 1 against all +1 and all -1, two random rows."""
    def cases(N):
        for q in QS:
            fq, g = pg.public_key_rows(N, q)
            for p in (3, 8):
                want = [orc.public_key_batch(N, q, p, fq, g)]
                for path in pg.paths(N):
                    ctx = ("public_key", N, q, p)

                    def run(ctx=ctx, q=q, p=p, want=want, fq=fq, g=g):
                        name, got = call(eng, ctx, eng.public_key_batch_dev, (ctx[1], q, p), (fq, g), [(fq.shape, np.uint16)])
                        assert name == "k_public_key_m", ("launched", name)
                        assert_equal(got, want, "h")
                    yield ctx, path, run
    sweep(eng, ns, cases)


@pytest.mark.parametrize("ns", EVERY_N, ids=IDS)
def test_polymul_split_every_n(eng, ns):
    """k_polymul_m<true> (moduli 2 and 256) and k_polymul_m<false> (8192): quotient and remainder of (mod - 1) x^i times (mod - 1) x^j
    over the spike pairs (those with i + j >= N put their coefficient into the quotient), random rows, all mod - 1, all 65535."""
    def cases(N):
        for mod in (2,) + QS:
            a, b = pg.polymul_rows(N, mod)
            want = list(orc.polymul_split_batch(N, mod, a % mod, b % mod))
            assert want[0].any() and want[1].any()
            for path in pg.paths(N):
                ctx = ("polymul_split", N, mod)

                def run(ctx=ctx, mod=mod, want=want, a=a, b=b):
                    name, got = call(eng, ctx, eng.polymul_split_dev, (ctx[1], mod), (a, b), [(a.shape, np.uint16)] * 2)
                    assert name == "k_polymul_m", ("launched", name)
                    assert_equal(got, want, "quot, rem")
                yield ctx, path, run
    sweep(eng, ns, cases)


def verify_want(N, q, ins, rows):
    """The oracle's outputs, and what the rows' construction promises of its flags (tests/peritem_geometry.py verify_rows)."""
    want = orc.verify_keys_batch(N, q, 3, *ins)
    fl = want["flags"]
    assert fl[0] == 0 and fl[1] & 1 and fl[2] & 2 and fl[3] & 4 and fl[4] == 7, (N, q, fl[:7])
    assert not fl[rows["true"]].any() and not fl[rows["one_plus"]].any(), (N, q)
    assert (fl[rows["last_only"]] == 3).all() and fl[rows["index_1"]].tolist() == [1, 2], (N, q)
    assert not fl[rows["constant"]].any(), (N, q)
    for name in ("rem_fq", "rem_fp"):                                 # a remainder of length 1 that is not 1
        r = want[name][rows["constant"]]
        assert (r[:, 0] == 2).all() and not r[:, 1:].any(), (N, q, name)
    for name, at in (("rem_fq", N - 1), ("rem_fp", N - 1)):          # the flags of "last_only" hang on the last valid index alone
        r = want[name][rows["last_only"]]
        assert (r[:, at] == 1).all() and (r != 0).sum() == len(r), (N, q, name)
    assert (fl[rows["h_cut"][1:]] & 4 == 0).all() and (fl[[b + 2 for b in rows["h_cut"]]] & 4 != 0).all(), (N, q)
    return [want[k] for k, _ in VK_OUT] + [fl]


@pytest.mark.parametrize("ns", EVERY_N, ids=IDS)
def test_verify_keys_every_n(eng, ns):
    """k_verify_keys_m: variant_runners.key_pairs (all five flag values), true keys f = +-x^k at the spikes, remainders 1 + x^(N-1)
    and x^(N-1) (PiNotOne's last valid index), 2 + x and the constant 2 (PiNotOne's junk at and beyond N) of both inverses, and h cut at 0, N - 17, N - 16, N - 15, N - 2, N - 1, N in
    the four kinds of test_verify_keys_h_comparison_boundaries_and_unreduced_fp plus the zero polynomial, fp unreduced there."""
    def cases(N):
        for q in QS:
            ins, rows = pg.verify_rows(N, q)
            want = verify_want(N, q, ins, rows)
            B = ins[0].shape[0]
            outs = [((B, N), dt) for _, dt in VK_OUT] + [((B,), np.uint8)]
            for path in pg.paths(N):
                ctx = ("verify_keys", N, q)

                def run(ctx=ctx, q=q, want=want, ins=ins, outs=outs):
                    name, got = call(eng, ctx, eng.verify_keys_batch_dev, (ctx[1], q, 3), ins, outs)
                    assert name == "k_verify_keys_m", ("launched", name)
                    assert_equal(got, want, [k for k, _ in VK_OUT] + ["flags"])
                yield ctx, path, run
    sweep(eng, ns, cases)


@pytest.mark.parametrize("ns", EVERY_N, ids=IDS)
def test_invert_key_every_n(eng, ns):
    """k_newton_round_m (both of its pi_product_cyc calls, e's image at offset P) behind invert_key at kernel path 4, on the 32 rows of
    peritem_geometry.inversion_rows at three Newton schedules: the rows with NOT_UNIT_MOD2 clear are exactly the units modulo 2 of the
    CPU module's gcd; on those f fq = 1 modulo q and x^N - 1 by the oracle's product, and fq is byte for byte what kernel path 1 (the
    vector-ALU rounds) gives.  invert_key names no inner kernel: polymul_split at the same N and path taking k_polymul_m is the
    proxy, as in tests/test_peritem_item_loop_gpu.py."""
    def cases(N):
        f = pg.inversion_rows(N)
        units = pg.inversion_units(N)
        assert units.sum() >= pg.INVERT_MIN_UNITS, N
        B = f.shape[0]
        one = np.zeros((int(units.sum()), N), np.uint16); one[:, 0] = 1
        outs = [((B, N), np.uint16), None, ((B,), np.uint8)]
        for q in INVERT_QS:
            ctx = ("invert_key", N, q)
            fq_of = {}

            def run(ctx=ctx, q=q, fq_of=fq_of, path=None):
                name, (fq, flags) = call(eng, ctx, eng.invert_key_batch_dev, (ctx[1], q, 3), (f,), outs)
                assert name == "k_invert_key", ("launched", name)
                assert np.array_equal(flags & pg.FLAG_NOT_UNIT_MOD2 == 0, units) and not (flags & (255 ^ pg.FLAG_NOT_UNIT_MOD2)).any(), (
                    "flags", flags.tolist(), "units", units.astype(int).tolist())
                fq_of[path] = fq[units]
                if path == 4:
                    z = np.zeros((1, N), np.uint16)
                    inner, _ = call(eng, ctx, eng.polymul_split_dev, (ctx[1], q), (z, z), [((1, N), np.uint16)] * 2)
                    assert inner == "k_polymul_m", ("the rounds' rule picks", inner)
                    rem = orc.polymul_split_batch(N, q, (f[units].astype(np.int64) % q).astype(np.uint16), fq_of[4])[1]
                    assert_equal([rem], [one], "f fq")
                else:
                    assert 4 in fq_of, "kernel path 4 failed before"
                    assert_equal([fq_of[4]], [fq_of[1]], "fq at kernel path 4 against kernel path 1")
            yield ctx, 4, lambda run=run: run(path=4)
            yield ctx, 1, lambda run=run: run(path=1)
    sweep(eng, ns, cases)
