"""A batch times one shared polynomial, the parts that need no GPU: the three-plane arithmetic of k_mul_shared_m (tests/mulshared_ref.py
and tools/mfma_model.py) against the oracle, its constants pinned to the kernel source, the argument checks of the two entry points
through ctypes with a NULL engine, header / binding / export agreement, the fixture of the unmodified reference, and the build of
matrix_mulshared.hip."""
import ctypes as C
import importlib.util
import os
import re
import subprocess

import numpy as np
import pytest

import __graft_entry__ as ge
import mulshared_ref as ref

SRC = os.path.join(ge.PKG_DIR, "csrc")
ERR_ARG, ERR_UNSUPPORTED = 2, 3


@pytest.fixture(scope="module")
def pkg():
    return ge.build()


@pytest.fixture(scope="module")
def lib(pkg):
    return pkg.load_library()


# ---- the planes ------------------------------------------------------------------------------------------------------------------------
def test_digits_rebuild_every_value():
    for q in (2, 64, 128, 256, 2048, 4096, 8192):
        x = np.arange(65536)                                               # unreduced values included
        s0, s1x2 = ref.s_planes(x, q)
        e_lo, e_hi2 = ref.row_planes(x, q)
        assert s0.min() >= -64 and s0.max() <= 63 and s1x2.min() >= 0 and s1x2.max() <= 126
        assert e_lo.min() >= 0 and e_lo.max() <= 127 and e_hi2.min() >= 0 and e_hi2.max() <= 126
        assert not ((s0 + 64 * s1x2 - x) % q).any() and not ((e_lo + 64 * e_hi2 - x) % q).any()
    s0, s1x2 = ref.s_planes(np.array([0, 63, 64, 65, 127, 128, 8192 - 64, 8191]), 8192)
    assert s0.tolist() == [0, 63, -64, -63, -1, 0, -64, -1] and s1x2.tolist() == [0, 0, 2, 2, 2, 2, 0, 0]


@pytest.mark.parametrize("q", [2, 128, 2048, 4096, 8192])
def test_plane_model_equals_the_oracle_on_extreme_rows(q):
    """The rows the issue lists: random, all q - 1, s on every edge of both digits, spikes at 0 and N - 1, unreduced 0xFFFF; and the
    largest partial sums (e = 127 everywhere against s = 127 / s = 64: 2 e_hi s0 and e_lo 2 s1 at their extremes)."""
    rng = np.random.default_rng(q)
    for N in (2, 31, 33, 65, 167):
        sets = ref.operand_sets(N, q, 3, rng)
        sets += [("planted", np.array(ref.pad([q - 1, 64 % q, 127 % q], N)[:N], np.uint16) % q, rng.integers(0, q, (3, N)))]
        sets += [("e_127", np.full(N, v % q, np.uint16), np.full((2, N), 127 % q, np.uint16)) for v in (127, 64, 8191 - 63)]
        for label, s, rows in sets:
            quot, rem = ref.plane_model(N, q, s, rows)
            wq, wr = ref.want(N, q, s, rows)
            assert np.array_equal(quot, wq) and np.array_equal(rem, wr), (N, q, label)


def test_the_largest_sums_at_the_longest_row():
    """N = 1024 of the largest planes (e = 8191: 127 and 126; s = 8127: 63 and 126; s = 8000: -64 and 126): pass B's sum times 64
    reaches 2^30 and the bytes are the oracle's."""
    N, q = 1024, 8192
    for sv in (8127, 8000):
        s, rows = np.full(N, sv, np.uint16), np.full((1, N), 8191, np.uint16)
        s0, s1x2 = ref.s_planes(s, q)
        e_lo, e_hi2 = ref.row_planes(rows, q)
        assert s1x2[0] == 126 and s0[0] in (63, -64) and e_lo[0, 0] == 127 and e_hi2[0, 0] == 126
        quot, rem = ref.plane_model(N, q, s, rows)
        wq, wr = ref.want(N, q, s, rows)
        assert np.array_equal(quot, wq) and np.array_equal(rem, wr), sv
    assert (1024 * (127 * 126 + 126 * 63)) << 6 >= 1 << 30


def test_fragment_model_of_the_strips():
    """tools/mfma_model.py walks the kernel's strips, fragments and diagonal masks: one row block at a size with several strips."""
    spec = importlib.util.spec_from_file_location("mfma_model", os.path.join(ge.ROOT, "tools", "mfma_model.py"))
    model = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(model)
    rng = np.random.default_rng(3)
    for N, q in ((65, 8192), (33, 128)):
        s, rows = ref.edge_s(N, q, rng), rng.integers(0, q, (32, N))
        rows[0], rows[1] = q - 1, 127 % q
        rem, quot = model.mul_shared_model(N, q, s, rows)
        wq, wr = ref.want(N, q, s, rows)
        assert np.array_equal(quot, wq) and np.array_equal(rem, wr), (N, q)


def test_constants_are_the_kernels():
    src = open(os.path.join(SRC, "matrix_mulshared.hip")).read()
    const = lambda name: int(re.search(r"constexpr \w+ %s = (\w+);" % name, src).group(1), 0)
    assert const("MS_RADIX") == ref.RADIX == 128 and const("MS_HALF") == ref.HALF == 64
    assert const("MS_S1_MASK") == ref.S1_MASK == 0x3F and const("MS_CARRY_SHIFT") == ref.CARRY_SHIFT == 6
    assert const("MS_FALLBACK_PASS") == ref.FALLBACK_PASS == 65536
    assert "(s + MS_HALF) & (MS_RADIX - 1)) - MS_HALF" in src and ">> 7) & MS_S1_MASK" in src      # the digits are made of them
    assert "0x007F007Fu" in src and "0x00FE00FEu" in src                                              # e & 127 and 2 (e >> 7), two per dword


def test_the_launchers_rule():
    assert [ref.matrix_range(167, 128, p) for p in range(6)] == [True, False, False, False, True, True]
    assert [ref.matrix_range(33, 4096, p) for p in (0, 4, 5)] == [False, True, True]               # path 0 wants N >= 64
    assert not ref.matrix_range(167, 65536, 0) and not ref.matrix_range(167, 3, 4) and not ref.matrix_range(1025, 4096, 4)
    assert ref.matrix_range(1024, 8192, 0) and ref.matrix_range(2, 2, 5)


# ---- the entry points' checks, with a NULL engine --------------------------------------------------------------------------------------
def _call(lib, form, N, mod, s, rows, B, quot, rem):
    ptr = lambda a: a if a is None or isinstance(a, C.c_void_p) else a.ctypes.data_as(C.c_void_p)
    fn = lib.ntru_mul_shared_batch_dev if form == "dev" else lib.ntru_mul_shared_batch
    rc = fn(None, N, mod, ptr(s), ptr(rows), B, ptr(quot), ptr(rem))
    return rc, lib.ntru_last_error().decode()


@pytest.mark.parametrize("form", ["host", "dev"])
def test_argument_errors_come_before_the_engine(lib, form):
    N, B = 17, 5
    z = lambda *shape: np.zeros(shape, np.uint16)
    bad = [(dict(N=1), ERR_UNSUPPORTED, "unsupported"), (dict(N=1921), ERR_UNSUPPORTED, "unsupported"),
           (dict(mod=1), ERR_UNSUPPORTED, "unsupported"), (dict(mod=100), ERR_UNSUPPORTED, "unsupported"),
           (dict(mod=131072), ERR_UNSUPPORTED, "unsupported"), (dict(B=-1), ERR_ARG, "negative"),
           (dict(s=None), ERR_ARG, "NULL buffer (s)"), (dict(rows=None), ERR_ARG, "NULL buffer (rows)"),
           (dict(rem=None), ERR_ARG, "NULL buffer (rem)")]
    seen = set()
    for change, code, word in bad:
        args = dict(N=N, mod=4096, s=z(N), rows=z(B, N), B=B, quot=z(B, N), rem=z(B, N))
        args.update(change)
        rc, msg = _call(lib, form, **args)
        assert rc == code and msg.startswith("ntru_mul_shared_batch: ") and word in msg and "engine" not in msg, (change, rc, msg)
        seen.add(msg)
    assert len(seen) == 5                                                # B < 0, the domain, and one message per NULL buffer ...
    # ... and the engine comes last: valid arguments, with and without quot, B == 0 with nothing at all
    for args in (dict(quot=z(B, N)), dict(quot=None), dict(B=0, s=None, rows=None, quot=None, rem=None), dict(N=2, mod=2),
                 dict(N=1920, mod=65536), dict(mod=3)):
        full = dict(N=N, mod=4096, s=z(1920), rows=z(B, 1920), B=B, quot=z(B, 1920), rem=z(B, 1920))
        full.update(args)
        rc, msg = _call(lib, form, **full)
        assert rc == ERR_ARG and msg == "engine is NULL", (args, msg)


@pytest.mark.parametrize("form", ["host", "dev"])
def test_overlapping_outputs_are_refused(lib, form):
    N, B = 17, 5
    n = B * N
    buf = np.zeros(8192, np.uint16)
    s, rows, quot, rem = buf[0:N], buf[1000:1000 + n], buf[2000:2000 + n], buf[3000:3000 + n]
    cases = [(dict(rem=buf[1000 + n - 1:1000 + 2 * n - 1]), "rem overlaps rows"), (dict(rem=buf[1000 - n + 1:1001]), "rem overlaps rows"),
             (dict(quot=buf[1000:1000 + n]), "quot overlaps rows"), (dict(rem=buf[N - 1:N - 1 + n]), "rem overlaps s"),
             (dict(quot=buf[0:n]), "quot overlaps s"), (dict(quot=buf[3000 + n - 1:3000 + 2 * n - 1]), "quot overlaps rem"),
             (dict(quot=rem), "quot overlaps rem")]
    for change, word in cases:
        args = dict(s=s, rows=rows, quot=quot, rem=rem)
        args.update(change)
        rc, msg = _call(lib, form, N, 4096, args["s"], args["rows"], B, args["quot"], args["rem"])
        assert rc == ERR_ARG and msg == "ntru_mul_shared_batch: " + word, (word, msg)
    # touching ranges do not overlap, and with B == 0 nothing is read or written: what is left is the engine
    for B_, q_, r_ in ((B, buf[1000 + n:1000 + 2 * n], buf[N:N + n]), (0, rows, rows)):
        rc, msg = _call(lib, form, N, 4096, s, rows, B_, q_, r_)
        assert rc == ERR_ARG and msg == "engine is NULL", msg


# ---- header, binding, exports ----------------------------------------------------------------------------------------------------------
def test_symbols_are_declared_and_bound(pkg, lib):
    hdr = open(os.path.join(ge.ROOT, "include", "ntru_engine.h")).read()
    for s in ("ntru_mul_shared_batch", "ntru_mul_shared_batch_dev"):
        assert hasattr(lib, s) and re.search(r"\bint %s\(" % s, hdr), s
        assert s in pkg.engine._SIGS and len(pkg.engine._SIGS[s][1]) == 8
    assert hdr.index("int ntru_polymul_split_dev(") < hdr.index("int ntru_mul_shared_batch(") < hdr.index("int ntru_split_by_I(")
    assert pkg.shared_product.mul_shared_batch is pkg.mul_shared_batch and pkg.shared_product.mul_shared_batch_dev is pkg.mul_shared_batch_dev
    assert callable(pkg.NTRU.multiplyByPolynomialBatch)
    assert not [c for c in pkg.engine._CALLS if "shared" in c.name]
    assert not [n for n in dir(pkg.Engine) if "mul_shared" in n]
    # abi.hip and ntru_host.hip are linked against fixed test doubles by tests/hostcheck: they must not need the new file
    for tu in ("abi.hip", "ntru_host.hip"):
        assert "mul_shared" not in open(os.path.join(SRC, tu)).read(), tu
    shim = open(os.path.join(ge.PKG_DIR, "js", "index.mjs")).read()
    assert "export function multiplyByPolynomialBatch(" in shim and re.search(r"^  multiplyByPolynomialBatch\(rows, B, poly", shim, flags=re.M)


# ---- the fixture -----------------------------------------------------------------------------------------------------------------------
def test_fixture_of_the_reference_equals_the_oracle_and_the_model():
    sets = ref.load_sets()
    assert os.path.getsize(ref.GOLDEN) < 16 * 1024
    assert [(s["N"], s["q"], len(s["rows"])) for s in sets] == [(17, 32, 3), (33, 4096, 3), (65, 8192, 2), (31, 128, 2)]
    for st in sets:
        N, q = st["N"], st["q"]
        quot, rem = ref.want(N, q, st["s"], st["rows"])
        mq, mr = ref.plane_model(N, q, st["s"], st["rows"])
        for b, c in enumerate(st["cases"]):
            assert len(c["quotient"]) <= N and len(c["remainder"]) <= N
            assert quot[b].tolist() == ref.pad(c["quotient"], N) and rem[b].tolist() == ref.pad(c["remainder"], N), (N, q, b)
            assert mq[b].tolist() == quot[b].tolist() and mr[b].tolist() == rem[b].tolist(), (N, q, b)
        assert {0, 63 % q, 64 % q, 127 % q, q - 1} <= set(st["s"]) and st["rows"][1] == [q - 1] * N


# ---- the build -------------------------------------------------------------------------------------------------------------------------
def test_new_kernels_do_not_spill(tmp_path):
    out = subprocess.run(["make", "-C", SRC, "ASMDIR=%s" % tmp_path, "%s/matrix_mulshared.s" % tmp_path], capture_output=True, text=True,
                         timeout=900)
    assert out.returncode == 0, out.stderr[-2000:]
    text = open(os.path.join(str(tmp_path), "matrix_mulshared.usage")).read()
    names = re.findall(r"Function Name: (\S+)", text)
    scratch = [int(x) for x in re.findall(r"ScratchSize \[bytes/lane\]: (\d+)", text)]
    assert len(names) == len(scratch) == 2 and not [(n, s) for n, s in zip(names, scratch) if s]
    assert sorted(re.search(r"k_mul_shared_[a-z]+", n).group(0) for n in names) == ["k_mul_shared_m", "k_mul_shared_replicate"]
    isa = open(os.path.join(str(tmp_path), "matrix_mulshared.s")).read()
    meta = isa[isa.index("amdhsa.kernels"):]
    entry = next(e for e in meta.split("  - .agpr_count") if "k_mul_shared_mE" in e)
    assert re.search(r"\.private_segment_fixed_size: 0\b", entry) and re.search(r"\.vgpr_spill_count: +0\b", entry)
    assert int(re.search(r"\.vgpr_count: +(\d+)", entry).group(1)) <= 256      # two workgroups of four waves per CU
    assert "v_mfma_i32_32x32x32_i8" in isa
    mk = open(os.path.join(SRC, "Makefile")).read()
    assert re.search(r"^MULSHARED_SRCS := matrix_mulshared.hip$", mk, flags=re.M)
    assert "matrix_mulshared.hip" not in re.search(r"^KERNEL_SRCS := (.*)$", mk, flags=re.M).group(1)
