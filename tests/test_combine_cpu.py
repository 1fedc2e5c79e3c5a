"""Combining ciphertexts by a weight matrix, the parts that need no GPU: the digit-plane arithmetic of k_combine_m (tests/combine_ref.py)
against the exact integer product, the argument checks of the two entry points through ctypes with a NULL engine, the ValueErrors of
the Python wrappers, the fixture of the unmodified reference, and the build of matrix_combine.hip."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import __graft_entry__ as ge
import combine_ref as ref

SRC = os.path.join(ge.PKG_DIR, "csrc")
ERR_ARG = 2


@pytest.fixture(scope="module")
def pkg():
    return ge.build()


@pytest.fixture(scope="module")
def lib(pkg):
    return pkg.load_library()


# ---- the digit planes ----------------------------------------------------------------------------------------------------------------
def test_digits_rebuild_every_value_modulo_2_16():
    x = np.arange(65536)
    lo, hi = ref.digits(x)
    assert lo.min() == -128 and lo.max() == 127 and hi.min() == -128 and hi.max() == 127
    assert np.array_equal((lo + 256 * hi) % 65536, x)


def test_plane_model_on_every_row_value():
    """Every one of the 65536 row values against the weights that sit on the digit boundaries, at the widest modulus."""
    mod = 65536
    rows = np.arange(65536, dtype=np.int64).reshape(1, -1)              # B = 1: one product per (weight, value)
    weights = np.array([[0, 1, 127, 128, 255, 256, mod - 1]])
    assert np.array_equal(ref.plane_model(rows, weights, mod), ref.np_combine(rows, weights, mod))


@pytest.mark.parametrize("mod", [2, 128, 2048, 4096, 8192])
def test_plane_model_with_long_contractions(mod):
    """B = 2^18 rows of one column, all-max operands; and operands of 128 (lo = -128, the largest digit product), which make the
    int32 accumulator of the model wrap: 2^18 * 2^14 = 2^32."""
    B = 1 << 18
    for v in sorted({mod - 1, min(128, mod - 1)}):
        rows = np.full((B, 1), v, np.int64)
        weights = np.full((B, 1), v, np.int64)
        assert np.array_equal(ref.plane_model(rows, weights, mod), ref.np_combine(rows, weights, mod)), v
    lo, _ = ref.digits(np.array([min(128, mod - 1)]))
    if mod > 128:
        assert abs(int(lo[0]) ** 2 * B) >= 1 << 31                      # the wrap does happen


def test_plane_model_on_random_operands():
    rng = np.random.default_rng(5)
    for mod in (2, 256, 512, 4096, 65536):
        rows, weights = rng.integers(0, mod, (77, 9)), rng.integers(0, mod, (77, 5))
        assert np.array_equal(ref.plane_model(rows, weights, mod), ref.np_combine(rows, weights, mod)), mod
    assert [ref.planes_of(m) for m in (2, 128, 256, 512, 2048, 8192, 65536)] == [1, 1, 1, 2, 2, 2, 2]


def test_the_launchers_rule():
    assert [ref.kernel_of(4096, p, 3) for p in range(6)] == ["k_combine_m<2,1>", "k_combine_v<1>", "k_combine_v<1>", "k_combine_v<1>",
                                                             "k_combine_m<2,1>", "k_combine_m<2,1>"]
    assert ref.kernel_of(128, 0, 32) == "k_combine_m<1,1>" and ref.kernel_of(256, 4, 33) == "k_combine_m<1,2>"
    assert ref.kernel_of(512, 5, 4096) == "k_combine_m<2,2>" and ref.kernel_of(65521, 0, 3) == "k_combine_v<0>"


# ---- the entry points' checks, with a NULL engine --------------------------------------------------------------------------------------
def _call(lib, form, N, mod, rows, weights, B, G, out):
    ptr = lambda a: a if a is None or isinstance(a, C.c_void_p) else a.ctypes.data_as(C.c_void_p)
    fn = lib.ntru_combine_batch_dev if form == "dev" else lib.ntru_combine_batch
    rc = fn(None, N, mod, ptr(rows), ptr(weights), B, G, ptr(out))
    return rc, lib.ntru_last_error().decode()


@pytest.mark.parametrize("form", ["host", "dev"])
def test_domain_errors_come_before_the_engine(lib, form):
    N, G, B = 17, 3, 5
    rows, weights, out = np.zeros((B, N), np.uint16), np.zeros((B, G), np.uint16), np.zeros((G, N), np.uint16)
    bad = [
        (dict(N=1), "N"), (dict(N=1921), "N"), (dict(mod=1), "mod"), (dict(mod=65537), "mod"), (dict(G=0), "G"), (dict(G=4097), "G"),
        (dict(B=-1), "B"), (dict(B=(1 << 31) + 1), "B"), (dict(rows=None), "NULL"), (dict(weights=None), "NULL"), (dict(out=None), "NULL"),
    ]
    seen = set()
    for change, word in bad:
        args = dict(N=N, mod=4096, rows=rows, weights=weights, B=B, G=G, out=out)
        args.update(change)
        rc, msg = _call(lib, form, **args)
        assert rc == ERR_ARG, (change, msg)
        assert msg.startswith("ntru_combine_batch: ") and word in msg and "engine" not in msg, (change, msg)
        seen.add(msg)
    assert len(seen) >= 7                                                  # messages of their own


@pytest.mark.parametrize("form", ["host", "dev"])
def test_overlapping_out_is_refused(lib, form):
    N, G, B = 17, 3, 5
    buf = np.zeros(4096, np.uint16)
    rows, weights = buf[:B * N], buf[1000:1000 + B * G]
    for out, word in ((buf[B * N - 1:B * N - 1 + G * N], "rows"), (buf[1000 - G * N + 1:1001], "weights"), (buf[0:G * N], "rows"),
                      (buf[1000 + B * G - 1:1000 + B * G - 1 + G * N], "weights")):
        rc, msg = _call(lib, form, N, 4096, rows, weights, B, G, out)
        assert rc == ERR_ARG and "overlaps " + word in msg, msg
    # touching ranges do not overlap: what is left is the engine
    rc, msg = _call(lib, form, N, 4096, rows, weights, B, G, buf[B * N:B * N + G * N])
    assert rc == ERR_ARG and msg == "engine is NULL"
    # B == 0: nothing is read, so nothing can overlap
    rc, msg = _call(lib, form, N, 4096, rows, weights, 0, G, buf[0:G * N])
    assert rc == ERR_ARG and msg == "engine is NULL"


@pytest.mark.parametrize("form", ["host", "dev"])
def test_valid_arguments_reach_the_engine_check(lib, form):
    for N, mod, G, B in ((2, 2, 1, 1), (1920, 65536, 4096, 1), (17, 65521, 3, 5), (17, 4096, 3, 0)):
        rows, weights, out = np.zeros((max(B, 1), N), np.uint16), np.zeros((max(B, 1), G), np.uint16), np.zeros((G, N), np.uint16)
        rc, msg = _call(lib, form, N, mod, rows, weights, B, G, out)
        assert rc == ERR_ARG and msg == "engine is NULL", (N, mod, G, B, msg)
    # B == 0 needs no rows and no weights
    rc, msg = _call(lib, form, 17, 4096, None, None, 0, 3, np.zeros((3, 17), np.uint16))
    assert rc == ERR_ARG and msg == "engine is NULL"
    # B = 2^31 is inside the domain (nothing is read before the engine check)
    rc, msg = _call(lib, "dev", 2, 2, C.c_void_p(1 << 40), C.c_void_p(1 << 50), 1 << 31, 1, C.c_void_p(1 << 30))
    assert rc == ERR_ARG and msg == "engine is NULL"


def test_symbols_are_declared_and_bound(pkg, lib):
    hdr = open(os.path.join(ge.ROOT, "include", "ntru_engine.h")).read()
    for s in ("ntru_combine_batch", "ntru_combine_batch_dev"):
        assert hasattr(lib, s) and re.search(r"\bint %s\(" % s, hdr), s
        assert s in pkg.engine._SIGS and len(pkg.engine._SIGS[s][1]) == 8
    assert "#define NTRU_COMBINE_MAX_G 4096" in hdr and pkg.combine.MAX_G == ref.MAX_G == 4096
    assert pkg.combine.combine_batch is pkg.combine_batch and pkg.combine.combine_batch_dev is pkg.combine_batch_dev
    assert callable(pkg.combineCiphertexts) and callable(pkg.NTRU.combineBatch)
    assert not [c for c in pkg.engine._CALLS if "combine" in c.name]
    assert not [n for n in dir(pkg.Engine) if "combine" in n]
    # abi.hip and ntru_host.hip are linked against fixed test doubles by tests/hostcheck: they must not need the new file
    for tu in ("abi.hip", "ntru_host.hip"):
        assert "combine" not in open(os.path.join(SRC, tu)).read(), tu


# ---- the Python wrappers ---------------------------------------------------------------------------------------------------------------
class _NoEngine:
    """Stands where an Engine would: the wrappers must raise before they touch it."""
    def __getattr__(self, name):
        raise AssertionError("the engine was touched: " + name)


def test_wrappers_refuse_mismatched_row_counts(pkg):
    rows = np.zeros((5, 17), np.uint16)
    with pytest.raises(ValueError, match="4 rows of weights for 5 rows"):
        pkg.combine_batch(_NoEngine(), 17, 4096, rows, np.zeros((4, 3), np.uint16))
    with pytest.raises(ValueError, match="6 rows of weights for 5 rows"):
        pkg.combine_batch(_NoEngine(), 17, 4096, rows, np.zeros(6, np.uint16))
    with pytest.raises(ValueError, match=r"\[B\]\[G\]"):
        pkg.combine_batch(_NoEngine(), 17, 4096, rows, np.zeros((5, 3, 1), np.uint16))
    with pytest.raises(ValueError):
        pkg.combineCiphertexts([[1, 2], [3, 4]], 4096, [[1, 1], [1, 1], [1, 1]], engine=_NoEngine())


# ---- the fixture -----------------------------------------------------------------------------------------------------------------------
def test_fixture_loads_and_equals_the_exact_product():
    sets = ref.load_sets()
    assert os.path.getsize(ref.GOLDEN) < 150 * 1024
    assert [(s["options"]["N"], s["options"]["q"], s["B"]) for s in sets] == [(167, 128, 8), (509, 2048, 8)]
    for s in sets:
        N, q, p, f, fp, rows = ref.set_arrays(s)
        assert [(c["kind"], c["G"]) for c in s["cases"]] == [("memberships", 3), ("small_weights", 2), ("all_ones", 1)]
        m = np.array(s["m"])
        for c in s["cases"]:
            w, sums = ref.case_arrays(s, c)
            assert w.shape == (8, c["G"]) and sums.shape == (c["G"], N)
            assert np.array_equal(ref.np_combine(rows, w, q), sums), (s["set"], c["kind"])
            assert np.array_equal(ref.plane_model(rows, w, q), sums), (s["set"], c["kind"])
            want = (w.astype(np.int64).T @ m) % p
            for g, o in enumerate(c["outputs"]):
                assert ref.pad(o["decrypt"]["inputs"]["e"], N + 1, np.int64)[:N].tolist() == sums[g].tolist()
                assert ref.pad(o["expected"], N, np.int64).tolist() == want[g].tolist()
                assert (ref.pad(o["decrypt"]["value"], N, np.int64).tolist() == want[g].tolist()) == o["recovered"]
        member = s["cases"][0]
        w = np.array(member["weights"])
        assert set(w.ravel().tolist()) == {0, 1} and w[:, 0].all() and np.array_equal(w[:, 1] + w[:, 2], w[:, 0])
    assert all(o["recovered"] for o in sets[1]["cases"][0]["outputs"])      # at least one end-to-end correct tally


# ---- the build -------------------------------------------------------------------------------------------------------------------------
def test_new_kernels_do_not_spill(tmp_path):
    out = subprocess.run(["make", "-C", SRC, "ASMDIR=%s" % tmp_path, "%s/matrix_combine.s" % tmp_path], capture_output=True, text=True,
                         timeout=900)
    assert out.returncode == 0, out.stderr[-2000:]
    text = open(os.path.join(str(tmp_path), "matrix_combine.usage")).read()
    names = re.findall(r"Function Name: (\S+)", text)
    scratch = [int(x) for x in re.findall(r"ScratchSize \[bytes/lane\]: (\d+)", text)]
    assert len(names) == len(scratch) and names
    assert not [(n, s) for n, s in zip(names, scratch) if s]
    assert sorted({re.search(r"k_combine_[a-z]+", n).group(0) for n in names}) == ["k_combine_finish", "k_combine_m", "k_combine_v"]
    isa = open(os.path.join(str(tmp_path), "matrix_combine.s")).read()
    assert "v_mfma_i32_32x32x32_i8" in isa and "global_atomic" not in isa and "flat_atomic" not in isa
    mk = open(os.path.join(SRC, "Makefile")).read()
    assert re.search(r"^COMBINE_SRCS := matrix_combine.hip$", mk, flags=re.M)
    assert "matrix_combine.hip" not in re.search(r"^KERNEL_SRCS := (.*)$", mk, flags=re.M).group(1)
