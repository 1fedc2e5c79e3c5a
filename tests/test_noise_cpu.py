"""Measuring noise, the parts that need no GPU: every refusal of the four entry points through ctypes with a NULL engine and the order
of the checks, the numpy model of k_noise_m's epilogue (tools/mfma_model.py, noise_*) against a plain numpy reduction, the launcher's
rule and the constants pinned to the kernel source, header / binding / export agreement, the fixture of the unmodified reference, and
the build of matrix_noise.hip."""
import ctypes as C
import importlib.util
import os
import re
import subprocess

import numpy as np
import pytest

import __graft_entry__ as ge
import noise_ref as ref

SRC = os.path.join(ge.PKG_DIR, "csrc")
ERR_ARG, ERR_UNSUPPORTED = 2, 3
FORMS = ["ntru_noise_batch", "ntru_noise_batch_dev", "ntru_noise_packed_batch", "ntru_noise_packed_batch_dev"]


@pytest.fixture(scope="module")
def pkg():
    return ge.build()


@pytest.fixture(scope="module")
def lib(pkg):
    return pkg.load_library()


@pytest.fixture(scope="module")
def model():
    spec = importlib.util.spec_from_file_location("mfma_model", os.path.join(ge.ROOT, "tools", "mfma_model.py"))
    m = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(m)
    return m


# ---- the entry points' checks, with a NULL engine --------------------------------------------------------------------------------------
def _call(lib, form, N, q, f, rows, B, peak, energy):
    ptr = lambda a: a if a is None or isinstance(a, C.c_void_p) else a.ctypes.data_as(C.c_void_p)
    rc = getattr(lib, form)(None, N, q, ptr(f), ptr(rows), B, ptr(peak), ptr(energy))
    return rc, lib.ntru_last_error().decode()


def _valid(form, N=17, B=5):
    """Arguments that pass every check; the rows are large enough for the packed forms too (32 bytes per field element)."""
    return dict(N=N, q=4096, f=np.zeros(1920, np.int8), rows=np.zeros(B * 1920 * 4, np.uint64), B=B, peak=np.zeros(B, np.uint16),
                energy=np.zeros(B, np.uint64))


@pytest.mark.parametrize("form", FORMS)
def test_argument_errors_come_before_the_engine(lib, form):
    who = form.replace("_dev", "") + ": "
    rows_name = "packed" if "packed" in form else "e"
    off4 = np.zeros(6, np.uint64)
    bad = [(dict(B=-1), ERR_ARG, "negative batch size"),
           (dict(N=1), ERR_UNSUPPORTED, "unsupported (N, q)"), (dict(N=1921), ERR_UNSUPPORTED, "unsupported (N, q)"),
           (dict(q=1), ERR_UNSUPPORTED, "unsupported (N, q)"), (dict(q=100), ERR_UNSUPPORTED, "unsupported (N, q)"),
           (dict(q=3), ERR_UNSUPPORTED, "unsupported (N, q)"), (dict(q=131072), ERR_UNSUPPORTED, "unsupported (N, q)"),
           (dict(f=None), ERR_ARG, "NULL buffer (f)"), (dict(rows=None), ERR_ARG, "NULL buffer (%s)" % rows_name),
           (dict(peak=None, energy=None), ERR_ARG, "peak and energy are both NULL"),
           (dict(energy=C.c_void_p(off4.ctypes.data + 4)), ERR_ARG, "energy must be 8-byte aligned"),
           (dict(energy=C.c_void_p(off4.ctypes.data + 2), peak=None), ERR_ARG, "energy must be 8-byte aligned")]
    seen = set()
    for change, code, word in bad:
        args = _valid(form)
        args.update(change)
        rc, msg = _call(lib, form, **args)
        assert rc == code and msg.startswith(who) and word in msg and "engine" not in msg, (change, rc, msg)
        seen.add(msg)
    assert len(seen) == 6                        # B < 0, the domain, one per NULL input, both outputs NULL, the alignment
    # ... and the engine comes last: valid arguments, with either output alone, the corners of the domain, B == 0 without rows
    for change in (dict(), dict(peak=None), dict(energy=None), dict(N=2, q=2), dict(N=1920, q=65536), dict(B=0, f=None, rows=None)):
        args = _valid(form)
        args.update(change)
        rc, msg = _call(lib, form, **args)
        assert rc == ERR_ARG and msg == "engine is NULL", (change, msg)


@pytest.mark.parametrize("form", FORMS)
def test_the_order_of_the_checks(lib, form):
    """Each refusal wins over every one behind it: B < 0, the domain, NULL inputs, both outputs NULL, the alignment, the overlaps, and
    only then the engine."""
    who = form.replace("_dev", "") + ": "
    odd = C.c_void_p(np.zeros(4, np.uint64).ctypes.data + 4)
    v = _valid(form)
    order = [(dict(B=-1), "negative batch size"), (dict(q=100), "unsupported (N, q)"), (dict(f=None), "NULL buffer (f)"),
             (dict(peak=None, energy=None), "peak and energy are both NULL"), (dict(energy=odd), "energy must be 8-byte aligned"),
             (dict(peak=v["rows"]), "peak overlaps")]
    for k, (_, word) in enumerate(order):
        args = dict(v)
        for change, _w in reversed(order[k:]):                            # this failure and every later one at once
            args.update(change)
        rc, msg = _call(lib, form, **args)
        assert msg.startswith(who) and word in msg, (k, word, msg)


@pytest.mark.parametrize("form", FORMS)
def test_overlapping_outputs_are_refused(lib, form):
    N, B = 17, 5
    rows_name = "packed" if "packed" in form else "e"
    row_bytes = 96 if "packed" in form else 2 * N                         # (the packed row: the test below)
    buf = np.zeros(4096, np.uint64)
    raw = buf.view(np.uint8)
    at = lambda byte: C.c_void_p(raw.ctypes.data + byte)
    f, rows, peak, energy = at(0), at(1024), at(8192), at(16384)
    n_in = B * row_bytes
    cases = [(dict(peak=at(1024 + n_in - 2)), "peak overlaps " + rows_name), (dict(peak=at(1024 - 2 * B + 2)), "peak overlaps " + rows_name),
             (dict(energy=at((1024 + n_in - 1) // 8 * 8)), "energy overlaps " + rows_name), (dict(energy=at(1024 - 8 * B + 8)), "energy overlaps " + rows_name),
             (dict(peak=at(N - 1)), "peak overlaps f"), (dict(energy=at(8)), "energy overlaps f"),
             (dict(peak=at(16384 + 8 * B - 2)), "peak overlaps energy"), (dict(peak=at(16384)), "peak overlaps energy"),
             (dict(energy=at(8192 - 8 * B + 8)), "peak overlaps energy")]
    who = form.replace("_dev", "") + ": "
    for change, word in cases:
        args = dict(f=f, rows=rows, peak=peak, energy=energy)
        args.update(change)
        rc, msg = _call(lib, form, N, 4096, args["f"], args["rows"], B, args["peak"], args["energy"])
        assert rc == ERR_ARG and msg == who + word, (word, msg)
    # touching ranges do not overlap, and with B == 0 nothing is read or written: what is left is the engine
    for B_, pk, en in ((B, at(1024 + n_in), at(1024 - 8 * B)), (0, rows, rows)):
        rc, msg = _call(lib, form, N, 4096, f, rows, B_, pk, en)
        assert rc == ERR_ARG and msg == "engine is NULL", msg


def test_the_packed_row_of_the_overlap_test():
    from oracle import ntru_oracle as orc
    assert orc.pack_params(4095, 17)["outputSize"] * 32 == 96


# ---- the model of the epilogue -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("q", [2, 128, 8192])
def test_epilogue_model_equals_numpy(model, q):
    """NT = 1, 3, 4, 16, 17 and 32: waves without a strip, one and two rounds, the widest row; rows with a all 0, all q/2 and all
    q/2 + 1 among random ones; junk in the columns >= N, and low / high that only sum to a modulo q."""
    rng = np.random.default_rng(q)
    for N in (17, 96, 97, 509, 513, 1024, 1023):
        NT, NP = model.tiles(N)
        a = rng.integers(0, q, (32, N))
        a[0], a[1], a[2] = 0, q // 2, (q // 2 + 1) % q
        a[3, :] = 0
        a[3, N - 1] = q // 2                                               # the last valid column alone
        low = rng.integers(-2 ** 20, 2 ** 20, (32, NP))
        high = np.zeros((32, NP), np.int64)
        high[:, :N] = a - low[:, :N] + q * rng.integers(-5, 5, (32, N))
        high[:, N:] = rng.integers(-2 ** 20, 2 ** 20, (32, NP - N))        # junk columns: large, and never to be seen
        peak, energy = model.noise_epilogue(N, q, low, high)
        wp, we = ref.reduce_rows(a, q)
        assert peak.tolist() == wp.tolist() and energy.tolist() == we.tolist(), (N, q)
        assert (peak[0], energy[0]) == (0, 0) and (peak[1], energy[1]) == (q // 2, N * (q // 2) ** 2)
        assert peak[2] == (q // 2 - 1 if q > 2 else 0) and (peak[3], energy[3]) == (q // 2, (q // 2) ** 2)
    assert sorted({model.tiles(N)[0] for N in (17, 96, 97, 509, 513, 1024, 1023)}) == [1, 3, 4, 16, 17, 32]


def test_model_of_the_whole_kernel_on_one_row_block(model):
    rng = np.random.default_rng(11)
    for N, q in ((65, 8192), (33, 128), (130, 4096)):
        f, e = ref.ternary(rng, N), rng.integers(0, q, (32, N))
        e[0], e[1] = 0, q - 1
        peak, energy = model.noise_model(N, q, f, e)
        wp, we = ref.want(N, q, f, e)
        assert peak.tolist() == wp.tolist() and energy.tolist() == we.tolist(), (N, q)


def test_the_slots_are_for_each_strips(model):
    """Slot j is strip j in column order; only NT < 4 leaves waves without a strip, and the count the fold runs to is min(NT, 4 rounds)."""
    for NT in range(1, 33):
        slots = model.noise_strip_slots(NT)
        rounds = -(-(-(-NT // 4)) // 4)
        assert len(slots) == min(NT, 4 * rounds) <= ref.MAX_STRIPS and sum(nt for _, nt in slots) == NT
        assert all(1 <= nt <= 4 for _, nt in slots) and slots[0][0] == 0
        assert all(a[0] + a[1] == b[0] for a, b in zip(slots, slots[1:]))
    src = open(os.path.join(SRC, "matrix_noise.hip")).read()
    assert "g.NT < rounds * WAVES_PER_BLOCK ? g.NT : rounds * WAVES_PER_BLOCK" in src
    assert "wave ^ (2 * blockIdx.x >= gridDim.x ? 2 : 0)" in src           # for_each_strip's swap, restated for the slot index
    common = open(os.path.join(SRC, "matrix_common.h")).read()
    assert "if (!all && 2 * blockIdx.x >= gridDim.x) wave ^= 2;" in common


def test_the_launchers_rule_is_make_mgeoms():
    assert [ref.matrix_range(167, 128, p) for p in range(6)] == [True, False, False, False, True, True]
    assert [ref.matrix_range(33, 4096, p) for p in (0, 4, 5)] == [False, True, True]                # path 0 wants N >= 64
    assert [ref.matrix_range(63, 2, 0), ref.matrix_range(64, 2, 0)] == [False, True]
    assert not ref.matrix_range(167, 16384, 0) and not ref.matrix_range(1025, 4096, 4)
    assert ref.matrix_range(1024, 8192, 0) and ref.matrix_range(2, 2, 5)
    common = open(os.path.join(SRC, "matrix_common.h")).read()
    assert "static inline bool matrix_path_allowed(const ntru_engine *eng) { return eng->path == 0 || eng->path >= 4; }" in common
    assert "if (q > 8192 || N > 1024 || ld > 1024 || N < (eng->path >= 4 || ld != N ? 2 : 64)) return false;" in common
    src = open(os.path.join(SRC, "matrix_noise.hip")).read()
    assert "if (!make_mgeom(eng, N, q, N, mg)) return false;" in src
    const = lambda name: int(re.search(r"constexpr \w+ %s = (\w+);" % name, src).group(1), 0)
    assert const("NOISE_PASS") == ref.PASS == 65536 and const("NOISE_MAX_STRIPS") == ref.MAX_STRIPS == 8


# ---- header, binding, exports ----------------------------------------------------------------------------------------------------------
def test_symbols_are_declared_and_bound(pkg, lib):
    hdr = open(os.path.join(ge.ROOT, "include", "ntru_engine.h")).read()
    for s in FORMS:
        assert hasattr(lib, s) and re.search(r"\bint %s\(" % s, hdr), s
        assert s in pkg.engine._SIGS and len(pkg.engine._SIGS[s][1]) == 8
    for name in ("noise_batch", "noise_batch_dev", "noise_packed_batch", "noise_packed_batch_dev"):
        assert getattr(pkg.noise, name) is getattr(pkg, name)
    assert callable(pkg.NTRU.noiseBatch)
    assert not [c for c in pkg.engine._CALLS if "noise" in c.name] and not [n for n in dir(pkg.Engine) if "noise" in n]
    for word in ("(-q/2, q/2]", "guard band", "q/2 - peak", "wrapped"):
        assert word in hdr, word
    # abi.hip and ntru_host.hip are linked against fixed test doubles by tests/hostcheck: they must not need the new file
    for tu in ("abi.hip", "ntru_host.hip"):
        assert "noise" not in open(os.path.join(SRC, tu)).read(), tu
    shim = open(os.path.join(ge.PKG_DIR, "js", "index.mjs")).read()
    assert re.search(r"^  noiseBatch\(e, B\) \{", shim, flags=re.M)
    doc = open(os.path.join(ge.ROOT, "INTEGRATION.md")).read()
    assert "## Measuring noise" in doc and "guard band" in doc


# ---- the fixture -----------------------------------------------------------------------------------------------------------------------
def test_fixture_is_consistent_with_itself_and_the_oracle():
    sets = ref.load_sets()
    assert os.path.getsize(ref.GOLDEN) < 64 * 1024
    assert [s["set"] for s in sets] == ["n17_q32", "n167_q128_low_noise", "n167_q128_default", "n509_q2048"]
    assert sets[2]["options"] == {"N": 167, "q": 128, "p": 3, "df": 61, "dg": 20, "dr": 18}
    inside = outside = 0
    for st in sets:
        o = st["options"]
        N, q, p = o["N"], o["q"], o["p"]
        f, g = np.array(st["f"]), np.array(st["g"])
        assert (f == 1).sum() == o["df"] and (f == -1).sum() == o["df"] - 1 and (g == 1).sum() == (g == -1).sum() == o["dg"]
        assert [c["K"] for c in st["cases"]] == [1, 2, 4, 8]
        e = np.array([c["e"] for c in st["cases"]], np.uint16)
        rem = ref.rem1(N, q, f.astype(np.int8), e)
        for b, c in enumerate(st["cases"]):
            assert rem[b].tolist() == c["remainder1"], (st["set"], c["K"], "the oracle's rem1 is the reference's remainder1")
            A = ref.plain_A(N, p, f, g, st["r"][:c["K"]], st["m"][:c["K"]])
            assert A.tolist() == c["A"], (st["set"], c["K"], "A recomputed from f, g, r and m")
            assert c["inside"] == bool((2 * A > -q).all() and (2 * A <= q).all())
            assert not ((A - np.array(c["remainder1"])) % q).any(), "a is A modulo q, inside the interval or not"
            pk, en = ref.reduce_rows(np.array([c["remainder1"]]), q)
            if c["inside"]:
                inside += 1
                assert int(pk[0]) == int(np.abs(A).max()) and int(en[0]) == int((A * A).sum())
            else:
                outside += 1
                assert (ref.centred(c["remainder1"], q) != A).any()                             # the wrapped value is not A
    assert inside >= 8 and outside >= 2


# ---- the build -------------------------------------------------------------------------------------------------------------------------
def test_new_kernels_do_not_spill(tmp_path):
    out = subprocess.run(["make", "-C", SRC, "ASMDIR=%s" % tmp_path, "%s/matrix_noise.s" % tmp_path], capture_output=True, text=True,
                         timeout=900)
    assert out.returncode == 0, out.stderr[-2000:]
    text = open(os.path.join(str(tmp_path), "matrix_noise.usage")).read()
    names = re.findall(r"Function Name: (\S+)", text)
    scratch = [int(x) for x in re.findall(r"ScratchSize \[bytes/lane\]: (\d+)", text)]
    assert len(names) == len(scratch) == 2 and not [(n, s) for n, s in zip(names, scratch) if s]
    assert sorted(re.search(r"k_noise_[a-z]+", n).group(0) for n in names) == ["k_noise_m", "k_noise_rows"]
    isa = open(os.path.join(str(tmp_path), "matrix_noise.s")).read()
    meta = isa[isa.index("amdhsa.kernels"):]
    entry = next(e for e in meta.split("  - .agpr_count") if "k_noise_mE" in e)
    assert re.search(r"\.private_segment_fixed_size: 0\b", entry) and re.search(r"\.vgpr_spill_count: +0\b", entry)
    assert int(re.search(r"\.vgpr_count: +(\d+)", entry).group(1)) <= 256      # two workgroups of four waves per CU
    assert "v_mfma_i32_32x32x32_i8" in isa and "ds_swizzle_b32" in isa and "ds_add" not in isa and "ds_max" not in isa
    mk = open(os.path.join(SRC, "Makefile")).read()
    assert re.search(r"^NOISE_SRCS := matrix_noise.hip$", mk, flags=re.M)
    assert "matrix_noise.hip" not in re.search(r"^KERNEL_SRCS := (.*)$", mk, flags=re.M).group(1)
    assert "$(NOISE_SRCS)" in re.search(r"^SRCS := (.*)$", mk, flags=re.M).group(1)
    assert "$(NOISE_SRCS:%.hip=$(ASMDIR)/%.s)" in mk
