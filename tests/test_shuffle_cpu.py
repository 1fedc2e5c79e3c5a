"""The mix order drawn on the device, the parts that need no GPU: the restatement (tests/shuffle_ref.py) against the oracle's ChaCha20 block
function and its uniformity on fixed inputs, the five new symbols in the library, the header and the binding, the argument checks that
come before the engine, and the build of permutation.hip (its kernels by name, none with scratch, no wide-store hazard)."""
import ctypes as C
import itertools
import os
import re
import subprocess

import numpy as np
import pytest

import __graft_entry__ as ge
import shuffle_ref as ref
from oracle import ntru_oracle as orc

SRC = os.path.join(ge.PKG_DIR, "csrc")
ARITY = {"ntru_argsort_keys_dev": 4, "ntru_draw_permutation": 6, "ntru_draw_permutation_dev": 6, "ntru_mix_batch": 16,
         "ntru_mix_batch_dev": 16}
KEY = [(i + 1) * 0x01010101 for i in range(8)]
MAX_B = 1 << 24


# ---- symbols --------------------------------------------------------------------------------------------------------------------------
def test_symbols_are_exported_declared_and_bound():
    pkg = ge.build()
    lib = pkg.load_library()
    raw = C.CDLL(pkg.engine.library_path())
    hdr = open(os.path.join(ge.ROOT, "include", "ntru_engine.h")).read()
    for s, n in ARITY.items():
        assert getattr(lib, s) is not None
        assert hasattr(raw, s), s
        assert re.search(r"\bint %s\(" % s, hdr), s
        assert s in pkg.engine._SIGS and len(pkg.engine._SIGS[s][1]) == n, s
    assert not hasattr(raw, "ntru_argsort_keys") and not hasattr(raw, "ntru_reencrypt_host")
    assert "#define NTRU_PERM_NONCE2 0x5045524d" in hdr and "#define NTRU_PERM_MAX_B (1 << 24)" in hdr
    assert "uniform up to ties" in hdr and "B^2 / 2^65" in hdr
    assert pkg.mix.PERM_NONCE2 == ref.PERM_NONCE2 == int.from_bytes(b"PERM", "big") and pkg.mix.PERM_MAX_B == MAX_B
    for name in ("argsort_keys_dev", "draw_permutation", "draw_permutation_dev", "mix_batch", "mix_batch_dev"):
        assert getattr(pkg.mix, name) is getattr(pkg, name)
    assert not [n for n in dir(pkg.Engine) if "perm" in n or "mix_batch" in n]
    assert not [c for c in pkg.engine._CALLS if "perm" in c.name or "mix_batch" in c.name]
    assert callable(pkg.NTRU.mixBatch)
    # abi.hip and ntru_host.hip are linked against fixed test doubles by tests/hostcheck: they must not need the new file
    for tu in ("abi.hip", "ntru_host.hip"):
        text = open(os.path.join(SRC, tu)).read()
        assert "perm" not in text and "mix_batch" not in text and "argsort" not in text, tu


# ---- argument errors ------------------------------------------------------------------------------------------------------------------
def _ptr(a):
    return a.ctypes.data_as(C.c_void_p)


def _off(a, nbytes):
    return C.c_void_p(a.ctypes.data + nbytes)


def test_argsort_argument_errors_come_before_the_engine():
    lib = ge.build().load_library()
    err = lambda: lib.ntru_last_error().decode()
    keys, order = np.zeros(8, np.uint64), np.zeros(12, np.int64)
    call = lambda k, B, o: lib.ntru_argsort_keys_dev(None, k, B, o)
    assert call(_ptr(keys), 4, _ptr(order)) == 2 and "engine is NULL" in err()
    assert call(_ptr(keys), 0, _ptr(order)) == 2 and "engine is NULL" in err()
    assert call(_ptr(keys), -1, _ptr(order)) == 2 and "negative batch" in err()
    assert call(_ptr(keys), MAX_B + 1, _ptr(order)) == 2 and "NTRU_PERM_MAX_B" in err()
    assert call(None, 4, _ptr(order)) == 2 and "NULL buffer" in err()
    assert call(_ptr(keys), 4, None) == 2 and "NULL buffer" in err()
    assert call(_ptr(order), 8, _off(order, 32)) == 2 and "overlap" in err()
    assert call(_ptr(order), 4, _off(order, 32)) == 2 and "engine is NULL" in err()          # adjacent: fine


@pytest.mark.parametrize("sym", ["ntru_draw_permutation", "ntru_draw_permutation_dev"])
def test_draw_argument_errors_come_before_the_engine(sym):
    lib = ge.build().load_library()
    err = lambda: lib.ntru_last_error().decode()
    key, buf = np.array(KEY, np.uint32), np.zeros(16, np.int64)
    call = lambda k, B, s, d, pid=0: getattr(lib, sym)(None, k, pid, B, s, d)
    assert call(_ptr(key), 4, _ptr(buf), _off(buf, 32)) == 2 and "engine is NULL" in err()
    assert call(_ptr(key), 4, _ptr(buf), None, pid=2**64 - 1) == 2 and "engine is NULL" in err()
    assert call(_ptr(key), 4, None, _ptr(buf)) == 2 and "engine is NULL" in err()
    assert call(_ptr(key), 0, None, None) == 2 and "engine is NULL" in err()
    assert call(_ptr(key), 4, None, None) == 2 and "both NULL" in err()
    assert call(_ptr(key), -1, _ptr(buf), None) == 2 and "negative batch" in err()
    assert call(_ptr(key), MAX_B + 1, _ptr(buf), None) == 2 and "NTRU_PERM_MAX_B" in err()
    assert call(None, 4, _ptr(buf), None) == 2 and "key is NULL" in err()
    assert call(_ptr(key), 4, _ptr(buf), _off(buf, 24)) == 2 and "src and dst overlap" in err()
    assert call(_ptr(key), 4, _ptr(buf), _ptr(buf)) == 2 and "src and dst overlap" in err()


def _mix(lib, sym, N=17, q=32, p=3, n1=2, n2=2, B=4, key=True, h=True, e_in=True, r=True, src=True, e_out=True, quot=True, alias=None):
    """One call with every array argument a real host array, so that only the argument under test is wrong.  alias = (a, b, bytes):
    argument a points `bytes` into argument b's array."""
    rows = max(B, 1) if B <= 64 else 1
    arr = {"h": np.zeros(N, np.uint16), "key": np.array(KEY, np.uint32), "e_in": np.zeros((2 * rows, N), np.uint16),
           "r": np.zeros((2 * rows, N), np.uint8), "src": np.zeros(2 * rows, np.int64), "e_out": np.zeros((2 * rows, N), np.uint16),
           "quot": np.zeros((2 * rows, N), np.uint16)}
    on = dict(h=h, key=key, e_in=e_in, r=r, src=src, e_out=e_out, quot=quot)
    a = {k: (_ptr(v) if on[k] else None) for k, v in arr.items()}
    if alias:
        a[alias[0]] = _off(arr[alias[1]], alias[2])
    return getattr(lib, sym)(None, N, q, p, a["h"], a["key"], 2**33 + 5, n1, n2, 2**64 - 1, a["e_in"], B, a["r"], a["src"], a["e_out"],
                             a["quot"])


@pytest.mark.parametrize("sym", ["ntru_mix_batch", "ntru_mix_batch_dev"])
def test_mix_argument_errors_come_before_the_engine(sym):
    """Every one of these is NTRU_ERR_ARG with its own message although the engine is NULL: nothing needs a GPU."""
    lib = ge.build().load_library()
    err = lambda: lib.ntru_last_error().decode()
    dev = sym.endswith("_dev")
    assert _mix(lib, sym) == 2 and "engine is NULL" in err()
    assert _mix(lib, sym, quot=False) == 2 and "engine is NULL" in err()
    assert _mix(lib, sym, B=0) == 2 and "engine is NULL" in err()
    assert _mix(lib, sym, B=-1) == 2 and "negative batch" in err()
    assert _mix(lib, sym, B=MAX_B + 1) == 2 and "NTRU_PERM_MAX_B" in err()
    assert _mix(lib, sym, key=False) == 2 and "key is NULL" in err()
    for missing in ("h", "e_in", "e_out"):
        assert _mix(lib, sym, **{missing: False}) == 2 and "NULL buffer" in err(), missing
    for optional in ("r", "src"):                                    # outputs the _dev form needs and the host form may leave out
        assert _mix(lib, sym, **{optional: False}) == 2 and ("NULL buffer" if dev else "engine is NULL") in err(), optional
    assert _mix(lib, sym, alias=("e_out", "e_in", 17 * 2 * 3)) == 2 and "e_in and e_out overlap" in err()
    assert _mix(lib, sym, alias=("e_out", "e_in", 0)) == 2 and "e_in and e_out overlap" in err()          # in place: src is always given
    assert _mix(lib, sym, alias=("e_out", "e_in", 17 * 2 * 4)) == 2 and "engine is NULL" in err()          # adjacent: fine
    assert _mix(lib, sym, alias=("quot", "e_out", 17 * 2)) == 2 and "e_out and quotE overlap" in err()
    assert _mix(lib, sym, alias=("src", "r", 8)) == 2 and "r and src overlap" in err()
    # what ntru_sample_ternary refuses
    assert _mix(lib, sym, n1=9, n2=9) == 2 and "cannot exceed the array length" in err()
    assert _mix(lib, sym, n1=-1) == 2 and "negative size" in err()
    assert _mix(lib, sym, p=257) == 2 and "p <= 256" in err()
    assert _mix(lib, sym, p=0) == 2 and "p <= 256" in err()


# ---- the build ------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def asm_dir(tmp_path_factory):
    """`make <ASMDIR>/permutation.s` into a fresh directory; returns it."""
    d = str(tmp_path_factory.mktemp("asm_perm"))
    out = subprocess.run(["make", "-C", SRC, d + "/permutation.s", "ASMDIR=" + d], capture_output=True, text=True, timeout=1800)
    assert out.returncode == 0, out.stderr[-2000:]
    return d


def test_new_kernels_are_there_and_do_not_spill(asm_dir):
    text = open(os.path.join(asm_dir, "permutation.usage")).read()
    names = re.findall(r"Function Name: (\S+)", text)
    scratch = [int(x) for x in re.findall(r"ScratchSize \[bytes/lane\]: (\d+)", text)]
    assert len(names) == len(scratch) == 5, names
    assert not [(n, s) for n, s in zip(names, scratch) if s]
    for must in ("k_perm_keys", "k_perm_hist", "k_perm_offsets", "k_perm_scatter", "k_perm_finish"):
        assert any(must in n for n in names), must
    mk = open(os.path.join(SRC, "Makefile")).read()
    assert re.search(r"^PERM_SRCS := permutation\.hip$", mk, flags=re.M) and "permutation.hip" not in re.search(r"^KERNEL_SRCS := .*$", mk, flags=re.M).group(0)


def test_no_wide_store_followed_by_a_write_of_its_data_registers(asm_dir):
    """The gfx950 hazard of test_build_quality.py (a 12- or 16-byte store whose data registers the very next instruction overwrites can
    store the new value), scanned over the ISA of permutation.hip as tests/test_mix_cpu.py scans matrix_reencrypt.hip."""
    lines = open(os.path.join(asm_dir, "permutation.s")).read().split("\n")
    kern, bad = None, []
    for i, line in enumerate(lines):
        m = re.match(r"^(_Z\w+):", line)
        if m:
            kern = m.group(1)
        if not re.search(r"\b(buffer|global|flat|scratch)_store_dwordx[34]\b", line):
            continue
        regs = re.findall(r"v\[(\d+):(\d+)\]", line)
        lo, hi = (int(x) for x in (regs[-1] if line.split()[0].startswith(("global", "flat", "scratch")) else regs[0]))
        j = i + 1
        while j < len(lines) and (lines[j].strip().startswith(";") or not lines[j].strip()):
            j += 1
        nxt = lines[j].strip()
        w = re.match(r"^v_\w+\s+v\[?(\d+)(?::(\d+))?", nxt)
        if w and not nxt.startswith(("v_cmp", "v_cmpx")):
            a = int(w.group(1)); b = int(w.group(2) or a)
            if not (b < lo or a > hi):
                bad.append((kern, line.strip(), nxt))
    assert any(re.match(r"^_Z\w*k_perm_scatter\w*:", l) for l in lines)
    assert not bad, bad[:5]


# ---- the restatement ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("B", [0, 1, 7, 8, 9, 1000])
def test_restatement_returns_a_permutation_and_its_inverse(B):
    keys = ref.perm_keys(KEY, 5, B)
    src, dst = ref.permutation(KEY, 5, B)
    assert keys.dtype == np.uint64 and keys.shape == (B,) and src.dtype == dst.dtype == np.int64
    assert sorted(src.tolist()) == list(range(B))
    assert np.array_equal(dst[src], np.arange(B)) and np.array_equal(src[dst], np.arange(B))
    ranked = keys[src]
    assert all(ranked[j] < ranked[j + 1] or (ranked[j] == ranked[j + 1] and src[j] < src[j + 1]) for j in range(B - 1))


def test_first_block_is_the_chacha20_block():
    w = orc.chacha20_block(KEY, 0, [0, 0, 0x5045524D])
    keys = ref.perm_keys(KEY, 0, 8)
    assert [int(k) for k in keys] == [int(w[2 * j]) | int(w[2 * j + 1]) << 32 for j in range(8)]
    w1 = orc.chacha20_block(KEY, 1, [7, 9, 0x5045524D])
    assert int(ref.perm_keys(KEY, 7 | 9 << 32, 10)[9]) == int(w1[2]) | int(w1[3]) << 32
    # a stable sort keeps index order among equal keys
    src, dst = ref.argsort_inverse(np.array([5, 1, 5, 1, 0], np.uint64))
    assert src.tolist() == [4, 1, 3, 0, 2] and dst.tolist() == [3, 1, 4, 2, 0]


def test_another_id_or_key_gives_another_order():
    base = ref.permutation(KEY, 0, 1000)[0]
    assert not np.array_equal(base, ref.permutation(KEY, 1, 1000)[0])
    assert not np.array_equal(base, ref.permutation(KEY, 1 << 32, 1000)[0])
    assert not np.array_equal(base, ref.permutation([KEY[0] ^ 1] + KEY[1:], 0, 1000)[0])
    assert np.array_equal(base, ref.permutation(KEY, 0, 1000)[0])


def test_orders_of_four_items_are_uniform():
    """B = 4 under perm_id 0 .. 23999: all 24 orders occur, and the chi-square statistic against 1000 each stays below 70.55, the
    1 - 1e-6 quantile at 23 degrees of freedom.  The inputs are fixed, so the test is deterministic (the statistic is 21.29)."""
    count = {o: 0 for o in itertools.permutations(range(4))}
    for perm_id in range(24000):
        count[tuple(ref.permutation(KEY, perm_id, 4)[0].tolist())] += 1
    assert len(count) == 24 and min(count.values()) > 0
    chi2 = sum((c - 1000.0) ** 2 / 1000.0 for c in count.values())
    print("chi-square = %.2f" % chi2)
    assert chi2 < 70.55


def test_mix_restatement_is_the_composition():
    N, q, p, B = 17, 32, 3, 9
    g = np.random.default_rng(3)
    h, e_in = g.integers(0, q, N), g.integers(0, q, (B, N))
    e_out, quot, r, src = ref.mix(N, q, p, h, KEY, 2**33 + 5, 2, 2, 11, e_in)
    assert r.shape == (B, N) and ((r == 1).sum(axis=1) == 2).all() and ((r == 2).sum(axis=1) == 2).all()
    assert np.array_equal(r, orc.sample_ternary_batch(N, 2, 2, 2, KEY, 2**33 + 5, B))
    assert np.array_equal(src, ref.permutation(KEY, 11, B)[0])
    for i in range(B):
        oq, orem = orc.polymul_split(r[i].tolist(), h.tolist(), N, q, addend=e_in[src[i]].tolist())
        assert e_out[i].tolist() == orc.expand(orem, N) and quot[i].tolist() == orc.expand([x % q for x in oq], N), i
