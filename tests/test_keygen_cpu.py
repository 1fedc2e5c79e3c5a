"""ntru_keygen_batch on the CPU: argument checks happen before any device work, the _dev workspace is bounded in B, and the
kernels of keygen_batch.hip do not spill."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import __graft_entry__ as ge

pkg = ge.load_package()
KEY = np.arange(8, dtype=np.uint32)


@pytest.fixture(scope="module")
def lib():
    ge.build()
    return pkg.load_library()


def call(lib, N=17, q=32, p=3, df=3, dg=2, key=KEY, first=0, tries=10, B=4, dev=False):
    kp = key.ctypes.data_as(C.c_void_p) if key is not None else None
    if dev:
        rc = lib.ntru_keygen_batch_dev(None, N, q, p, df, dg, kp, first, tries, B, *([None] * 8))
    else:
        flags = np.zeros(max(B, 1), np.uint8)
        rc = lib.ntru_keygen_batch(None, N, q, p, df, dg, kp, first, tries, B, None, None, None, None, None, None,
                                   flags.ctypes.data_as(C.c_void_p), None)
    return rc, lib.ntru_last_error().decode()


@pytest.mark.parametrize("dev", [False, True])
@pytest.mark.parametrize("kw,code,msg", [
    (dict(N=1), 3, "2 <= N"), (dict(N=1921), 3, "2 <= N"),
    (dict(q=48), 3, "power of two"), (dict(q=1), 3, "power of two"), (dict(q=32768), 3, "p\\*\\(q-1\\)"),
    (dict(p=2), 3, "p = 3"), (dict(p=5), 3, "p = 3"),
    (dict(df=0), 2, "df"), (dict(df=10), 2, "df"), (dict(dg=9), 2, "dg"), (dict(dg=-1), 2, "dg"),
    (dict(tries=0), 2, "max_tries"), (dict(tries=256), 2, "max_tries"),
    (dict(key=None), 2, "key is NULL"), (dict(B=-1), 2, "negative"),
    (dict(first=(1 << 40) - 3), 2, "2\\^40"), (dict(first=1 << 41, B=0), 2, "2\\^40"),
])
def test_argument_checks(lib, dev, kw, code, msg):
    rc, err = call(lib, dev=dev, **kw)
    assert rc == code, (rc, err)
    assert re.search(msg, err), err


@pytest.mark.parametrize("dev", [False, True])
def test_valid_arguments_reach_the_engine_check(lib, dev):
    """Every parameter passes: the NULL engine is what is refused (no device work was attempted before)."""
    rc, err = call(lib, dev=dev, N=821, q=4096, df=273, dg=273, first=(1 << 40) - 4, B=4)
    assert rc == 2 and "engine is NULL" in err


def test_workspace_is_bounded_in_B(lib):
    def ws(N, B):
        n = C.c_size_t()
        assert lib.ntru_keygen_workspace_bytes(N, B, C.byref(n)) == 0
        return n.value
    assert ws(821, 1) < ws(821, 4096)
    assert ws(821, 4096) == ws(821, 1 << 20) == ws(821, 1 << 40)
    assert ws(821, 1 << 40) < 16 << 20
    assert ws(17, 100) < ws(17, 5000)
    n = C.c_size_t()
    assert lib.ntru_keygen_workspace_bytes(1, 4, C.byref(n)) == 2
    assert lib.ntru_keygen_workspace_bytes(17, -1, C.byref(n)) == 2
    assert lib.ntru_keygen_workspace_bytes(17, 4, None) == 2


def test_new_kernels_do_not_spill(tmp_path):
    """`make asm` of keygen_batch.hip: every kernel reports ScratchSize 0, and the three kernels are there; the fourth, the sampler at
    listed positions, is an instantiation in ternary_sampler.hip, with ScratchSize 0 as well."""
    src = os.path.join(ge.PKG_DIR, "csrc")
    targets = [os.path.join(str(tmp_path), tu + ".s") for tu in ("keygen_batch", "ternary_sampler")]
    out = subprocess.run(["make", "-C", src, "-j2", "ASMDIR=" + str(tmp_path)] + targets, capture_output=True, text=True, timeout=900)
    assert out.returncode == 0, out.stderr[-2000:]

    def usage(tu):
        text = open(os.path.join(str(tmp_path), tu + ".usage")).read()
        names = re.findall(r"Function Name: (\S+)", text)
        scratch = [int(x) for x in re.findall(r"ScratchSize \[bytes/lane\]: (\d+)", text)]
        assert len(names) == len(scratch), names
        return names, scratch

    names, scratch = usage("keygen_batch")
    assert len(names) == 3, names
    for must in ("k_keygen_compact", "k_keygen_scatter", "k_keygen_finalize"):
        assert any(must in n for n in names), must
    assert not any(scratch), list(zip(names, scratch))
    listed = [s for n, s in zip(*usage("ternary_sampler")) if "k_sample_ternary" in n and "ListedItems" in n]
    assert listed == [0], listed


def test_shims_expose_key_generation():
    src = open(os.path.join(ge.PKG_DIR, "ntru.py")).read()
    assert "def generateKeysBatch" in src and "def loadKeyFromBatch" in src
    assert hasattr(pkg.Engine, "keygen_batch") and hasattr(pkg.Engine, "keygen_batch_dev")
