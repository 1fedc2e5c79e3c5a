"""Scanning for decryptable rows, the parts that need no GPU: the restatement (tests/scan_ref.py) against the fixture of the unmodified
reference, the four new symbols in the library, the header and the binding, the argument checks that come before the engine, and the
build of scan_hits.hip (its kernels by name, none with scratch)."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import __graft_entry__ as ge
import lift_ref
import scan_ref

SRC = os.path.join(ge.PKG_DIR, "csrc")
SYMBOLS = ("ntru_scan_bytes_batch", "ntru_scan_bytes_batch_dev", "ntru_scan_bytes_packed_batch", "ntru_scan_bytes_packed_batch_dev")


@pytest.fixture(scope="module")
def cases():
    return scan_ref.load_cases()


def test_fixture_has_the_sets(cases):
    assert [(c["options"]["N"], c["options"]["q"], c["liftRight"]) for c in cases] == [(17, 32, True), (167, 128, True), (167, 256, False)]
    assert os.path.getsize(scan_ref.GOLDEN) < 64 * 1024
    for c in cases:
        assert c["f"].shape == c["fp"].shape == (3, c["options"]["N"]) and c["e"].shape[0] == 11
        assert c["W"] == c["options"]["N"] // 8 and c["tagOffset"] + len(c["tag"]) <= c["W"]
        assert [k["kind"] for k in c["kinds"]].count("arbitrary") == 2
        for k in range(3):
            own = [b for b, kd in enumerate(c["kinds"]) if kd["key"] == k]
            assert sorted(c["kinds"][b]["kind"] for b in own) == ["tagged", "tagged", "wrong_tag"]
            if c["liftRight"]:
                assert c["hit"][k].any() and not c["hit"][k].all()
                assert all(c["hit"][k][b] == (c["kinds"][b]["kind"] == "tagged") for b in own)
            else:
                assert not c["hit"][k][own].any()          # q = 1 (mod 3): index.js:117 does not return the plaintext


def test_restatement_reproduces_every_record(cases):
    for c in cases:
        o = c["options"]
        N, q, p, W = o["N"], o["q"], o["p"], c["W"]
        for k in range(3):
            value = lift_ref.decrypt(N, q, p, c["f"][k], c["fp"][k], c["e"], lift_ref.REFERENCE)[0]
            assert np.array_equal(value, c["value"][k]), (c["set"], k)
        count, rows, data = scan_ref.scan(N, q, p, W, c["f"], c["fp"], c["e"], c["tag"], c["tagOffset"])
        assert count.tolist() == c["hit"].sum(axis=1).tolist(), c["set"]
        for k in range(3):
            assert np.array_equal(rows[k], np.flatnonzero(c["hit"][k])), (c["set"], k)
            assert np.array_equal(rows[k], c["hits"][k][0]) and np.array_equal(data[k], c["hits"][k][1]), (c["set"], k)


def test_centred_lift_recovers_the_honest_rows_of_the_third_set(cases):
    c = cases[2]
    o = c["options"]
    count, rows, _ = scan_ref.scan(o["N"], o["q"], o["p"], c["W"], c["f"], c["fp"], c["e"], c["tag"], c["tagOffset"], mode=lift_ref.CENTRED)
    for k in range(3):
        tagged = [b for b, kd in enumerate(c["kinds"]) if kd == {"key": k, "kind": "tagged"}]
        assert set(tagged) <= set(rows[k].tolist()), k


def test_select_truncates_and_orders():
    data = np.zeros((9, 3), np.uint8)
    data[:, 1] = [7, 7, 0, 7, 7, 7, 0, 7, 7]
    flags = np.array([0, 32, 0, 0, 64, 0, 0, 96, 0], np.uint8)
    count, rows, kept = scan_ref.select(data, flags, b"\x07", 1)
    assert count == 4 and rows.tolist() == [0, 3, 5, 8] and np.array_equal(kept, data[rows])
    assert scan_ref.select(data, flags, b"\x07", 1, max_hits=2)[1].tolist() == [0, 3]
    assert scan_ref.select(data, flags, b"\x07", 1, max_hits=0)[0] == 4
    assert scan_ref.select(data, flags)[1].tolist() == [0, 2, 3, 5, 6, 8]


def test_symbols_are_exported_declared_and_bound():
    pkg = ge.build()
    lib = pkg.load_library()
    raw = C.CDLL(pkg.engine.library_path())
    hdr = open(os.path.join(ge.ROOT, "include", "ntru_engine.h")).read()
    for s in SYMBOLS:
        assert getattr(lib, s) is not None
        assert hasattr(raw, s), s
        assert re.search(r"\bint %s\(" % s, hdr), s
        assert s in pkg.engine._SIGS and len(pkg.engine._SIGS[s][1]) == 17
    assert "#define NTRU_SCAN_MAX_TAG 32" in hdr and "index.js:84-86" in hdr and "index.js:111-140" in hdr
    for name in ("scan_bytes_batch", "scan_bytes_batch_dev", "scan_bytes_packed_batch", "scan_bytes_packed_batch_dev"):
        assert getattr(pkg.scan, name) is getattr(pkg, name)
    assert pkg.scan.MAX_TAG == 32
    assert not [c for c in pkg.engine._CALLS if "scan" in c.name]
    assert not [n for n in dir(pkg.Engine) if "scan" in n]
    assert callable(pkg.NTRU.scanBytes) and callable(pkg.NTRU.scanPacked)
    # abi.hip and ntru_host.hip are linked against fixed test doubles by tests/hostcheck: they must not need the new file
    for tu in ("abi.hip", "ntru_host.hip"):
        assert "scan" not in open(os.path.join(SRC, tu)).read(), tu


def _call(lib, sym, eng=None, N=167, q=128, p=3, nbytes=20, K=1, B=4, tag_off=0, tag_len=4, max_hits=0, bufs=False, count=True):
    """One call with every array argument a real host array, so that only the argument under test is wrong."""
    f, fp = np.zeros((max(K, 1), N), np.int8), np.zeros((max(K, 1), N), np.uint8)
    rows = np.zeros((max(B, 1), 4 * N), np.uint16)
    tag = np.zeros(64, np.uint8)
    hr, hb = np.zeros((max(K, 1), 8), np.int64), np.zeros((max(K, 1), 8, N), np.uint8)
    cnt = np.zeros(max(K, 1), np.int64)
    ptr = lambda a: a.ctypes.data_as(C.c_void_p)
    return getattr(lib, sym)(eng, N, q, p, nbytes, K, ptr(f), ptr(fp), ptr(rows), B, tag_off, tag_len, ptr(tag), max_hits,
                             ptr(hr) if bufs else None, ptr(hb) if bufs else None, ptr(cnt) if count else None)


@pytest.mark.parametrize("sym", SYMBOLS)
def test_argument_errors_come_before_the_engine(sym):
    """Every one of these is NTRU_ERR_ARG with its own message although the engine is NULL: nothing needs a GPU."""
    lib = ge.build().load_library()
    err = lambda: lib.ntru_last_error().decode()
    assert _call(lib, sym) == 2 and "engine is NULL" in err()
    assert _call(lib, sym, tag_len=33) == 2 and "tag_len" in err()
    assert _call(lib, sym, tag_len=-1) == 2 and "tag_len" in err()
    assert _call(lib, sym, tag_off=17, tag_len=4) == 2 and "does not lie inside" in err()
    assert _call(lib, sym, tag_off=-1, tag_len=0) == 2 and "does not lie inside" in err()
    assert _call(lib, sym, tag_off=16, tag_len=4) == 2 and "engine is NULL" in err()          # ends at nbytes: fine
    assert _call(lib, sym, K=0) == 2 and "K >= 1" in err()
    assert _call(lib, sym, max_hits=-1) == 2 and "max_hits" in err()
    assert _call(lib, sym, max_hits=8) == 2 and "NULL hit buffer" in err()
    assert _call(lib, sym, max_hits=8, bufs=True) == 2 and "engine is NULL" in err()
    assert _call(lib, sym, count=False) == 2 and "count is NULL" in err()
    assert _call(lib, sym, nbytes=21) == 2 and "nbytes" in err()
    assert _call(lib, sym, B=-1) == 2 and "negative batch" in err()


# ---- the build ----------------------------------------------------------------------------------------------------------------------
def test_new_kernels_are_there_and_do_not_spill(tmp_path):
    """`make <ASMDIR>/scan_hits.s` into a fresh directory: the three select kernels by name, ScratchSize 0 for every kernel of the file."""
    d = str(tmp_path)
    out = subprocess.run(["make", "-C", SRC, d + "/scan_hits.s", "ASMDIR=" + d], capture_output=True, text=True, timeout=1800)
    assert out.returncode == 0, out.stderr[-2000:]
    text = open(os.path.join(d, "scan_hits.usage")).read()
    names = re.findall(r"Function Name: (\S+)", text)
    scratch = [int(x) for x in re.findall(r"ScratchSize \[bytes/lane\]: (\d+)", text)]
    assert len(names) == len(scratch) == 3, names
    assert not [(n, s) for n, s in zip(names, scratch) if s]
    for must in ("k_scan_mark", "k_scan_offsets", "k_scan_emit"):
        assert any(must in n for n in names), must
