"""Re-randomising and shuffling ciphertexts, the parts that need no GPU: the numpy restatement (tests/mix_ref.py) against the fixture of
the unmodified reference and against the literal oracle, the two new symbols in the library, the header and the binding, and the build
of matrix_reencrypt.hip (no spills, no wide-store hazard, matrix_encrypt.hip keeps exactly its two kernels)."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import __graft_entry__ as ge
import mix_ref
from oracle import ntru_oracle as orc

SRC = os.path.join(ge.PKG_DIR, "csrc")
SYMBOLS = ("ntru_reencrypt_batch", "ntru_reencrypt_batch_dev")


@pytest.fixture(scope="module")
def cases():
    return mix_ref.load_cases()


def test_fixture_has_the_sets(cases):
    assert [(c["options"]["N"], c["options"]["q"], c["options"]["dr"]) for c in cases] == [
        (17, 32, 1), (167, 128, 5), (509, 2048, 20), (701, 8192, 30), (167, 128, 18), (821, 4096, 30)]
    assert os.path.getsize(mix_ref.GOLDEN) < 400 * 1024
    for c in cases:
        assert [len(rd["src"]) for rd in c["rounds"]] == [6, 6, 9]
        for rd in c["rounds"][:2]:
            assert sorted(rd["src"].tolist()) == list(range(6))
        assert len(set(c["rounds"][2]["src"].tolist())) < 9          # repeats
        if c["mustRecover"]:
            assert all(rd["recovered"].all() for rd in c["rounds"])
    assert not any(rd["recovered"].any() for rd in cases[5]["rounds"])          # N = 821 / q = 4096: q = 1 (mod 3), the lift is off


def test_restatement_equals_the_reference(cases):
    for c in cases:
        N, q = c["options"]["N"], c["options"]["q"]
        cur = c["e"]
        for rd in c["rounds"]:
            e_out, quot = mix_ref.reencrypt(N, q, c["key"]["h"], rd["r"], cur, rd["src"])
            assert np.array_equal(e_out, rd["remainder"]), c["set"]
            assert np.array_equal(quot, rd["quotient"]), c["set"]
            cur = rd["remainder"]


@pytest.mark.parametrize("N,q,B", [(17, 32, 24), (167, 128, 12), (509, 2048, 1)])
def test_restatement_equals_the_literal_oracle(N, q, B):
    rng = np.random.default_rng(N)
    h = rng.integers(0, q, N)
    r = rng.integers(0, 3, (B, N))
    e = rng.integers(0, 65536, (B + 3, N))            # values >= q among them
    e[0] = 65535
    assert (e >= q).any()
    src = rng.integers(0, B + 3, B)
    src[0] = 0
    e_out, quot = mix_ref.reencrypt(N, q, h, r, e, src)
    for i in range(B):
        oq, orem = orc.polymul_split(r[i].tolist(), h.tolist(), N, q, addend=e[src[i]].tolist())
        assert e_out[i].tolist() == orc.expand(orem, N), i
        assert quot[i].tolist() == orc.expand([x % q for x in oq], N), i
    # an index outside the rows adds nothing
    rz = rng.integers(0, 3, (2, N))
    z_out, z_quot = mix_ref.reencrypt(N, q, h, rz, e, np.array([-1, B + 3]))
    e0, q0 = mix_ref.reencrypt(N, q, h, rz, np.zeros((2, N), np.int64))
    assert np.array_equal(z_out, e0) and np.array_equal(z_quot, q0)


def test_symbols_are_exported_declared_and_bound():
    pkg = ge.build()
    lib = pkg.load_library()
    raw = C.CDLL(pkg.engine.library_path())
    hdr = open(os.path.join(ge.ROOT, "include", "ntru_engine.h")).read()
    for s in SYMBOLS:
        assert getattr(lib, s) is not None
        assert hasattr(raw, s), s
        assert re.search(r"\bint %s\(" % s, hdr), s
        assert s in pkg.engine._SIGS and len(pkg.engine._SIGS[s][1]) == 11
    assert "index.js:87-110" in hdr and "circuits/ntru.circom:188-208" in hdr
    assert pkg.mix.reencrypt_batch is pkg.reencrypt_batch and pkg.mix.reencrypt_batch_dev is pkg.reencrypt_batch_dev
    assert not [c for c in pkg.engine._CALLS if "reencrypt" in c.name]
    assert not [n for n in dir(pkg.Engine) if "reencrypt" in n]
    # abi.hip and ntru_host.hip are linked against fixed test doubles by tests/hostcheck: they must not need the new file
    for tu in ("abi.hip", "ntru_host.hip"):
        assert "reencrypt" not in open(os.path.join(SRC, tu)).read(), tu


def test_null_engine_is_rejected():
    lib = ge.build().load_library()
    assert lib.ntru_reencrypt_batch(None, 17, 32, None, None, None, 1, None, 1, None, None) == 2
    assert lib.ntru_reencrypt_batch_dev(None, 17, 32, None, None, None, 1, None, 1, None, None) == 2
    assert b"NULL" in lib.ntru_last_error()


# ---- the build ----------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def asm_dir(tmp_path_factory):
    """`make asm` into a fresh directory; returns it."""
    d = str(tmp_path_factory.mktemp("asm_mix"))
    out = subprocess.run(["make", "-C", SRC, "asm", "ASMDIR=" + d], capture_output=True, text=True, timeout=1800)
    assert out.returncode == 0, out.stderr[-2000:]
    return d


def _names(asm_dir, tu):
    return re.findall(r"Function Name: (\S+)", open(os.path.join(asm_dir, tu + ".usage")).read())


def test_new_kernels_do_not_spill(asm_dir):
    text = open(os.path.join(asm_dir, "matrix_reencrypt.usage")).read()
    names = re.findall(r"Function Name: (\S+)", text)
    scratch = [int(x) for x in re.findall(r"ScratchSize \[bytes/lane\]: (\d+)", text)]
    assert len(names) == len(scratch) == 3, names
    assert not [(n, s) for n, s in zip(names, scratch) if s]
    for must in ("k_reencrypt_m5MGeom", "k_reencrypt_md5MGeom", "k_add_gathered_rows"):
        assert any(must in n for n in names), must
    # two workgroups of four waves per CU: two waves per SIMD
    occ = [int(x) for x in re.findall(r"Occupancy \[waves/SIMD\]: (\d+)", text)]
    assert all(o >= 2 for o in occ), occ


def test_no_wide_store_followed_by_a_write_of_its_data_registers(asm_dir):
    """The gfx950 hazard of test_build_quality.py (a 16-byte store whose data registers the very next instruction overwrites can store
    the new value), scanned over the ISA of matrix_reencrypt.hip, which that test does not read."""
    lines = open(os.path.join(asm_dir, "matrix_reencrypt.s")).read().split("\n")
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
    assert any(re.match(r"^_Z\w*k_reencrypt_md\w*:", l) for l in lines)
    assert not bad, bad[:5]


def test_matrix_encrypt_keeps_its_two_kernels(asm_dir):
    """Moving the body into matrix_encrypt_body.h added or removed no kernel in matrix_encrypt.hip, and the new kernels live in their own
    translation unit only."""
    assert sorted(set(_names(asm_dir, "matrix_encrypt"))) == sorted(["_Z11k_encrypt_m5MGeomjPKtPKhS3_lPtS4_",
                                                                     "_Z12k_encrypt_md5MGeomjPKtPKhS3_lPtS4_"])
    for fn in sorted(os.listdir(asm_dir)):
        if fn.endswith(".usage") and fn != "matrix_reencrypt.usage":
            assert "k_reencrypt" not in open(os.path.join(asm_dir, fn)).read(), fn
