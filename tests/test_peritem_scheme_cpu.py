"""Build-time checks of the per-item-key encrypt / decrypt (CPU only: hipcc cross-compiles gfx950 without a GPU): the new entry points
are exported, the new translation unit's kernels keep everything in registers and avoid the wide-store hazard, and matrix_peritem.hip
still compiles exactly the kernels it did before its helpers moved into peritem_common.h."""
import ctypes as C
import os
import re
import subprocess

import pytest

import __graft_entry__ as ge

SRC = os.path.join(ge.PKG_DIR, "csrc")
SYMBOLS = ("ntru_encrypt_peritem_batch", "ntru_encrypt_peritem_batch_dev", "ntru_decrypt_peritem_batch", "ntru_decrypt_peritem_batch_dev")


@pytest.fixture(scope="module")
def asm_dir(tmp_path_factory):
    """`make asm` into a fresh directory; returns it."""
    d = str(tmp_path_factory.mktemp("asm_peritem_scheme"))
    out = subprocess.run(["make", "-C", SRC, "asm", "ASMDIR=" + d], capture_output=True, text=True, timeout=1800)
    assert out.returncode == 0, out.stderr[-2000:]
    return d


def _usage(asm_dir, tu):
    return open(os.path.join(asm_dir, tu + ".usage")).read()


def test_symbols_are_exported():
    pkg = ge.build()
    lib = pkg.load_library()
    for s in SYMBOLS:
        assert getattr(lib, s) is not None
    raw = C.CDLL(pkg.engine.library_path())
    for s in SYMBOLS:
        assert hasattr(raw, s), s
    hdr = open(os.path.join(ge.ROOT, "include", "ntru_engine.h")).read()
    for s in SYMBOLS:
        assert re.search(r"\bint %s\(" % s, hdr), s


def test_new_kernels_do_not_spill(asm_dir):
    text = _usage(asm_dir, "matrix_peritem_scheme")
    names = re.findall(r"Function Name: (\S+)", text)
    scratch = [int(x) for x in re.findall(r"ScratchSize \[bytes/lane\]: (\d+)", text)]
    assert len(names) == len(scratch) and len(names) >= 4, (len(names), len(scratch))
    assert not [(n, s) for n, s in zip(names, scratch) if s]
    for must in ("k_encrypt_pi_mILb0", "k_encrypt_pi_mILb1", "k_decrypt_pi_mILb0", "k_decrypt_pi_mILb1"):
        assert any(must in n for n in names), must


def test_no_wide_store_followed_by_a_write_of_its_data_registers(asm_dir):
    """The gfx950 hazard of test_build_quality.py (a buffer_store_dwordx4 whose data registers the very next instruction overwrites can
    store the new value), scanned over the ISA of matrix_peritem_scheme.hip, which that test does not read."""
    lines = open(os.path.join(asm_dir, "matrix_peritem_scheme.s")).read().split("\n")
    kern, bad = None, []
    for i, line in enumerate(lines):
        m = re.match(r"^(_Z\w+):", line)
        if m:
            kern = m.group(1)
        if not re.search(r"\b(buffer|global|flat|scratch)_store_dwordx[34]\b", line):
            continue
        data = re.search(r"v\[(\d+):(\d+)\]", line)
        lo, hi = int(data.group(1)), int(data.group(2))
        j = i + 1
        while j < len(lines) and (lines[j].strip().startswith(";") or not lines[j].strip()):
            j += 1
        nxt = lines[j].strip()
        w = re.match(r"^v_\w+\s+v\[?(\d+)(?::(\d+))?", nxt)
        if w and not nxt.startswith(("v_cmp", "v_cmpx")):
            a = int(w.group(1)); b = int(w.group(2) or a)
            if not (b < lo or a > hi):
                bad.append((kern, line.strip(), nxt))
    assert any(re.match(r"^_Z\w*k_decrypt_pi_m\w*:", l) for l in lines)
    assert not bad, bad[:5]


def test_matrix_peritem_keeps_its_instantiations(asm_dir):
    """Moving the shared helpers into peritem_common.h added or removed no kernel in matrix_peritem.hip, and the new kernels live in
    their own translation unit only."""
    names = sorted(set(re.findall(r"Function Name: (\S+)", _usage(asm_dir, "matrix_peritem"))))
    assert names == sorted(["_Z15k_verify_keys_m5PGeomjPKaS1_PKtPKhS3_lPtS6_PhS7_S6_S6_S7_", "_Z16k_newton_round_m5PGeomjjPKaPtl",
                            "_Z11k_polymul_mILb1EEv5PGeomjPKtS2_lPtS3_", "_Z11k_polymul_mILb0EEv5PGeomjPKtS2_lPtS3_",
                            "_Z16k_product_tern_mILb1EEv5PGeomjjPKtPKalPt", "_Z16k_product_tern_mILb0EEv5PGeomjjPKtPKalPt"]), names
    for tu in ("valu_families", "matrix_encrypt", "matrix_decrypt", "matrix_rowimage", "matrix_peritem", "key_inversion", "ternary_sampler", "elementwise",
               "ntru_generic"):
        assert "_pi_m" not in "".join(re.findall(r"Function Name: (\S+)", _usage(asm_dir, tu))), tu
