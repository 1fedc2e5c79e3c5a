"""Auditing a mix, the parts that need no GPU: the numpy restatement (tests/audit_ref.py) against the fixture of the unmodified reference,
the opening and the structural checks of an RPC round, the two new symbols in the library, the header and the binding, the refusals, and
the build of mix_audit.hip (no spills, no wide-store hazard)."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import __graft_entry__ as ge
import audit_ref
import mix_ref

SRC = os.path.join(ge.PKG_DIR, "csrc")
SYMBOLS = ("ntru_check_links_batch", "ntru_check_links_batch_dev")


@pytest.fixture(scope="module")
def cases():
    return mix_ref.load_cases()


def test_recorded_rounds_are_links_that_hold(cases):
    """Every round of the fixture, the two sets that do not decrypt included: the links (src[i], i, r[i]) from its input to its recorded
    remainder hold, with the counts the reference's sampler keeps; one coefficient changed anywhere flags that link only."""
    rng = np.random.default_rng(11)
    for c in cases:
        N, q, dr, h = c["options"]["N"], c["options"]["q"], c["options"]["dr"], c["key"]["h"]
        cur = c["e"]
        for rd in c["rounds"]:
            r, src, out = rd["r"], rd["src"], rd["remainder"]
            L = len(src)
            kw = dict(in_idx=src, other=c["options"]["p"] - 1, n1=dr, n2=dr)
            flags, n_bad = audit_ref.check_links(N, q, h, r, cur, out, **kw)
            assert not flags.any() and n_bad == 0, c["set"]
            l, k = int(rng.integers(L)), int(rng.integers(N))
            want = np.zeros(L, np.uint8)
            want[l] = audit_ref.MISMATCH
            e2 = out.copy()
            e2[l, k] = (e2[l, k] + 1) % q
            assert audit_ref.check_links(N, q, h, r, cur, e2, **kw)[0].tobytes() == want.tobytes()
            e1 = cur.copy()
            e1[src[l], k] = (e1[src[l], k] + q - 1) % q
            hit = np.where(src == src[l], audit_ref.MISMATCH, 0).astype(np.uint8)          # a repeated source row is every link that uses it
            assert audit_ref.check_links(N, q, h, r, e1, out, **kw)[0].tobytes() == hit.tobytes()
            r2 = r.copy()
            r2[l, k] = (r2[l, k] + 1) % 3                                               # stays in the domain: a count goes off
            want[l] = audit_ref.BAD_R
            assert audit_ref.check_links(N, q, h, r2, cur, out, **kw)[0].tobytes() == want.tobytes()
            want[l] = audit_ref.MISMATCH
            assert audit_ref.check_links(N, q, h, r2, cur, out, in_idx=src)[0].tobytes() == want.tobytes()      # counts not asked for
            r2[l, k] = 3
            want[l] = audit_ref.BAD_R
            assert audit_ref.check_links(N, q, h, r2, cur, out, in_idx=src)[0].tobytes() == want.tobytes()
            cur = out


def test_flag_rule_of_the_restatement():
    N, q = 17, 32
    g = np.random.default_rng(3)
    h, r, e_in = g.integers(0, q, N), g.integers(0, 3, (6, N)), g.integers(0, 65536, (4, N))
    i, o = np.array([0, 1, 2, 3, 4, -1]), np.array([5, 4, 3, 2, 1, 0])
    e_out = np.zeros((6, N), np.int64)
    e_out[o[:4]] = mix_ref.reencrypt(N, q, h, r[:4], e_in, i[:4])[0]
    e_out[4] += q                                                       # q added still matches
    r[1, 5] = 7
    flags, n_bad = audit_ref.check_links(N, q, h, r, e_in, e_out + q * (e_out < 65536 - q), i, o)
    assert flags.tolist() == [0, audit_ref.BAD_R, 0, 0, audit_ref.BAD_INDEX, audit_ref.BAD_INDEX] and n_bad == 3
    r[5, 0] = 9                                                         # both bits, and never MISMATCH with them
    assert audit_ref.check_links(N, q, h, r, e_in, e_out, i, o)[0][5] == audit_ref.BAD_INDEX | audit_ref.BAD_R
    ones = np.ones((2, N), np.int64)
    assert audit_ref.r_is_bad(ones, 1, 10, 7).tolist() == [False, False] and audit_ref.r_is_bad(ones, 1, 10, 6).all()
    assert not audit_ref.r_is_bad(ones, 1, -1, 6).any()


def test_open_links_and_the_structural_checks():
    pkg = ge.build()
    N, q, B = 17, 32, 12
    g = np.random.default_rng(8)
    h, e0 = g.integers(0, q, N), g.integers(0, q, (B, N))
    r1, r2 = g.integers(0, 3, (B, N)), g.integers(0, 3, (B, N))
    src1, src2 = g.permutation(B), g.permutation(B)
    e1 = mix_ref.reencrypt(N, q, h, r1, e0, src1)[0]
    e2 = mix_ref.reencrypt(N, q, h, r2, e1, src2)[0]
    side = g.integers(0, 2, B)
    side[:2] = [0, 1]
    left, right = pkg.audit.open_links(side, src1, r1, src2, r2)
    ref_left, ref_right = audit_ref.open_links(side, src1, r1, src2, r2)
    for got, want in ((left, ref_left), (right, ref_right)):
        for a, b in zip(got, want):
            assert np.array_equal(np.asarray(a), b)
    assert audit_ref.structure_ok(side, left, right) and pkg.audit._structure(side, left, right) == []
    # the honest opening holds link by link
    assert not audit_ref.check_links(N, q, h, left.r, e0, e1, left.in_idx, left.out_idx)[0].any()
    assert not audit_ref.check_links(N, q, h, right.r, e1, e2, right.in_idx, right.out_idx)[0].any()
    Links = pkg.audit.Links

    def both(l, r_):
        msgs = pkg.audit._structure(side, l, r_)
        assert bool(msgs) == (not audit_ref.structure_ok(side, l, r_))
        return msgs

    # a swapped pair of outputs: the structure is intact, the two links fail
    swapped = right.out_idx.copy()
    swapped[[0, 1]] = swapped[[1, 0]]
    assert both(left, Links(right.in_idx, swapped, right.r)) == []
    flags = audit_ref.check_links(N, q, h, right.r, e1, e2, right.in_idx, swapped)[0]
    assert flags[:2].tolist() == [audit_ref.MISMATCH] * 2 and not flags[2:].any()
    # a link opened on the wrong side: middle item j of the left list is one whose right link was asked for
    j_right = int(right.in_idx[0])
    wrong = left.out_idx.copy()
    wrong[0] = j_right
    assert any("left" in m for m in both(Links(left.in_idx, wrong, left.r), right))
    # a repeated index
    twice = right.out_idx.copy()
    twice[1] = twice[0]
    assert any("twice" in m for m in both(left, Links(right.in_idx, twice, right.r)))
    twice_in = left.in_idx.copy()
    twice_in[1] = twice_in[0]
    assert any("twice" in m for m in both(Links(twice_in, left.out_idx, left.r), right))
    # a link left out
    assert both(Links(left.in_idx[1:], left.out_idx[1:], left.r[1:]), right)


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
    for name, value in (("NTRU_LINK_BAD_INDEX", 1), ("NTRU_LINK_BAD_R", 2), ("NTRU_LINK_MISMATCH", 4)):
        assert re.search(r"#define %s %d\b" % (name, value), hdr), name
    assert (pkg.audit.LINK_BAD_INDEX, pkg.audit.LINK_BAD_R, pkg.audit.LINK_MISMATCH) == (1, 2, 4)
    assert pkg.audit.check_links is pkg.check_links and pkg.audit.check_links_dev is pkg.check_links_dev
    assert pkg.audit.open_links is pkg.open_links and pkg.audit.verify_rpc is pkg.verify_rpc
    assert hasattr(pkg.NTRU, "auditLinks")
    assert not [c for c in pkg.engine._CALLS if "links" in c.name]
    assert not [n for n in dir(pkg.Engine) if "links" in n]
    # abi.hip and ntru_host.hip are linked against fixed test doubles by tests/hostcheck: they must not need the new file
    for tu in ("abi.hip", "ntru_host.hip"):
        assert "check_links" not in open(os.path.join(SRC, tu)).read(), tu
    mk = open(os.path.join(SRC, "Makefile")).read()
    assert re.search(r"^AUDIT_SRCS := mix_audit\.hip$", mk, re.M)
    assert "mix_audit" not in re.search(r"^KERNEL_SRCS := (.*)$", mk, re.M).group(1)


def test_null_engine_and_bad_arguments_are_refused():
    """Everything that is refused before the engine is used: no GPU is needed for any of these."""
    lib = ge.build().load_library()
    N, q, L = 17, 32, 4
    ptr = lambda a: None if a is None else a.ctypes.data_as(C.c_void_p)
    h, r = np.ones(N, np.uint16), np.ones((L, N), np.uint8)
    e_in, e_out = np.zeros((L, N), np.uint16), np.zeros((L, N), np.uint16)
    idx, flags, n_bad = np.arange(L, dtype=np.int64), np.full(L, 0x5A, np.uint8), np.full(1, -7, np.int64)
    for fn in (lib.ntru_check_links_batch, lib.ntru_check_links_batch_dev):
        assert fn(None, N, q, 2, -1, -1, ptr(h), ptr(r), ptr(e_in), L, None, ptr(e_out), L, None, L, ptr(flags), ptr(n_bad)) == 2
        assert b"NULL" in lib.ntru_last_error()
    assert flags.tobytes() == np.full(L, 0x5A, np.uint8).tobytes() and n_bad[0] == -7


# ---- the build ----------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def asm_dir(tmp_path_factory):
    """The ISA and resource usage of mix_audit.hip alone, by the Makefile's own rule, into a fresh directory; returns it."""
    d = str(tmp_path_factory.mktemp("asm_audit"))
    out = subprocess.run(["make", "-C", SRC, os.path.join(d, "mix_audit.s"), "ASMDIR=" + d], capture_output=True, text=True, timeout=1800)
    assert out.returncode == 0, out.stderr[-2000:]
    return d


def test_new_kernels_do_not_spill(asm_dir):
    text = open(os.path.join(asm_dir, "mix_audit.usage")).read()
    assert "warning:" not in text.replace("argument unused during compilation: '--hip-link'", "").replace(
        "clang++: warning: ", ""), text[:2000]
    names = re.findall(r"Function Name: (\S+)", text)
    scratch = [int(x) for x in re.findall(r"ScratchSize \[bytes/lane\]: (\d+)", text)]
    assert len(names) == len(scratch) == 4, names
    assert not [(n, s) for n, s in zip(names, scratch) if s]
    for must in ("k_linkcheck_m5MGeom", "k_linkcheck_md5MGeom", "k_clean_r", "k_compare_links"):
        assert any(must in n for n in names), must
    # two workgroups of four waves per CU: two waves per SIMD
    occ = [int(x) for x in re.findall(r"Occupancy \[waves/SIMD\]: (\d+)", text)]
    assert all(o >= 2 for o in occ), occ


def test_no_wide_store_followed_by_a_write_of_its_data_registers(asm_dir):
    """The gfx950 hazard of test_build_quality.py (a 16-byte store whose data registers the very next instruction overwrites can store
    the new value), scanned over the ISA of mix_audit.hip as tests/test_mix_cpu.py scans matrix_reencrypt.hip."""
    lines = open(os.path.join(asm_dir, "mix_audit.s")).read().split("\n")
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
    assert any(re.match(r"^_Z\w*k_linkcheck_md\w*:", l) for l in lines)
    assert not bad, bad[:5]


def test_the_link_kernels_live_in_their_own_translation_unit():
    for fn in sorted(os.listdir(SRC)):
        if fn.endswith(".hip") and fn != "mix_audit.hip":
            assert "k_linkcheck" not in open(os.path.join(SRC, fn)).read(), fn
