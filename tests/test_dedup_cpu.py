"""Removing duplicates, the parts that need no GPU: the five exported symbols, every refusal of the four entry points through ctypes with
a NULL engine, the workspace size, the numpy reference against a plain dictionary, header / binding / export agreement, the build of
dedup_rows.hip, the fixture, and the Node shim, which is composed in JavaScript and runs without the addon."""
import ctypes as C
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

import __graft_entry__ as ge
import dedup_ref as ref
import packed_ref

SRC = os.path.join(ge.PKG_DIR, "csrc")
ERR_ARG = 2
FORMS = ["ntru_dedup_rows", "ntru_dedup_rows_dev", "ntru_dedup_packed", "ntru_dedup_packed_dev"]
SYMBOLS = FORMS + ["ntru_dedup_workspace_bytes"]
MAX_ROWS = 1 << 24


@pytest.fixture(scope="module")
def pkg():
    return ge.build()


@pytest.fixture(scope="module")
def lib(pkg):
    return pkg.load_library()


def test_the_library_exports_the_five_symbols(lib):
    out = subprocess.run(["nm", "-D", "--defined-only", os.path.join(ge.PKG_DIR, "lib", "libntru_engine.so")], capture_output=True, text=True)
    exported = set(re.findall(r" T (ntru_dedup\w+)", out.stdout)) if out.returncode == 0 else {s for s in SYMBOLS if hasattr(lib, s)}
    assert exported == set(SYMBOLS)


# ---- the entry points' checks, with a NULL engine --------------------------------------------------------------------------------------
def _call(lib, form, N, mod, prior, S, rows, B, bits, work, first, unique, count, salt=1):
    ptr = lambda a: a if a is None or isinstance(a, C.c_void_p) else a.ctypes.data_as(C.c_void_p)
    args = [None, N, mod, ptr(prior), S, ptr(rows), B, salt, bits] + ([ptr(work)] if form.endswith("_dev") else []) + [ptr(first), ptr(unique), ptr(count)]
    rc = getattr(lib, form)(*args)
    return rc, lib.ntru_last_error().decode()


def _valid(B=5, S=3):
    """Arguments that pass every check; the rows are large enough for the packed forms too (32 bytes per field element)."""
    return dict(N=17, mod=4096, prior=np.zeros(S * 3 * 4, np.uint64), S=S, rows=np.zeros(B * 3 * 4, np.uint64), B=B, bits=64,
                work=np.zeros(1 << 16, np.uint64), first=np.zeros(B, np.int64), unique=np.zeros(B, np.int64), count=np.zeros(1, np.int64))


@pytest.mark.parametrize("form", FORMS)
def test_argument_errors_come_before_the_engine(lib, form):
    who = form.replace("_dev", "") + ": "
    rows_name = "packed" if "packed" in form else "rows"
    bad = [(dict(B=-1), "negative batch size"), (dict(S=-1), "negative number of prior rows"),
           (dict(S=MAX_ROWS, B=1), "S + B <= NTRU_DEDUP_MAX_ROWS"), (dict(B=MAX_ROWS + 1, S=0), "S + B <= NTRU_DEDUP_MAX_ROWS"),
           (dict(bits=-1), "0 <= fingerprint_bits <= 64"), (dict(bits=65), "0 <= fingerprint_bits <= 64"),
           (dict(N=1), "need 2 <= N <= 1920"), (dict(N=1921), "need 2 <= N <= 1920"),
           (dict(mod=1), "need 2 <= mod <= 65536"), (dict(mod=65537), "need 2 <= mod <= 65536"),
           (dict(count=None), "count is NULL"), (dict(rows=None), "NULL buffer (%s)" % rows_name),
           (dict(prior=None), "prior is NULL with S > 0")]
    if form.endswith("_dev"):
        bad.append((dict(work=None), "NULL buffer (work)"))
    seen = set()
    for change, word in bad:
        args = _valid()
        args.update(change)
        rc, msg = _call(lib, form, **args)
        assert rc == ERR_ARG and msg.startswith(who) and word in msg and "engine" not in msg, (change, rc, msg)
        seen.add(word)
    assert len(seen) == (10 if form.endswith("_dev") else 9)
    # ... and the engine comes last: valid arguments, either output NULL, no prior set, the corners of the domain, B == 0 without rows
    for change in (dict(), dict(first=None), dict(unique=None), dict(first=None, unique=None), dict(S=0, prior=None), dict(N=2, mod=2),
                   dict(N=1920, mod=65536, rows=np.zeros(5 * 1920, np.uint64), prior=np.zeros(3 * 1920, np.uint64)), dict(mod=3), dict(bits=0),
                   dict(B=0, rows=None, work=None, first=None, unique=None), dict(S=1000, prior=C.c_void_p(1 << 40))):      # (a prior set is never read here)
        args = _valid()
        args.update(change)
        rc, msg = _call(lib, form, **args)
        assert rc == ERR_ARG and msg == "engine is NULL", (change, msg)


@pytest.mark.parametrize("form", FORMS)
def test_overlapping_outputs_are_refused(lib, form):
    N, B, S = 17, 5, 3
    rows_name = "packed" if "packed" in form else "rows"
    row_bytes = 96 if "packed" in form else 2 * N
    assert packed_ref.params(4095, N)[3] * 32 == 96
    buf = np.zeros(1 << 14, np.uint64)
    raw = buf.view(np.uint8)
    at = lambda byte: C.c_void_p(raw.ctypes.data + byte)
    base = dict(prior=at(0), rows=at(1024), first=at(4096), unique=at(8192), count=at(12288), work=at(16384))
    cases = [(dict(unique=at(4096 + 8 * B - 8)), "first overlaps unique"), (dict(count=at(4096)), "first overlaps count"),
             (dict(count=at(8192 + 8 * B - 8)), "unique overlaps count"), (dict(first=at(1024 + B * row_bytes - 8)), "first overlaps " + rows_name),
             (dict(unique=at(1024 - 8 * B + 8)), "unique overlaps " + rows_name), (dict(count=at(S * row_bytes - 8)), "count overlaps prior"),
             (dict(first=at(0)), "first overlaps prior")]
    if form.endswith("_dev"):
        cases += [(dict(first=at(16384)), "first overlaps work"), (dict(unique=at(16384 - 8)), "unique overlaps work"),
                  (dict(count=at(16384 + 1024)), "count overlaps work")]
    who = form.replace("_dev", "") + ": "
    for change, word in cases:
        args = dict(base)
        args.update(change)
        rc, msg = _call(lib, form, N, 4096, args["prior"], S, args["rows"], B, 64, args["work"], args["first"], args["unique"], args["count"])
        assert rc == ERR_ARG and msg == who + word, (word, msg)
    # touching ranges do not overlap
    rc, msg = _call(lib, form, N, 4096, base["prior"], S, base["rows"], B, 64, base["work"], at(1024 + B * row_bytes), at(4096 + 8 * B), at(4096 - 8))
    assert rc == ERR_ARG and msg == "engine is NULL", msg


def test_workspace_bytes_is_monotone_and_granular(pkg, lib):
    n = C.c_size_t()
    sizes = []
    for rows in (0, 1, 2, 255, 256, 257, 1024, 1025, 65536, 70001, 2 ** 18 + 3, 2 ** 20, MAX_ROWS):
        assert lib.ntru_dedup_workspace_bytes(167, rows, C.byref(n)) == 0
        assert n.value % 256 == 0 and n.value >= 34 * rows
        sizes.append(n.value)
    assert sizes == sorted(sizes) and sizes[0] > 0
    assert sizes[-3] < 48 * 2 ** 20                                           # about 34 bytes per row, beside the sort's 24
    assert lib.ntru_dedup_workspace_bytes(2, 2 ** 20, C.byref(n)) == 0 and n.value == sizes[-2]       # the size does not depend on N
    for bad, word in ((dict(N=1), "need 2 <= N"), (dict(N=1921), "need 2 <= N"), (dict(rows=-1), "total_rows"), (dict(rows=MAX_ROWS + 1), "total_rows")):
        a = dict(N=167, rows=5)
        a.update(bad)
        assert lib.ntru_dedup_workspace_bytes(a["N"], a["rows"], C.byref(n)) == ERR_ARG
        msg = lib.ntru_last_error().decode()
        assert msg.startswith("ntru_dedup_workspace_bytes: ") and word in msg
    assert lib.ntru_dedup_workspace_bytes(167, 5, None) == ERR_ARG


# ---- the reference ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("N,mod,S,B", [(2, 2, 0, 9), (7, 3, 4, 40), (17, 128, 0, 64), (33, 65536, 11, 50), (9, 7, 1, 1), (8, 4096, 30, 2)])
def test_reference_agrees_with_a_dictionary(N, mod, S, B):
    rng = np.random.default_rng(N + B)
    both = ref.family_rows(rng, N, mod, S + B)
    prior, rows = (both[:S] if S else None), both[S:]
    first, unique = ref.want(mod, rows, prior)
    wf, wu = ref.by_dictionary(mod, rows.tolist(), prior.tolist() if S else None)
    assert first.tolist() == wf and unique.tolist() == wu
    assert first.dtype == unique.dtype == np.int64
    bits = packed_ref.params(mod - 1, N)[0]
    raw = both & ((1 << bits) - 1)
    pk = packed_ref.set_ignored_bits(mod, N, packed_ref.pack_rows(mod, raw))
    pf, pu = ref.want_packed(mod, N, pk[S:], pk[:S] if S else None)
    wf, wu = ref.by_dictionary(mod, raw[S:].tolist(), raw[:S].tolist() if S else None)
    assert pf.tolist() == wf and pu.tolist() == wu


def test_the_families_hold_what_they_promise():
    rng = np.random.default_rng(1)
    N, mod, B = 17, 128, 45
    rows = ref.family_rows(rng, N, mod, B).astype(np.int64)
    first, unique = ref.want(mod, rows)
    base = rows[0]
    assert (rows >= mod).any() and first[3] == 0 and (rows[3] != base).any()              # mod added: equal
    assert first[4] == 4 and (rows[4, 1:] == base[1:]).all() and first[5] == 5 and (rows[5, :-1] == base[:-1]).all()
    assert first[6] == 6 and sorted(rows[6]) == sorted(base) and first[7] == 7 and sorted(rows[7]) == sorted(base)
    assert first[12] == 11 and first[8] == 8 and first[19] == 8 and not rows[8].any()     # an adjacent copy; the zero row
    assert 3 < len(unique) < B


def test_fixture_is_consistent_with_the_reference():
    cases = ref.load_cases()
    assert os.path.getsize(ref.GOLDEN) < 64 * 1024 and len(cases) == 4
    for c in cases:
        prior = np.array(c["prior"], np.int64).reshape(-1, c["N"])
        first, unique = ref.want(c["q"], np.array(c["rows"]), prior if len(prior) else None)
        assert first.tolist() == c["first"] and unique.tolist() == c["unique"], c["name"]
        assert 0 < len(c["unique"]) < len(c["rows"])
    assert any(c["prior"] for c in cases) and any(not c["prior"] for c in cases)
    assert any(min(c["first"]) < len(c["prior"]) for c in cases if c["prior"])            # a new row repeats a prior row
    assert any(np.array(c["rows"]).max() >= c["q"] for c in cases)                        # a copy with q added


# ---- header, binding, exports ----------------------------------------------------------------------------------------------------------
def test_symbols_are_declared_and_bound(pkg, lib):
    hdr = open(os.path.join(ge.ROOT, "include", "ntru_engine.h")).read()
    for s in SYMBOLS:
        assert hasattr(lib, s) and re.search(r"\bint %s\(" % s, hdr), s
        assert s in pkg.engine._SIGS
    assert [len(pkg.engine._SIGS[s][1]) for s in SYMBOLS] == [12, 13, 12, 13, 3]
    assert "#define NTRU_DEDUP_MAX_ROWS NTRU_PERM_MAX_B" in hdr and pkg.dedup.DEDUP_MAX_ROWS == pkg.mix.PERM_MAX_B == MAX_ROWS
    assert hdr.index("drawing the mix order") < hdr.index("removing duplicates")
    for name in ("dedup_rows", "dedup_rows_dev", "dedup_packed", "dedup_packed_dev", "dedup_workspace_bytes"):
        assert getattr(pkg.dedup, name) is getattr(pkg, name)
    assert callable(pkg.NTRU.dedupBatch)
    assert not [c for c in pkg.engine._CALLS if "dedup" in c.name] and not [n for n in dir(pkg.Engine) if "dedup" in n]
    # abi.hip and ntru_host.hip are linked against fixed test doubles by tests/hostcheck: they must not need the new file; and the sort
    # is reached through its entry point
    for tu in ("abi.hip", "ntru_host.hip", "permutation.hip"):
        assert "dedup" not in open(os.path.join(SRC, tu)).read(), tu
    shim = open(os.path.join(ge.PKG_DIR, "js", "index.mjs")).read()
    assert re.search(r"^  dedupCiphertexts\(e, B, \{ prior = null \} = \{\}\) \{", shim, flags=re.M)
    doc = open(os.path.join(ge.ROOT, "INTEGRATION.md")).read()
    assert "## Removing duplicates" in doc and "re-randomised" in doc


# ---- the build -------------------------------------------------------------------------------------------------------------------------
def test_new_kernels_do_not_spill(tmp_path):
    out = subprocess.run(["make", "-C", SRC, "ASMDIR=%s" % tmp_path, "%s/dedup_rows.s" % tmp_path], capture_output=True, text=True,
                         timeout=900)
    assert out.returncode == 0, out.stderr[-2000:]
    text = open(os.path.join(str(tmp_path), "dedup_rows.usage")).read()
    names = re.findall(r"Function Name: (\S+)", text)
    scratch = [int(x) for x in re.findall(r"ScratchSize \[bytes/lane\]: (\d+)", text)]
    assert len(names) == len(scratch) == 10 and not [(n, s) for n, s in zip(names, scratch) if s]
    assert sorted({re.search(r"k_dedup_[a-z]+", n).group(0) for n in names}) == [
        "k_dedup_assign", "k_dedup_emit", "k_dedup_fingerprint", "k_dedup_mark", "k_dedup_neighbours", "k_dedup_offsets", "k_dedup_walk"]
    isa = open(os.path.join(str(tmp_path), "dedup_rows.s")).read()
    meta = isa[isa.index("amdhsa.kernels"):]
    assert len(re.findall(r"\.private_segment_fixed_size: 0\b", meta)) == 10 and len(re.findall(r"\.private_segment_fixed_size:", meta)) == 10
    assert "global_load_dwordx4" in isa and "global_atomic" not in isa
    mk = open(os.path.join(SRC, "Makefile")).read()
    assert re.search(r"^DEDUP_SRCS := dedup_rows.hip$", mk, flags=re.M)
    assert "dedup_rows.hip" not in re.search(r"^KERNEL_SRCS := (.*)$", mk, flags=re.M).group(1)
    assert "$(DEDUP_SRCS)" in re.search(r"^SRCS := (.*)$", mk, flags=re.M).group(1)
    assert "$(DEDUP_SRCS:%.hip=$(ASMDIR)/%.s)" in mk


# ---- Node ---------------------------------------------------------------------------------------------------------------------------------
NODE = shutil.which("node")


@pytest.mark.skipif(NODE is None, reason="node is not installed")
def test_shim_dedup():
    r = subprocess.run([NODE, os.path.join(ge.ROOT, "tests", "js", "shim_dedup.mjs")], cwd=ge.ROOT, capture_output=True, text=True,
                       timeout=600)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    assert "shim_dedup: 4 cases, 79 rows" in r.stdout
