"""Counting decrypted messages, the parts that need no GPU: the restatement (tests/count_ref.py) against the fixture of the unmodified
reference, the four new symbols in the library, the header and the binding, the argument checks that come before the engine, and the
build of count_bytes.hip (its kernel by name, no scratch; the border between its two accumulation routes)."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import __graft_entry__ as ge
import count_ref
import lift_ref

SRC = os.path.join(ge.PKG_DIR, "csrc")
SYMBOLS = ("ntru_count_bytes_batch", "ntru_count_bytes_batch_dev", "ntru_count_bytes_packed_batch", "ntru_count_bytes_packed_batch_dev")
PLAN = ["honest", "honest", "foreign", "honest", "below", "arbitrary", "honest", "honest", "wrong_tag", "honest", "above", "foreign",
        "honest", "arbitrary", "honest", "honest"]


@pytest.fixture(scope="module")
def cases():
    return count_ref.load_cases()


def test_fixture_has_the_sets(cases):
    assert [(c["options"]["N"], c["options"]["q"], c["liftRight"]) for c in cases] == [(17, 32, True), (167, 128, True), (167, 256, False)]
    assert os.path.getsize(count_ref.GOLDEN) < 64 * 1024
    assert (cases[0]["W"], cases[0]["fieldOffset"], cases[0]["fieldLength"], cases[0]["tagOffset"], len(cases[0]["tag"])) == (2, 0, 1, 1, 1)
    for c in cases[1:]:
        assert (c["W"], c["tagOffset"], c["tag"], c["fieldOffset"], c["fieldLength"], c["firstChoice"], c["nChoices"]) == \
               (20, 3, b"NTRU", 8, 2, 0x0100, 5)
    for c in cases:
        N, n = c["options"]["N"], c["nChoices"]
        assert c["f"].shape == c["fp"].shape == (2, N) and c["e"].shape == c["value"].shape == (16, N)
        assert [k["kind"] for k in c["kinds"]] == PLAN and c["G"] == 3 and set(c["group"].tolist()) <= {0, 1, 2}
        assert c["count"].shape == (3, n + 3) and c["count"].sum() == 16
        assert np.array_equal(c["count"].sum(axis=1), np.bincount(c["group"], minlength=3))
        honest = [b for b, k in enumerate(c["kinds"]) if k["kind"] == "honest"]
        assert len({c["kinds"][b]["choice"] for b in honest}) >= 3
        if c["liftRight"]:
            assert all(c["cls"][b] == c["kinds"][b]["choice"] for b in honest)
            assert c["cls"][PLAN.index("below")] == c["cls"][PLAN.index("above")] == n and c["cls"][PLAN.index("wrong_tag")] == n + 1
            assert (c["count"].sum(axis=0)[n:] > 0).all() and c["count"][:, :n].sum() == len(honest)
        else:
            assert all(c["cls"][b] >= n for b in honest)          # q = 1 (mod 3): index.js:117 does not return the plaintext


def test_restatement_reproduces_every_record(cases):
    for c in cases:
        o = c["options"]
        N, q, p = o["N"], o["q"], o["p"]
        value = lift_ref.decrypt(N, q, p, c["f"][0], c["fp"][0], c["e"], lift_ref.REFERENCE)[0]
        assert np.array_equal(value, c["value"]), c["set"]
        count, cls = count_ref.count_bytes(N, q, p, c["W"], c["f"][0], c["fp"][0], c["e"], groups=c["group"], G=3, **count_ref.layout(c))
        assert np.array_equal(cls, c["cls"]) and np.array_equal(count, c["count"]), c["set"]
        assert count.dtype == np.int64 and cls.dtype == np.int32
        # one group: the column sums
        one, cls1 = count_ref.count_bytes(N, q, p, c["W"], c["f"][0], c["fp"][0], c["e"], **count_ref.layout(c))
        assert np.array_equal(one, c["count"].sum(axis=0, keepdims=True)) and np.array_equal(cls1, c["cls"])


def test_centred_lift_puts_the_honest_ballots_of_the_third_set_in_their_bins(cases):
    c = cases[2]
    o = c["options"]
    count, cls = count_ref.count_bytes(o["N"], o["q"], o["p"], c["W"], c["f"][0], c["fp"][0], c["e"], mode=lift_ref.CENTRED, groups=c["group"],
                                       G=3, **count_ref.layout(c))
    honest = [b for b, k in enumerate(c["kinds"]) if k["kind"] == "honest"]
    assert len(honest) == 9 and all(cls[b] == c["kinds"][b]["choice"] for b in honest)
    n = c["nChoices"]
    assert cls[PLAN.index("below")] == cls[PLAN.index("above")] == n and cls[PLAN.index("wrong_tag")] == n + 1
    assert count.sum() == 16


def test_restatement_on_hand_made_bytes():
    data = np.zeros((8, 6), np.uint8)
    data[:, 1:3] = [0xAB, 0xCD]
    data[:, 2:6] = [[0xCD, 0, 0, 5], [0xCD, 0, 0, 6], [0xCD, 0, 0, 4], [0xCD, 0, 0, 7], [0xCD, 0, 1, 5], [0xCE, 0, 0, 5], [0xCD, 0, 0, 5],
                    [0xCD, 255, 255, 255]]
    flags = np.array([0, 0, 0, 0, 0, 0, 64, 0], np.uint8)
    kw = dict(first_choice=5, n_choices=2, field_off=3, field_len=3, tag=b"\xab\xcd", tag_off=1)
    assert count_ref.classify(data, flags, **kw).tolist() == [0, 1, 2, 2, 2, 3, 4, 2]
    count, cls = count_ref.count_data(data, flags, groups=[0, 1, 1, 0, 2, 5, -1, 1], G=3, **kw)
    assert cls.tolist() == [0, 1, 2, 2, 2, -1, -1, 2] and count.tolist() == [[1, 0, 1, 0, 0], [0, 1, 2, 0, 0], [0, 0, 1, 0, 0]]
    # a field that overlaps the tag, and the 64-bit comparison at the top of the range
    top = dict(first_choice=0xFFFFFFFF, n_choices=2, field_off=2, field_len=4)
    assert count_ref.classify(data, flags, **top).tolist() == [2, 2, 2, 2, 2, 2, 4, 2]
    data[7, 2:6] = 255
    assert count_ref.classify(data, flags, **top).tolist()[7] == 0


def test_symbols_are_exported_declared_and_bound():
    pkg = ge.build()
    lib = pkg.load_library()
    raw = C.CDLL(pkg.engine.library_path())
    hdr = open(os.path.join(ge.ROOT, "include", "ntru_engine.h")).read()
    for s in SYMBOLS:
        assert getattr(lib, s) is not None
        assert hasattr(raw, s), s
        assert re.search(r"\bint %s\(" % s, hdr), s
        assert s in pkg.engine._SIGS and len(pkg.engine._SIGS[s][1]) == 20
        assert pkg.engine._SIGS[s][1][14] is C.c_uint64          # first_choice
    assert "#define NTRU_COUNT_MAX_CHOICES 65536" in hdr and "#define NTRU_COUNT_MAX_BINS (1 << 24)" in hdr
    for name in ("NTRU_COUNT_OTHER", "NTRU_COUNT_BAD_TAG", "NTRU_COUNT_MALFORMED"):
        assert "#define %s(" % name in hdr
    assert "do not depend on the order of the adds" in hdr
    for name in ("count_bytes_batch", "count_bytes_batch_dev", "count_bytes_packed_batch", "count_bytes_packed_batch_dev"):
        assert getattr(pkg.count, name) is getattr(pkg, name)
    assert (pkg.count.MAX_CHOICES, pkg.count.MAX_BINS) == (count_ref.MAX_CHOICES, count_ref.MAX_BINS) == (65536, 1 << 24)
    assert (pkg.count.other(8), pkg.count.bad_tag(8), pkg.count.malformed(8)) == (8, 9, 10)
    assert not [c for c in pkg.engine._CALLS if "count" in c.name]
    assert not [n for n in dir(pkg.Engine) if "count" in n and n != "device_count"]
    assert callable(pkg.NTRU.countBytes) and callable(pkg.NTRU.countPacked)
    assert "countBytes" in pkg.NTRU.__doc__ and "countPacked" in pkg.NTRU.__doc__
    # abi.hip and ntru_host.hip are linked against fixed test doubles by tests/hostcheck: they must not need the new file
    for tu in ("abi.hip", "ntru_host.hip"):
        assert "ntru_count" not in open(os.path.join(SRC, tu)).read(), tu


def _call(lib, sym, eng=None, N=167, q=128, p=3, nbytes=20, B=4, tag_off=0, tag_len=4, field_off=8, field_len=2, first=0x100, n_choices=5,
          G=3, group=True, count=True, cls=True, rows=True, tag=True, ids=(0, 1, 2, 0), overlap=False):
    """One call with every array argument a real host array, so that only the argument under test is wrong."""
    f, fp = np.zeros(N, np.int8), np.zeros(N, np.uint8)
    e = np.zeros((max(B, 1), 4 * N), np.uint16)
    t = np.zeros(64, np.uint8)
    grp = np.array(list(ids) + [0] * max(B - len(ids), 0), np.int32)
    cnt = np.zeros(4096, np.int64)
    cl = np.zeros(max(B, 1), np.int32)
    ptr = lambda a: a.ctypes.data_as(C.c_void_p)
    p_cls = C.c_void_p(cnt.ctypes.data + 8) if overlap else ptr(cl)
    return getattr(lib, sym)(eng, N, q, p, nbytes, ptr(f), ptr(fp), ptr(e) if rows else None, B, tag_off, tag_len, ptr(t) if tag else None,
                             field_off, field_len, first, n_choices, G, ptr(grp) if group else None, ptr(cnt) if count else None,
                             p_cls if cls else None)


@pytest.mark.parametrize("sym", SYMBOLS)
def test_argument_errors_come_before_the_engine(sym):
    """Every one of these is NTRU_ERR_ARG with its own message although the engine is NULL: nothing needs a GPU."""
    lib = ge.build().load_library()
    err = lambda: lib.ntru_last_error().decode()
    host = not sym.endswith("_dev")
    assert _call(lib, sym) == 2 and "engine is NULL" in err()
    assert _call(lib, sym, cls=False) == 2 and "engine is NULL" in err()                       # cls is optional
    assert _call(lib, sym, G=1, group=False) == 2 and "engine is NULL" in err()               # group is optional with one group
    assert _call(lib, sym, B=0, rows=False) == 2 and "engine is NULL" in err()
    # NULL buffers
    assert _call(lib, sym, rows=False) == 2 and "NULL buffer" in err()
    assert _call(lib, sym, count=False) == 2 and "count is NULL" in err()
    assert _call(lib, sym, tag=False) == 2 and "tag is NULL" in err()
    assert _call(lib, sym, tag=False, tag_len=0) == 2 and "engine is NULL" in err()
    # the tag and the field inside the message
    assert _call(lib, sym, tag_len=33) == 2 and "tag_len" in err()
    assert _call(lib, sym, tag_len=-1) == 2 and "tag_len" in err()
    assert _call(lib, sym, tag_off=17, tag_len=4) == 2 and "the tag [17, 21) does not lie inside" in err()
    assert _call(lib, sym, tag_off=-1, tag_len=0) == 2 and "the tag" in err()
    assert _call(lib, sym, tag_off=16, tag_len=4) == 2 and "engine is NULL" in err()          # ends at nbytes: fine
    assert _call(lib, sym, field_len=0) == 2 and "field_len" in err()
    assert _call(lib, sym, field_len=5) == 2 and "field_len" in err()
    assert _call(lib, sym, field_off=19, field_len=2) == 2 and "the choice field [19, 21) does not lie inside" in err()
    assert _call(lib, sym, field_off=-1) == 2 and "the choice field" in err()
    assert _call(lib, sym, field_off=16, field_len=4) == 2 and "engine is NULL" in err()      # ends at nbytes: fine
    assert _call(lib, sym, field_off=1, field_len=4) == 2 and "engine is NULL" in err()       # overlaps the tag: fine
    # first_choice, n_choices, G and the product
    assert _call(lib, sym, first=1 << 32) == 2 and "first_choice = 4294967296 does not fit 32 bits" in err()
    assert _call(lib, sym, first=(1 << 32) - 1) == 2 and "engine is NULL" in err()
    assert _call(lib, sym, n_choices=0) == 2 and "n_choices" in err()
    assert _call(lib, sym, n_choices=65537, G=1) == 2 and "n_choices" in err()
    assert _call(lib, sym, n_choices=65536, G=1, group=False, cls=False) == 2 and "engine is NULL" in err()
    assert _call(lib, sym, G=0) == 2 and "G >= 1" in err()
    assert _call(lib, sym, G=-3) == 2 and "G >= 1" in err()
    assert _call(lib, sym, n_choices=5, G=(1 << 21) + 1) == 2 and "bins exceed" in err()
    assert _call(lib, sym, n_choices=65536, G=256) == 2 and "bins exceed" in err()
    assert _call(lib, sym, n_choices=1, G=1 << 30) == 2 and "bins exceed" in err()            # the product is taken in 64 bits
    assert _call(lib, sym, G=3, group=False) == 2 and "group is NULL with G = 3" in err()
    # overlapping outputs
    assert _call(lib, sym, overlap=True) == 2 and "count and cls overlap" in err()
    # the domain of the byte calls
    assert _call(lib, sym, nbytes=21) == 2 and "nbytes" in err()
    assert _call(lib, sym, B=-1) == 2 and "negative batch" in err()
    assert _call(lib, sym, N=7, nbytes=1) == 2 and "N = 7" in err()
    # group ids outside [0, G): the host forms name the index before anything is launched, the _dev forms cannot read them
    for ids, at in (((0, 1, 3, 0), 2), ((-1, 1, 2, 0), 0), ((0, 1, 2, 1 << 30), 3)):
        assert _call(lib, sym, ids=ids) == 2
        assert ("group[%d] = %d is outside [0, G)" % (at, ids[at]) in err()) if host else ("engine is NULL" in err())


# ---- the build ----------------------------------------------------------------------------------------------------------------------
def test_the_kernel_is_there_and_does_not_spill(tmp_path):
    """`make <ASMDIR>/count_bytes.s` into a fresh directory: k_count_classify by name, ScratchSize 0 for every kernel of the file."""
    d = str(tmp_path)
    out = subprocess.run(["make", "-C", SRC, d + "/count_bytes.s", "ASMDIR=" + d], capture_output=True, text=True, timeout=1800)
    assert out.returncode == 0, out.stderr[-2000:]
    text = open(os.path.join(d, "count_bytes.usage")).read()
    names = re.findall(r"Function Name: (\S+)", text)
    scratch = [int(x) for x in re.findall(r"ScratchSize \[bytes/lane\]: (\d+)", text)]
    assert names and len(names) == len(scratch), names
    assert not [(n, s) for n, s in zip(names, scratch) if s]
    assert all("k_count_classify" in n for n in names), names
    # the LDS route holds its whole histogram, the other route none
    lds = sorted(int(x) for x in re.findall(r"LDS Size \[bytes/block\]: (\d+)", text))
    assert lds == [0, 4 * count_ref.CT_LDS_BINS], lds


def test_the_border_between_the_routes_is_the_sources():
    src = open(os.path.join(SRC, "count_bytes.hip")).read()
    m = re.search(r"constexpr int CT_LDS_BINS = (\d+);", src)
    assert m and int(m.group(1)) == count_ref.CT_LDS_BINS == 8192
    mk = open(os.path.join(SRC, "Makefile")).read()
    assert "COUNT_SRCS := count_bytes.hip" in mk and "$(COUNT_SRCS)" in mk.split("SRCS := abi.hip")[1].splitlines()[0]
    assert "$(COUNT_SRCS:%.hip=$(ASMDIR)/%.s)" in mk
    assert "count_bytes.hip" not in [l for l in mk.splitlines() if l.startswith("KERNEL_SRCS")][0]
