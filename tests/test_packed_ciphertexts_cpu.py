"""Packed ciphertexts without a GPU: the restatement (tests/packed_ref.py) against the captured packOutput / unpackInput vectors and against
itself (Python ints and numpy limbs, the ignore rules), ntru_pack_params at the shapes the GPU tests use, and the new C ABI through
its layers: header, exported symbols, _SIGS, the packed module against a recording stub, the package's re-exports."""
import ctypes as C
import inspect
import os
import re

import numpy as np
import pytest

import __graft_entry__ as ge
import ciphertext_sum_ref as sum_ref
import packed_ref as ref
from conftest import load_golden

pkg = ge.load_package()
engine = pkg.engine

SHAPES = ref.SHAPES
NAMES = ["ntru_sum_groups_packed", "ntru_tally_decrypt_packed_batch", "ntru_decrypt_packed_batch"]


@pytest.fixture(scope="module")
def lib():
    ge.build()
    return pkg.load_library()


@pytest.mark.parametrize("N,mod,bits,per,os_", SHAPES)
def test_pack_params_at_the_shapes(lib, N, mod, bits, per, os_):
    v = [C.c_int(0) for _ in range(4)]
    assert lib.ntru_pack_params(mod - 1, N, *[C.byref(x) for x in v]) == 0
    assert (v[0].value, v[1].value, v[3].value) == (bits, per, os_)
    assert ref.params(mod - 1, N) == tuple(x.value for x in v)
    assert v[2].value >= N and v[3].value * per >= N                                  # every coefficient has a field


def test_restatement_equals_the_captured_packOutput_vectors():
    gold = load_golden("pack_functions.json")
    assert len(gold["packOutput"]) >= 10
    for c in gold["packOutput"]:
        want = [int(x, 16) for x in c["expected"]]                                    # the fixture spells BigInts in hex
        bits, per, arr_len, os_ = ref.params(c["maxVal"], c["dataLen"])
        assert (bits, per * bits, os_, arr_len) == (c["maxInputBits"], c["maxOutputBits"], c["outputSize"], c["arrLen"])
        assert ref.pack_ints(c["maxVal"], c["dataLen"], c["data"]) == want
        data = list(c["data"]) + [0] * (c["dataLen"] - len(c["data"]))
        assert ref.unpack_ints(c["maxVal"], c["dataLen"], want) == data
        if c["dataLen"] >= 2 and all(0 <= x <= c["maxVal"] for x in data):
            # the numpy form on the same vector (mod - 1 = maxVal)
            packed = ref.pack_rows(c["maxVal"] + 1, np.array([data]))
            assert ref.ints_of(packed[0]) == want
            assert ref.unpack_rows(c["maxVal"] + 1, c["dataLen"], packed)[0].tolist() == data
    for c in gold["unpackInput"]:
        bits = c["maxInputBits"]
        per = c["packedBits"] // bits
        got = [(int(v, 16) >> (j * bits)) & ((1 << bits) - 1) for v in c["data"] for j in range(per)]
        assert pkg.trimPolynomial(got) == c["unpacked"]


@pytest.mark.parametrize("N,mod,bits,per,os_", SHAPES)
def test_numpy_form_equals_the_int_form_and_ignores_what_it_must(N, mod, bits, per, os_):
    g = np.random.default_rng(N + mod)
    rows = g.integers(0, 1 << bits, (5, N), dtype=np.uint16)                          # raw fields: values >= mod included
    packed = ref.pack_rows(mod, rows)
    assert packed.shape == (5, os_, 4) and packed.dtype == np.uint64
    for b in range(5):
        assert ref.ints_of(packed[b]) == ref.pack_ints(mod - 1, N, rows[b].tolist())
    noisy = ref.set_ignored_bits(mod, N, packed)
    for b in range(5):
        ints = ref.ints_of(noisy[b])
        assert all(v >> (per * bits) == (1 << (256 - per * bits)) - 1 for v in ints)                 # the top of every element is set
        assert all((v >> (j * bits)) & ((1 << bits) - 1) == (1 << bits) - 1
                   for i, v in enumerate(ints) for j in range(per) if i * per + j >= N)              # and every pad field
        assert ref.unpack_ints(mod - 1, N, ints) == rows[b].tolist()
    assert np.array_equal(ref.unpack_rows(mod, N, noisy), rows) and np.array_equal(ref.unpack_rows(mod, N, packed), rows)
    w = g.integers(0, mod, 5, dtype=np.uint16)
    want = [[sum(int(w[r]) * int(rows[r, k]) for r in rs) % mod for k in range(N)] for rs in ([0, 1], [], [2, 3, 4])]
    assert ref.np_sum_packed(mod, N, noisy, offsets=[0, 2, 2, 5], weights=w).tolist() == want


def header_text():
    text = open(os.path.join(ge.ROOT, "include", "ntru_engine.h")).read()
    return re.sub(r"/\*.*?\*/", "", text, flags=re.S)


def test_header_sigs_and_exports(lib):
    text = header_text()
    for name in NAMES:
        host = re.search(r"\bint %s\s*\((.*?)\)\s*;" % name, text, flags=re.S).group(1)
        dev = re.search(r"\bint %s_dev\s*\((.*?)\)\s*;" % name, text, flags=re.S).group(1)
        strip = lambda a: re.sub(r"\bd_", "", " ".join(a.split()))
        assert strip(host) == strip(dev), name                                        # the two forms differ in where the pointers point
        assert "const uint64_t *packed" in strip(host)
        for sym in (name, name + "_dev"):
            assert hasattr(lib, sym), sym
            res, args = engine._SIGS[sym]
            assert res is C.c_int and len(args) == len(host.split(","))
            assert getattr(lib, sym).argtypes == args
    # the packed sum and tally take what their dense forms take
    for packed, dense in (("ntru_sum_groups_packed", "ntru_sum_groups"), ("ntru_tally_decrypt_packed_batch", "ntru_tally_decrypt_batch")):
        for suffix in ("", "_dev"):
            assert engine._SIGS[packed + suffix] == engine._SIGS[dense + suffix]
    assert engine._SIGS["ntru_decrypt_packed_batch"] == engine._SIGS["ntru_decrypt_batch"]


def test_argument_checks_need_no_device(lib):
    """The domain checks of ntru_sum_groups come first in the packed entries as well (NTRU_ERR_ARG = 2), ahead of the engine."""
    z = None
    for fn in (lib.ntru_sum_groups_packed, lib.ntru_sum_groups_packed_dev, lib.ntru_sum_groups, lib.ntru_sum_groups_dev):
        assert fn(z, 1, 32, z, z, z, 1, 1, z) == 2 and b"N" in lib.ntru_last_error()
        assert fn(z, 17, 1, z, z, z, 1, 1, z) == 2 and b"mod" in lib.ntru_last_error()
        assert fn(z, 17, 65537, z, z, z, 1, 1, z) == 2
        assert fn(z, 17, 32, z, z, z, 1, -1, z) == 2
        assert fn(z, 17, 32, z, z, z, 0, 1, z) == 2 and b"K >= 1" in lib.ntru_last_error()
        assert fn(z, 17, 32, z, z, z, 1, 1, z) == 2 and b"NULL" in lib.ntru_last_error()
    assert lib.ntru_sum_groups_packed(z, 17, 0, z, z, z, 1, 1, z) == 2 and lib.ntru_last_error().startswith(b"ntru_sum_groups_packed")


class Stub:
    """Records (name, arguments) of every library call; pack_params answers for N = 5, mod = 8 (3 bits, 84 per element, 3 elements)."""

    def __init__(self):
        self.calls = []

    def __getattr__(self, name):
        def fn(*args):
            self.calls.append((name, args))
            if name == "ntru_engine_create":
                args[-1]._obj.value = 0x5150
            if name == "ntru_pack_params":
                for r, v in zip(args[2:], (3, 84, 252, 3)):
                    r._obj.value = v
            return 0
        return fn


def test_packed_module_hands_the_library_what_the_header_asks_for(monkeypatch):
    stub = Stub()
    monkeypatch.setattr(engine, "_LIB", stub)
    eng = pkg.Engine(0)
    N, mod, B = 5, 8, 4
    packed = np.arange(B * 3 * 4, dtype=np.uint64).reshape(B, 3, 4)
    f, fp = np.ones(N, np.int8), np.ones(N, np.uint8)
    val = lambda a: a.value if isinstance(a, C.c_void_p) else a

    def last(symbol):
        name, args = stub.calls[-1]
        assert name == symbol
        return [val(a) for a in args]

    out = pkg.sum_groups_packed(eng, N, mod, packed, K=2, weights=[1, 2, 3, 4])
    a = last("ntru_sum_groups_packed")
    assert out.shape == (2, N) and out.dtype == np.uint16
    assert a[:4] == [0x5150, N, mod, packed.ctypes.data] and a[5] is None and a[6:8] == [2, 2] and a[8] == out.ctypes.data
    out = pkg.sum_groups_packed(eng, N, mod, packed, offsets=[0, 1, 4])
    a = last("ntru_sum_groups_packed")
    assert out.shape == (2, N) and a[4] is None and a[5] is not None and a[6:8] == [0, 2]
    with pytest.raises(ValueError):
        pkg.sum_groups_packed(eng, N, mod, packed, K=3)
    pkg.sum_groups_packed_dev(eng, N, mod, 0x1000, 0x2000, 2, K=2, d_weights=0x3000)
    assert last("ntru_sum_groups_packed_dev") == [0x5150, N, mod, 0x1000, 0x3000, None, 2, 2, 0x2000]
    pkg.sum_groups_packed_dev(eng, N, mod, 0x1000, 0x2000, 2, d_offsets=0x4000)
    assert last("ntru_sum_groups_packed_dev") == [0x5150, N, mod, 0x1000, None, 0x4000, 0, 2, 0x2000]

    total, value, q1, r1, q2 = pkg.tally_decrypt_packed_batch(eng, N, mod, 3, f, fp, packed, K=4)
    a = last("ntru_tally_decrypt_packed_batch")
    assert a[:4] == [0x5150, N, mod, 3] and a[6] == packed.ctypes.data and a[9:11] == [4, 1]
    assert a[11:] == [x.ctypes.data for x in (total, value, q1, r1, q2)]
    assert [x.shape for x in (total, value, q1, r1, q2)] == [(1, N)] * 5 and (total.dtype, value.dtype) == (np.uint16, np.uint8)
    assert pkg.tally_decrypt_packed_batch(eng, N, mod, 3, f, fp, packed, K=4, want_witness=False)[2:] == (None, None, None)
    assert last("ntru_tally_decrypt_packed_batch")[13:] == [None, None, None]
    pkg.tally_decrypt_packed_batch_dev(eng, N, mod, 3, 0x100, 0x200, 0x300, 0x400, 0x500, 1, K=4, d_quot2=0x600)
    assert last("ntru_tally_decrypt_packed_batch_dev") == [0x5150, N, mod, 3, 0x100, 0x200, 0x300, None, None, 4, 1, 0x400, 0x500, None, None,
                                                           0x600]

    value, q1, r1, q2 = pkg.decrypt_packed_batch(eng, N, mod, 3, f, fp, packed)
    a = last("ntru_decrypt_packed_batch")
    assert a[:4] == [0x5150, N, mod, 3] and a[6:8] == [packed.ctypes.data, B] and a[8:] == [x.ctypes.data for x in (value, q1, r1, q2)]
    assert value.shape == (B, N) and q2.dtype == np.uint8 and r1.dtype == np.uint16
    assert pkg.decrypt_packed_batch(eng, N, mod, 3, f, fp, packed, want_witness=False)[1:] == (None, None, None)
    pkg.decrypt_packed_batch_dev(eng, N, mod, 3, 0x100, 0x200, 0x300, B, 0x400)
    assert last("ntru_decrypt_packed_batch_dev") == [0x5150, N, mod, 3, 0x100, 0x200, 0x300, B, 0x400, None, None, None]


def test_the_surface():
    for name in ("sum_groups_packed", "tally_decrypt_packed_batch", "decrypt_packed_batch"):
        for suffix in ("", "_dev"):
            fn = getattr(pkg.packed, name + suffix)
            assert getattr(pkg, name + suffix) is fn and list(inspect.signature(fn).parameters)[0] == "eng"
    assert pkg.pack_rows is pkg.packed.pack_rows and pkg.unpack_rows is pkg.packed.unpack_rows
    assert str(inspect.signature(pkg.NTRU.tallyPacked)) == "(self, packed, offsets=None, weights=None, wantWitness=True)"
    assert str(inspect.signature(pkg.NTRU.decryptPackedBatch)) == "(self, packed, wantWitness=True)"
    js = open(os.path.join(ge.PKG_DIR, "js", "index.mjs")).read()
    assert "export function sumPackedCiphertexts(" in js and "tallyPackedBatch(" in js


def test_sum_ref_is_the_checker_of_the_dense_sums():
    """np_sum_packed is np_sum on the unpacked rows: the checker of tests/test_ciphertext_sum_gpu.py, unchanged."""
    rows = np.random.default_rng(1).integers(0, 4096, (40, 821), dtype=np.uint16)
    assert np.array_equal(ref.np_sum_packed(4096, 821, ref.pack_rows(4096, rows), K=8), sum_ref.np_sum(rows, 4096, K=8))


def test_variant_rows_reach_every_lane_layout_of_every_width(lib):
    """The 62 sum rows of tests/kernel_variants.py: each has one shape per lane layout its width reaches at N <= 1920, and every shape
    gives the layout it claims.  U and side are restated here from 252 // bits, the format from the library's own ntru_pack_params; the
    large launch of each shape has blocks of more than SP_BATCH side + side rows whatever the CU count."""
    import kernel_variants as kv
    src = open(os.path.join(ge.PKG_DIR, "csrc", "packed_ciphertexts.hip")).read()
    assert re.search(r"SP_BATCH = (\d+);", src).group(1) == str(kv.SP_BATCH)
    assert re.search(r"SP_WAVES_PER_CU = (\d+);", src).group(1) == str(kv.SP_WAVES_PER_CU)
    rows = [r for r in kv.ROWS if r["entry"] == "sum_groups_packed"]
    assert len(rows) == 62
    tiles_widths = set()
    for r in rows:
        m = re.fullmatch(r"\(anonymous namespace\)::k_sum_groups_packed<(\d+), (true|false), (true|false)>", r["kernel"])
        bits, pow2, weighted = int(m.group(1)), m.group(2) == "true", m.group(3) == "true"
        assert r["last"] == "k_sum_groups_packed<%d,%d,%d>" % (bits, pow2, weighted)
        mods = {s["q"] for s in r["shapes"]}
        assert mods == ({1 << bits} if pow2 else {(1 << bits) - 1, (1 << (bits - 1)) + 1}), r["kernel"]
        per = 252 // bits
        slices = -(-per // 32) if per > 36 else 1
        seen = {}
        for s in r["shapes"]:
            N, mod = s["N"], s["q"]
            assert 2 <= N <= 1920 and (mod & (mod - 1) == 0) == pow2 and s["extra"]["weights"] == weighted
            b, pr, al, os_ = (C.c_int() for _ in range(4))
            assert lib.ntru_pack_params(mod - 1, N, C.byref(b), C.byref(pr), C.byref(al), C.byref(os_)) == 0
            assert (b.value, pr.value) == (bits, per), (r["kernel"], s)
            U = os_.value * slices
            layout = "side" if U <= 32 else ("row" if U <= 64 else "tiles")
            assert layout == s["extra"]["layout"], (r["kernel"], s, U)
            lay = kv.packed_layout(bits, N)
            side = 64 // U if U <= 32 else 1
            assert (lay["os"], lay["U"], lay["side"], lay["NT"]) == (os_.value, U, side, 1 if U <= 64 else -(-U // 64))
            seen.setdefault(layout, set()).add(N)
            if layout == "side":
                assert os_.value == 3 and N == 2 * per + 1 and (side == 21) == (slices == 1)
            else:                                   # the smallest N of the layout: one coefficient fewer is one element fewer
                assert kv.packed_layout(bits, N - 1)["layout"] != layout
            for cus in (256, 304, 80, 20):
                first, T, R, Pb, off = kv.many_rows_per_block(bits, N, cus)
                assert first > 0 and R > kv.SP_BATCH * side + side and (R - 1) * Pb < T <= R * Pb
        assert all(len(ns) == 1 for ns in seen.values())
        reachable = {"side", "row"} | ({"tiles"} if (64 // slices) * per + 1 <= 1920 else set())
        assert set(seen) == reachable, (r["kernel"], seen)
        if "tiles" in seen:
            tiles_widths.add(bits)
    assert tiles_widths == {3, 5, 6, 9, 10, 11, 12, 13, 14, 15, 16}
    unpack = kv.BY_KERNEL["(anonymous namespace)::k_unpack_rows"]
    assert [s["q"] for s in unpack["shapes"]] == [1 << b for b in range(1, 17)]
    for s in unpack["shapes"]:
        bits = s["q"].bit_length() - 1
        per = 252 // bits
        assert s["N"] % per and s["N"] > 2 * per                                             # a partial last element
        straddles = [j for j in range(min(per, s["N"])) if j * bits // 64 != (j * bits + bits - 1) // 64]
        assert bool(straddles) == (64 % bits != 0), s
