"""The lift of decryptBits without a GPU: the restatement (tests/lift_ref.py) against every captured decryptBits case -- addend 1 is the
reference, the centred addend returns the plaintexts of the 821 / 4096 profile and changes nothing where it is 1 -- and the new mode
through its layers: the C ABI's argument checks and exports, lift.py and NTRU(lift=...) against a recording stub library."""
import ctypes as C

import numpy as np
import pytest

import __graft_entry__ as ge
import lift_ref as ref
from conftest import PROFILES, load_golden

pkg = ge.load_package()
engine = pkg.engine
lift = pkg.lift


def cases_of(profile):
    """(N, q, p, f signed [N], fp [N], e [B][N], m [B][N], captured decrypt objects) of a golden profile's first key."""
    gold = load_golden("scheme_%s.json" % profile)
    o, key = gold["options"], gold["keys"][0]
    N, q, p = o["N"], o["q"], o["p"]
    pad = lambda a: list(a) + [0] * (N - len(a))
    e = np.array([pad(c["decrypt"]["inputs"]["e"]) for c in key["cases"]], np.uint16)
    m = np.array([pad(c["m"]) for c in key["cases"]], np.uint8)
    return N, q, p, np.array(pad(key["f"]), np.int8), np.array(pad(key["fp"]), np.uint8), e, m, [c["decrypt"] for c in key["cases"]]


# ---- (a) the restatement ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("profile", PROFILES)
def test_addend_one_is_the_reference(profile):
    N, q, p, f, fp, e, m, captured = cases_of(profile)
    value, q1, r1, q2 = ref.decrypt(N, q, p, f, fp, e, ref.REFERENCE)
    assert len(captured) >= 1
    for b, d in enumerate(captured):
        assert pkg.trimPolynomial(value[b].tolist()) == d["value"]
        for got, name in ((q1, "quotient1"), (r1, "remainder1"), (q2, "quotient2"), (value, "remainder2")):
            assert got[b].tolist() + [0] == d["inputs"][name], (profile, b, name)


def test_centred_addend_returns_the_plaintexts_at_821_4096():
    N, q, p, f, fp, e, m, captured = cases_of("n821_q4096")
    assert (N, q, p) == (821, 4096, 3) and len(captured) == 7 and ref.addend(q, p, ref.CENTRED) == 2
    value = ref.decrypt(N, q, p, f, fp, e, ref.CENTRED)[0]
    assert np.array_equal(value, m)
    # the verbatim lift gives none of them back
    verbatim = ref.decrypt(N, q, p, f, fp, e, ref.REFERENCE)[0]
    assert not any(np.array_equal(verbatim[b], m[b]) for b in range(7))


@pytest.mark.parametrize("profile", [x for x in PROFILES if x != "n821_q4096"])
def test_centred_addend_changes_nothing_where_it_is_one(profile):
    N, q, p, f, fp, e, m, _ = cases_of(profile)
    assert ref.addend(q, p, ref.CENTRED) == 1
    a, b = ref.decrypt(N, q, p, f, fp, e, ref.REFERENCE), ref.decrypt(N, q, p, f, fp, e, ref.CENTRED)
    assert all(x.tobytes() == y.tobytes() for x, y in zip(a, b))
    assert np.array_equal(a[0], m)


def test_the_threshold_is_strict_and_the_addend_is_minus_q():
    for q, p in ((256, 3), (4096, 3), (2048, 3), (256, 5), (4096, 7), (64, 5), (65536, 3)):
        add = ref.addend(q, p, ref.CENTRED)
        assert 1 <= add < p and (add + q) % p == 0
        x = np.array([0, 1, q // 2 - 1, q // 2, q // 2 + 1, q - 1])
        want = [int(v) % p if v <= q // 2 else (int(v) - q) % p for v in x]
        assert ref.lift(x, q, p, add).tolist() == want
        assert ref.lift(x, q, p, 1).tolist() == [int(v) % p if v <= q // 2 else (int(v) + 1) % p for v in x]
    assert [ref.addend(q, 3, ref.CENTRED) for q in (128, 2048, 8192)] == [1, 1, 1]
    assert [ref.addend(q, 3, ref.CENTRED) for q in (256, 1024, 4096, 16384, 65536)] == [2] * 5


@pytest.mark.parametrize("p,K", [(7, 6), (5, 4)])
def test_the_tally_case_counts_under_the_centred_lift_only(p, K):
    """The inputs of the GPU tally tests (lift_ref.tally_case): the noise leaves room (max |T| < q/2), so a correct lift must return the
    sums of the plaintexts; the verbatim lift does not, at any of the groups."""
    c = ref.tally_case(p, K)
    N, q, G = c["N"], c["q"], c["G"]
    assert (N, q) == (167, 2048) and ref.addend(q, p, ref.CENTRED) != 1
    assert np.abs(c["T"]).max() < q // 2 and c["counts"].max() == K == p - 1
    sums = (c["e"].astype(np.int64).reshape(G, K, N).sum(axis=1) % q).astype(np.uint16)
    assert np.array_equal(ref.cyclic(c["f"], sums[0], N) % q, c["T"][0] % q)
    assert np.array_equal(ref.decrypt(N, q, p, c["f"], c["fp"], sums, ref.CENTRED)[0], c["counts"])
    verbatim = ref.decrypt(N, q, p, c["f"], c["fp"], sums, ref.REFERENCE)[0]
    assert not any(np.array_equal(verbatim[g], c["counts"][g]) for g in range(G))


# ---- (b) the binding against a recording stub ------------------------------------------------------------------------------------------
class Stub:
    """Records (name, arguments) of every library call and returns 0; ntru_engine_get_lift answers with what the setter was given."""

    def __init__(self):
        self.calls, self.mode, self.at = [], 0, []                     # at: (name, the mode at the time of the call)

    def __getattr__(self, name):
        def fn(*args):
            args = [a.value if isinstance(a, C.c_void_p) else a for a in args]
            self.calls.append((name, args))
            self.at.append((name, self.mode))
            if name in ("ntru_engine_create", "ntru_multi_create"):
                args[-1]._obj.value = 0x5150
            if name == "ntru_engine_set_lift":
                self.mode = args[1]
            if name == "ntru_engine_get_lift":
                return self.mode
            return 0
        return fn

    def names(self):
        return [n for n, _ in self.calls]

    def setters(self):
        return [(n, a) for n, a in self.calls if n in ("ntru_engine_set_lift", "ntru_multi_set_lift")]


@pytest.fixture()
def stub(monkeypatch):
    s = Stub()
    monkeypatch.setattr(engine, "_LIB", s)
    return s


def test_set_lift_calls_the_library(stub):
    eng = pkg.Engine(0)
    lift.set_lift(eng, "centred")
    assert stub.calls[-1] == ("ntru_engine_set_lift", [0x5150, 1])
    assert lift.get_lift(eng) == 1 and stub.calls[-1] == ("ntru_engine_get_lift", [0x5150])
    lift.set_lift(eng, 0)
    assert stub.calls[-1] == ("ntru_engine_set_lift", [0x5150, 0])
    lift.set_lift(eng, "reference")
    assert stub.calls[-1] == ("ntru_engine_set_lift", [0x5150, 0])
    lift.set_lift(eng, 1)
    assert stub.calls[-1] == ("ntru_engine_set_lift", [0x5150, 1])


def test_a_multi_engine_calls_the_multi_symbol(stub):
    multi = pkg.MultiEngine([0, 0])
    assert lift.get_lift(multi) == 0
    lift.set_lift(multi, "centred")
    assert stub.calls[-1] == ("ntru_multi_set_lift", [0x5150, 1]) and lift.get_lift(multi) == 1
    with lift.using(multi, "reference"):
        assert stub.calls[-1] == ("ntru_multi_set_lift", [0x5150, 0]) and lift.get_lift(multi) == 0
    assert stub.calls[-1] == ("ntru_multi_set_lift", [0x5150, 1])
    assert "ntru_engine_set_lift" not in stub.names()


def test_using_restores_the_mode_also_after_an_exception(stub):
    eng = pkg.Engine(0)
    with lift.using(eng, "centred") as inside:
        assert inside is eng and stub.mode == 1
    assert stub.mode == 0 and [a[1] for _, a in stub.setters()] == [1, 0]
    with pytest.raises(KeyError):
        with lift.using(eng, 1):
            raise KeyError("inside")
    assert stub.mode == 0 and [a[1] for _, a in stub.setters()] == [1, 0, 1, 0]
    # the mode it had, not the default: nested
    lift.set_lift(eng, "centred")
    with lift.using(eng, "reference"):
        assert stub.mode == 0
    assert stub.mode == 1


@pytest.mark.parametrize("bad", ["center", "CENTRED", 2, -1, None, 1.0, True])
def test_an_unknown_mode_is_refused_before_any_library_call(stub, bad):
    eng = pkg.Engine(0)
    n = len(stub.calls)
    with pytest.raises(ValueError, match="lift"):
        lift.set_lift(eng, bad)
    with pytest.raises(ValueError, match="lift"):
        with lift.using(eng, bad):
            pass
    with pytest.raises(ValueError, match="lift"):
        pkg.NTRU(lift=bad, engine=eng)
    assert len(stub.calls) == n


KEY = dict(N=5, q=64, p=3, f=[1, -1, 0, 1, 0], fp=[1, 2, 0, 1, 1], h=[3, 1, 4, 1, 5], dr=1)


def test_ntru_centred_sets_the_mode_around_decrypt_and_restores_it(stub):
    eng = pkg.Engine(0)
    ntru = pkg.NTRU(KEY, engine=eng, lift="centred")
    assert stub.setters() == []                                        # nothing at construction
    out = ntru.decryptBits([1, 2, 3])
    assert [n for n in stub.names() if n != "ntru_engine_create"] == ["ntru_engine_get_lift", "ntru_engine_set_lift", "ntru_decrypt_batch",
                                                                       "ntru_engine_set_lift"]
    assert [a[1] for _, a in stub.setters()] == [1, 0] and stub.mode == 0
    assert out["params"] == [64, ntru.calculateNq(), 3, ntru.calculateNp(), 5]          # params do not know the mode
    # every decrypt-family method, and the decrypt stage of the pipeline only
    calls = {
        "ntru_decrypt_batch": lambda: ntru.decryptStr([1, 2, 3]),
        "ntru_decrypt_bytes_batch": lambda: pkg.NTRU(dict(KEY, N=8, f=[1] * 8, fp=[1] * 8), engine=eng, lift="centred").decryptBytes(np.zeros((2, 8))),
        "ntru_tally_decrypt_batch": lambda: ntru.tallyBatch(np.zeros((4, 5))),
        "ntru_decrypt_peritem_batch": lambda: ntru.decryptBatchPerKey({"flags": np.zeros(2), "f": np.zeros((2, 5)), "fp": np.zeros((2, 5))},
                                                                      np.zeros((2, 5))),
        "ntru_pipeline_batch": lambda: ntru.pipeline(np.zeros((2, 5)), r=np.zeros((2, 5)), decrypt=True),
    }
    for symbol, call in calls.items():
        del stub.calls[:]
        call()
        names = stub.names()
        k = names.index(symbol)
        assert names[k - 1] == "ntru_engine_set_lift" and names[k + 1] == "ntru_engine_set_lift", (symbol, names)
        assert [a[1] for _, a in stub.setters()] == [1, 0], symbol
    del stub.calls[:]
    ntru.pipeline(np.zeros((2, 5)), r=np.zeros((2, 5)))                 # encrypt only: no decrypt stage, no mode
    ntru.encryptBits([1, 0, 1], r=[1, 0, 0, 0, -1])
    assert stub.setters() == [] and "ntru_pipeline_batch" in stub.names()


def test_ntru_centred_packed_calls(stub, monkeypatch):
    eng = pkg.Engine(0)
    monkeypatch.setattr(eng, "pack_params", lambda max_val, n: {"maxInputBits": 6, "numInputsPerOutput": 42, "arrLen": 126, "outputSize": 3})
    ntru = pkg.NTRU(KEY, engine=eng, lift="centred")
    packed = np.zeros((2, 3, 4), np.uint64)
    for symbol, call in (("ntru_tally_decrypt_packed_batch", lambda: ntru.tallyPacked(packed)),
                         ("ntru_decrypt_packed_batch", lambda: ntru.decryptPackedBatch(packed))):
        del stub.calls[:]
        call()
        names = stub.names()
        k = names.index(symbol)
        assert names[k - 1] == "ntru_engine_set_lift" and names[k + 1] == "ntru_engine_set_lift", (symbol, names)
        assert [a[1] for _, a in stub.setters()] == [1, 0]


def test_ntru_default_never_calls_the_setter(stub):
    eng = pkg.Engine(0)
    for ntru in (pkg.NTRU(KEY, engine=eng), pkg.NTRU(KEY, engine=eng, lift="reference"), pkg.NTRU(dict(KEY, lift=0), engine=eng)):
        ntru.decryptBits([1, 2, 3])
        ntru.tallyBatch(np.zeros((4, 5)))
        ntru.pipeline(np.zeros((2, 5)), r=np.zeros((2, 5)), decrypt=True)
    assert "ntru_decrypt_batch" in stub.names()
    assert not [n for n in stub.names() if "lift" in n]


def test_a_shared_engine_is_not_left_in_the_others_mode(stub):
    eng = pkg.Engine(0)
    plain, centred = pkg.NTRU(KEY, engine=eng), pkg.NTRU(KEY, engine=eng, lift="centred")
    plain.decryptBits([1]); centred.decryptBits([1]); plain.decryptBits([1]); centred.decryptBits([1]); plain.decryptBits([1])
    seen = [mode for name, mode in stub.at if name == "ntru_decrypt_batch"]
    assert seen == [0, 1, 0, 1, 0] and stub.mode == 0


# ---- (c) the real library: argument checks need no device ------------------------------------------------------------------------------
def test_the_real_library_exports_and_checks():
    ge.build()
    lib = pkg.load_library()
    for name in ("ntru_engine_set_lift", "ntru_engine_get_lift", "ntru_multi_set_lift"):
        assert hasattr(lib, name) and name in engine._SIGS
        assert getattr(lib, name).argtypes == engine._SIGS[name][1]
    assert lib.ntru_engine_set_lift(None, 1) == 2 and b"NULL" in lib.ntru_last_error()          # NTRU_ERR_ARG
    assert lib.ntru_engine_set_lift(None, 7) == 2 and b"NULL" in lib.ntru_last_error()          # the NULL engine first
    assert lib.ntru_multi_set_lift(None, 1) == 2 and b"NULL" in lib.ntru_last_error()
    assert lib.ntru_engine_get_lift(None) == 0
    header = open(ge.ROOT + "/include/ntru_engine.h").read()
    assert "#define NTRU_LIFT_REFERENCE 0" in header and "#define NTRU_LIFT_CENTRED 1" in header


def test_every_decrypt_row_of_the_variant_table_has_a_shape_that_tells_the_modes_apart():
    """tests/test_kernel_variants_gpu.py decrypts every shape in both lift modes; only where the centred addend is not 1 can a wrong
    addend show.  Exactly the rows whose selection rule admits no such q say so (addend_one_only), and no other row lacks the shape."""
    import kernel_variants as kv
    family = [r for r in kv.ROWS if r["entry"] in kv.LIFT_ENTRIES]
    assert len(family) == 32
    for q, p in ((2048, 3), (8192, 3), (32768, 3), (4096, 3), (16384, 3), (65536, 5)):
        assert kv.lift_addend(q, p) == ref.addend(q, p, ref.CENTRED)
    without = {r["kernel"] for r in family if all(ref.addend(s["q"], s["p"], ref.CENTRED) == 1 for s in r["shapes"])}
    noted = {r["kernel"] for r in kv.ROWS if r["addend_one_only"]}
    assert without == noted == {"k_decrypt_s<9, 7, false>", "k_decrypt_s<11, 7, false>", "k_decrypt_s<11, 7, true>", "k_decrypt_t<1, 1>",
                                "k_decrypt_t<5, 5>", "k_decrypt_t<7, 7>"}
    for k in noted:                                     # their rule: p = 3 and a single q = 2^odd
        assert {(s["q"], s["p"]) for s in kv.BY_KERNEL[k]["shapes"]} in ({(8192, 3)}, {(32768, 3)})
