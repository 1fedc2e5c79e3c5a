"""The centred lift on the GPU (ntru_engine_set_lift, ntru-circom_amd/lift.py): every kernel that lifts, once, against the restatement
(tests/lift_ref.py) at shapes whose addend is not 1; the captured 821 / 4096 cases, which only the centred mode decrypts; the default
mode before and after; a tally with room to count (p = 7 and 5); and the other entry points that run decryptBits.  Every test that sets
a mode does so inside lift.using, which restores it."""
import json
import os

import numpy as np
import pytest

import __graft_entry__ as ge
import lift_ref as ref
from conftest import GOLDEN, PROFILES
from oracle import ntru_oracle as orc

pytestmark = pytest.mark.gpu
pkg = ge.load_package()
lift = pkg.lift


@pytest.fixture(scope="module")
def eng():
    e = pkg.Engine(0)                                   # this module's own engine
    yield e
    e.set_kernel_path(0)


class Dev:
    """Device copies of host arrays through the engine's own allocator."""

    def __init__(self, eng):
        self.eng, self.held = eng, []

    def put(self, a):
        a = np.ascontiguousarray(a)
        p = self.eng.dev_alloc(a.nbytes + 64)
        self.held.append(p)
        self.eng.dev_upload(p, a)
        return p

    def free(self):
        self.eng.synchronize()
        for p in self.held:
            self.eng.dev_free(p)
        self.held = []


def edge_rows(N, q, B):
    """e cycling through 0, 1, q/2 - 1, q/2, q/2 + 1, q - 1, one position further in every row: with f = 1, remainder1 = e, so the lift
    sees the strict threshold from both sides and both ends of the range."""
    vals = np.array([0, 1, q // 2 - 1, q // 2, q // 2 + 1, q - 1], np.int64)
    return vals[(np.arange(N)[None, :] + np.arange(B)[:, None]) % 6].astype(np.uint16)


def one(N):
    f = np.zeros(N, np.int8)
    f[0] = 1
    return f


def same(got, want, tag):
    for g, w, name in zip(got, want, ("value", "quot1", "rem1", "quot2")):
        assert g.dtype == w.dtype and g.tobytes() == w.tobytes(), tag + (name,)


# ---- 1. every kernel that lifts ----------------------------------------------------------------------------------------------------------
SHARED = [  # kernel (last_kernel's name), N, q, p, path, B
    ("k_decrypt<1>", 17, 256, 5, 1, 3),
    ("k_decrypt<3>", 167, 4096, 7, 1, 3),
    ("k_decrypt_t<1,2>", 65, 4096, 3, 2, 5),
    ("k_decrypt_s<9,9>", 575, 4096, 3, 2, 3),
    ("k_decrypt_m", 128, 4096, 3, 4, 33),
    ("k_decrypt_m8", 513, 4096, 3, 0, 95),
]


@pytest.mark.parametrize("kernel,N,q,p,path,B", SHARED)
def test_shared_key_kernels(eng, kernel, N, q, p, path, B):
    assert ref.addend(q, p, ref.CENTRED) != 1
    g = np.random.default_rng(N + q + p)
    fp = g.integers(0, p, N).astype(np.uint8)
    sets = {"f = 1, e at the threshold and the ends": (one(N), edge_rows(N, q, B)),
            "random ternary f, random e": (g.integers(-1, 2, N).astype(np.int8), g.integers(0, q, (B, N)).astype(np.uint16))}
    eng.set_kernel_path(path)
    try:
        for name, (f, e) in sets.items():
            plain = eng.decrypt_batch(N, q, p, f, fp, e)
            assert eng.last_kernel() == kernel
            with lift.using(eng, "centred"):
                centred = eng.decrypt_batch(N, q, p, f, fp, e)
                assert eng.last_kernel() == kernel and lift.get_lift(eng) == 1
            assert lift.get_lift(eng) == 0
            same(centred, ref.decrypt(N, q, p, f, fp, e, ref.CENTRED), (kernel, name, "centred"))
            same(plain, ref.decrypt(N, q, p, f, fp, e, ref.REFERENCE), (kernel, name, "reference"))
            assert centred[1].tobytes() == plain[1].tobytes() and centred[2].tobytes() == plain[2].tobytes()       # quot1, rem1
            assert centred[0].tobytes() != plain[0].tobytes(), (kernel, name)                                      # the modes differ here
            if f is sets["f = 1, e at the threshold and the ends"][0]:
                assert np.array_equal(plain[2], e)                                                                  # remainder1 = e
    finally:
        eng.set_kernel_path(0)


def test_fused_decrypt_and_pack_kernel(eng):
    N, q, p, B = 97, 4096, 3, 33
    g = np.random.default_rng(97)
    fp = g.integers(0, p, N).astype(np.uint8)
    osz = eng.pack_params(p - 1, N)["outputSize"]
    d = Dev(eng)
    try:
        for f, e in ((one(N), edge_rows(N, q, B)), (g.integers(-1, 2, N).astype(np.int8), g.integers(0, q, (B, N)).astype(np.uint16))):
            d_f, d_fp, d_e = d.put(f), d.put(fp), d.put(e)
            d_value, d_packed = d.put(np.full((B, N), 0xEE, np.uint8)), d.put(np.zeros((B, osz, 4), np.uint64))
            got = {}
            for mode in ("reference", "centred"):
                with lift.using(eng, mode):
                    eng.decrypt_pack_batch_dev(N, q, p, d_f, d_fp, d_e, B, d_value, d_packed)
                    assert eng.last_kernel() == "k_decrypt_mp"
                got[mode] = (eng.dev_download(d_value, (B, N), np.uint8), eng.dev_download(d_packed, (B, osz, 4), np.uint64))
                want = ref.decrypt(N, q, p, f, fp, e, mode)[0]
                assert got[mode][0].tobytes() == want.tobytes(), mode
                assert got[mode][1].tobytes() == orc.pack_batch(p - 1, N, want).tobytes(), mode
            assert got["reference"][1].tobytes() != got["centred"][1].tobytes()
    finally:
        d.free()


PERITEM = [  # kernel, N, q, p, path, B
    ("k_decrypt_pi_m", 64, 256, 3, 4, 5),              # k_decrypt_pi_m<true>: one digit plane
    ("k_decrypt_pi_m", 128, 4096, 3, 0, 5),            # k_decrypt_pi_m<false>
    ("peritem_composed(", 17, 256, 5, 0, 3),           # k_pi_lift inside the composed path (q = 64 would not do: 64 = 4 mod 5, addend 1)
]


@pytest.mark.parametrize("kernel,N,q,p,path,B", PERITEM)
def test_per_item_kernels(eng, kernel, N, q, p, path, B):
    assert ref.addend(q, p, ref.CENTRED) != 1
    g = np.random.default_rng(N + q + p)
    f = g.integers(-1, 2, (B, N)).astype(np.int8)
    e = g.integers(0, q, (B, N)).astype(np.uint16)
    f[:2] = one(N)                                      # two rows with f = 1 and e at the threshold and the ends
    e[:2] = edge_rows(N, q, 2)
    fp = g.integers(0, p, (B, N)).astype(np.uint8)
    eng.set_kernel_path(path)
    try:
        plain = eng.decrypt_peritem_batch(N, q, p, f, fp, e)
        assert eng.last_kernel().startswith(kernel)
        with lift.using(eng, "centred"):
            centred = eng.decrypt_peritem_batch(N, q, p, f, fp, e)
            assert eng.last_kernel().startswith(kernel)
    finally:
        eng.set_kernel_path(0)
    same(centred, ref.decrypt_peritem(N, q, p, f, fp, e, ref.CENTRED), (kernel, N, "centred"))
    same(plain, ref.decrypt_peritem(N, q, p, f, fp, e, ref.REFERENCE), (kernel, N, "reference"))
    assert centred[1].tobytes() == plain[1].tobytes() and centred[2].tobytes() == plain[2].tobytes()
    assert centred[0].tobytes() != plain[0].tobytes()
    assert np.array_equal(plain[2][:2], e[:2])


# ---- 2. the captured cases -----------------------------------------------------------------------------------------------------------------
def golden(profile):
    with open(os.path.join(GOLDEN, "scheme_%s.json" % profile)) as fh:
        gold = json.load(fh)
    o, key = gold["options"], gold["keys"][0]
    N = o["N"]
    pad = lambda a, dt: np.array(list(a) + [0] * (N - len(a)), dtype=dt)
    e = np.array([pad(c["decrypt"]["inputs"]["e"], np.uint16) for c in key["cases"]])
    m = np.array([pad(c["m"], np.uint8) for c in key["cases"]])
    return o, key, pad(key["h"], np.uint16), pad(key["f"], np.int8), pad(key["fp"], np.uint8), e, m


def test_centred_decrypt_returns_the_plaintexts_at_821_4096(eng):
    o, key, h, f, fp, e, m = golden("n821_q4096")
    assert e.shape == (7, 821)
    with lift.using(eng, "centred"):
        value, q1, r1, q2 = eng.decrypt_batch(o["N"], o["q"], o["p"], f, fp, e)
    assert np.array_equal(value, m)
    for b, c in enumerate(key["cases"]):                # the first stage is the captured one
        assert q1[b].tolist() + [0] == c["decrypt"]["inputs"]["quotient1"] and r1[b].tolist() + [0] == c["decrypt"]["inputs"]["remainder1"]
    # the NTRU class with the option, and without it (the reference's own objects, as ever)
    opts = dict(o, f=key["f"], fp=key["fp"], h=key["h"])
    centred, plain = pkg.NTRU(opts, engine=eng, lift="centred"), pkg.NTRU(opts, engine=eng)
    for c in key["cases"][:2]:
        out = centred.decryptBits(c["decrypt"]["inputs"]["e"])
        assert out["value"] == pkg.trimPolynomial(c["m"]) and out["params"] == c["decrypt"]["params"]
        assert out["inputs"]["remainder1"] == c["decrypt"]["inputs"]["remainder1"]
        assert plain.decryptBits(c["decrypt"]["inputs"]["e"]) == c["decrypt"]
        assert lift.get_lift(eng) == 0


@pytest.mark.parametrize("profile", [x for x in PROFILES if x != "n821_q4096"])
def test_centred_equals_reference_where_the_addend_is_one(eng, profile):
    o, key, h, f, fp, e, m = golden(profile)
    assert ref.addend(o["q"], o["p"], ref.CENTRED) == 1
    plain = eng.decrypt_batch(o["N"], o["q"], o["p"], f, fp, e)
    with lift.using(eng, "centred"):
        centred = eng.decrypt_batch(o["N"], o["q"], o["p"], f, fp, e)
    same(centred, plain, (profile,))
    assert np.array_equal(plain[0], m)


# ---- 3. the default is untouched -----------------------------------------------------------------------------------------------------------
def test_default_mode_before_and_after():
    fresh = pkg.Engine(0)
    try:
        assert lift.get_lift(fresh) == 0
        o, key, h, f, fp, e, m = golden("n821_q4096")
        before = fresh.decrypt_batch(o["N"], o["q"], o["p"], f, fp, e)
        same(before, orc.decrypt_batch(o["N"], o["q"], o["p"], f, fp, e), ("before",))
        lift.set_lift(fresh, "centred")
        assert lift.get_lift(fresh) == 1
        assert np.array_equal(fresh.decrypt_batch(o["N"], o["q"], o["p"], f, fp, e)[0], m)
        lift.set_lift(fresh, "reference")
        assert lift.get_lift(fresh) == 0
        same(fresh.decrypt_batch(o["N"], o["q"], o["p"], f, fp, e), before, ("after",))
        with pytest.raises(pkg.EngineError, match="NTRU_ERR_ARG"):
            fresh._chk(fresh._lib.ntru_engine_set_lift(fresh._h, 2))
        assert lift.get_lift(fresh) == 0
    finally:
        fresh.close()


# ---- 4. a tally with room to count ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("p,K", [(7, 6), (5, 4)])
def test_tally_counts_in_centred_mode(eng, p, K):
    c = ref.tally_case(p, K)
    N, q, G = c["N"], c["q"], c["G"]
    assert np.abs(c["T"]).max() < q // 2               # the condition under which a correct lift must recover the sums
    packed = pkg.pack_rows(eng, N, q, c["e"])
    with lift.using(eng, "centred"):
        total, value, q1, r1, q2 = eng.tally_decrypt_batch(N, q, p, c["f"], c["fp"], c["e"], K=K)
        total_p, value_p = pkg.tally_decrypt_packed_batch(eng, N, q, p, c["f"], c["fp"], packed, K=K)[:2]
    assert np.array_equal(value, c["counts"]) and np.array_equal(value_p, c["counts"])
    assert total.tobytes() == total_p.tobytes()
    same((value, q1, r1, q2), ref.decrypt(N, q, p, c["f"], c["fp"], total, ref.CENTRED), (p, "witness"))
    plain = eng.tally_decrypt_batch(N, q, p, c["f"], c["fp"], c["e"], K=K)[1]
    plain_p = pkg.tally_decrypt_packed_batch(eng, N, q, p, c["f"], c["fp"], packed, K=K)[1]
    assert not np.array_equal(plain, c["counts"]) and plain.tobytes() == plain_p.tobytes()      # the test tells the modes apart
    ntru = pkg.NTRU(N=N, q=q, p=p, f=c["f"].tolist(), fp=c["fp"].tolist(), engine=eng, lift="centred")
    assert np.array_equal(ntru.tallyBatch(c["e"], offsets=[0, K, 2 * K, 3 * K])["value"], c["counts"])
    assert np.array_equal(ntru.tallyPacked(packed, offsets=[0, K, 2 * K, 3 * K])["value"], c["counts"])
    assert lift.get_lift(eng) == 0


# ---- 5. the other entry points that run decryptBits ------------------------------------------------------------------------------------------
def fresh_batch(o, B, seed):
    g = np.random.default_rng(seed)
    N = o["N"]
    m = g.integers(0, 2, (B, N)).astype(np.uint8)
    r = np.zeros((B, N), np.uint8)
    for b in range(B):
        perm = g.permutation(N)
        r[b, perm[:o["dr"]]], r[b, perm[o["dr"]:2 * o["dr"]]] = 1, o["p"] - 1
    return g, r, m


def test_bytes_pipeline_packed_pitched_and_multi(eng):
    o, key, h, f, fp, _, _ = golden("n821_q4096")
    N, q, p, B = o["N"], o["q"], o["p"], 3
    g, r, m = fresh_batch(o, B, 821)
    W = N // 8
    msg = g.integers(0, 256, (B, W)).astype(np.uint8)
    e_bytes, _ = eng.encrypt_bytes_batch(N, q, W, h, r, msg, want_quot=False)
    e, _ = eng.encrypt_batch(N, q, h, r, m, want_quot=False)
    want = ref.decrypt(N, q, p, f, fp, e, ref.CENTRED)
    assert np.array_equal(want[0], m)                   # no decryption failure among these rows: the plaintexts are what to expect
    # byte messages: honest ciphertexts are flagged in reference mode, and come back in centred mode
    _, flags = eng.decrypt_bytes_batch(N, q, p, W, f, fp, e_bytes)
    assert np.all(flags != 0)
    d = Dev(eng)
    try:
        with lift.using(eng, "centred"):
            out, flags = eng.decrypt_bytes_batch(N, q, p, W, f, fp, e_bytes)
            assert np.array_equal(out, msg) and not flags.any()
            assert np.array_equal(eng.pipeline_batch(N, q, p, h, m, f=f, fp=fp, r=r, want_value=True)["value"], m)
            packed_value = eng.pipeline_batch(N, q, p, h, m, f=f, fp=fp, r=r, want_packed=True)["packed"]     # the fused decrypt + pack
            assert packed_value.tobytes() == orc.pack_batch(p - 1, N, m).tobytes()
            pb = eng.pipeline_bytes_batch(N, q, p, W, h, msg, f=f, fp=fp, r=r, want_msg=True, want_flags=True)
            assert np.array_equal(pb["msg"], msg) and not pb["flags"].any()
            same(pkg.decrypt_packed_batch(eng, N, q, p, f, fp, pkg.pack_rows(eng, N, q, e)), want, ("packed",))
            same(eng.decrypt_batch(N, q, p, f, fp, e), want, ("dense",))
            # the pitched form: rows at ld = N + 3
            ld = N + 3
            wide = np.zeros((B, ld), np.uint16)
            wide[:, :N] = e
            d_f, d_fp, d_e = d.put(f), d.put(fp), d.put(wide)
            d_out = [d.put(np.zeros((B, ld), dt)) for dt in (np.uint8, np.uint16, np.uint16, np.uint8)]
            eng.decrypt_batch_dev(N, q, p, d_f, d_fp, d_e, B, *d_out, ld=ld)
            pitched = [eng.dev_download(ptr, (B, ld), dt)[:, :N] for ptr, dt in zip(d_out, (np.uint8, np.uint16, np.uint16, np.uint8))]
            same([np.ascontiguousarray(x) for x in pitched], want, ("pitched",))
        assert lift.get_lift(eng) == 0
        # the NTRU class on the same engine
        ntru = pkg.NTRU(dict(o, f=key["f"], fp=key["fp"], h=key["h"]), engine=eng, lift="centred")
        data, flags = ntru.decryptBytes(e_bytes, length=B * W)
        assert data == msg.tobytes() and not flags.any()
        assert np.array_equal(ntru.pipeline(m, r=r, decrypt=True)["value"], m)
        assert np.array_equal(ntru.decryptPackedBatch(pkg.pack_rows(eng, N, q, e))["value"], m)
        assert lift.get_lift(eng) == 0
    finally:
        d.free()
    multi = pkg.MultiEngine([0])
    try:
        same(multi.decrypt_batch(N, q, p, f, fp, e), orc.decrypt_batch(N, q, p, f, fp, e), ("multi", "reference"))
        lift.set_lift(multi, "centred")
        same(multi.decrypt_batch(N, q, p, f, fp, e), want, ("multi", "centred"))
    finally:
        multi.close()


def test_per_key_decrypt_through_the_class(eng):
    o, key, h, f, fp, e, m = golden("n821_q4096")
    N, B = o["N"], 3
    keys = {"flags": np.zeros(B, np.uint8), "f": np.tile(f, (B, 1)), "fp": np.tile(fp, (B, 1))}
    ntru = pkg.NTRU(dict(o), engine=eng, lift="centred")
    assert np.array_equal(ntru.decryptBatchPerKey(keys, e[:B])["value"], m[:B])
    assert not np.array_equal(pkg.NTRU(dict(o), engine=eng).decryptBatchPerKey(keys, e[:B])["value"], m[:B])
    assert lift.get_lift(eng) == 0
