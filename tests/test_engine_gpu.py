"""GPU parity tests: the HIP path (called through the C ABI) against the pinned CPU oracle and the golden
vectors captured from the reference.  Everything here is bit-exact (integer work)."""
import json
import os

import numpy as np
import pytest

import __graft_entry__ as ge
from oracle import ntru_oracle as orc

pytestmark = pytest.mark.gpu
pkg = ge.load_package()

CONFIGS = [  # (N, q, d) -- the BASELINE.json parameter sets first
    (167, 128, 18), (509, 2048, 169), (821, 4096, 273), (701, 8192, 233), (17, 32, 2),
    (2, 2, 0), (3, 4, 1), (5, 8, 1), (64, 16, 20), (127, 64, 40), (128, 256, 42), (129, 65536, 43),
    (255, 512, 85), (384, 1024, 100), (677, 2048, 225), (1000, 1024, 333), (1279, 4096, 400), (1920, 2048, 600),
]


@pytest.fixture(scope="module")
def eng():
    return pkg.Engine(0)


def ternary_rows(rng, B, N, n1, n2, two=2):
    out = np.zeros((B, N), np.int64)
    for b in range(B):
        perm = rng.permutation(N)
        out[b, perm[:n1]] = 1
        out[b, perm[n1:n1 + n2]] = two
    return out


# ---- golden witnesses through the reference-shaped host mirror ------------------------------------------------

def test_scheme_witnesses_equal_reference(eng, scheme_golden):
    opts = scheme_golden["options"]
    for key in scheme_golden["keys"]:
        n = pkg.NTRU(dict(opts, f=key["f"], fp=key["fp"], fq=key["fq"], g=key["g"], h=key["h"]), engine=eng)
        assert n.I == key["I"]
        for case in key["cases"]:
            it = iter(case["draws"])
            r = pkg.generateCustomArray(opts["N"], opts["dr"], opts["dr"], rand_u32=lambda: next(it))
            enc = n.encryptBits(list(case["m"]), r=r)
            assert enc == case["encrypt"]
            assert n.decryptBits(enc["value"]) == case["decrypt"]
        for s in key["sums"]:
            assert pkg.addCiphertexts(s["e1"], s["e2"], opts["q"], engine=eng) == s["eSum"]
            assert n.decryptBits(s["eSum"]) == s["decrypt"]
        for d in key["degenerate"]:
            assert n.decryptBits(d["e"]) == d["decrypt"]
        assert n.verifyKeysInputs() == key["verifyKeysInputs"]


def test_string_round_trip_like_reference_test(eng, scheme_golden):
    # test/reference.test.js:6-13 with a captured key (key generation is out of scope); q = 1 mod 3 never
    # round-trips in the reference either
    opts = scheme_golden["options"]
    if opts["q"] % 3 != 2 or opts["N"] < 88:
        pytest.skip("no string round trip for this parameter set in the reference")
    key = scheme_golden["keys"][0]
    n = pkg.NTRU(dict(opts, f=key["f"], fp=key["fp"], h=key["h"]), engine=eng)
    assert n.decryptStr(n.encryptStr("Hello World")) == "Hello World"
    other = scheme_golden["keys"][-1] if len(scheme_golden["keys"]) > 1 else None
    if other:
        wrong = pkg.NTRU(dict(opts, f=other["f"], fp=other["fp"], h=key["h"]), engine=eng)
        assert wrong.decryptStr(n.encryptStr("Hello World")) != "Hello World"   # reference.test.js:15-25


def test_pure_functions_equal_reference(eng, pure_golden):
    n_dev = n_big = 0
    for v in pure_golden["multiply"]:                    # incl. the 2^20 products of test/circuits.test.js:60-72
        assert pkg.multiplyPolynomials(v["a"], v["b"], v["p"], engine=eng) == v["out"]
        n_dev += 1
        n_big += v["p"] > 65536
    assert n_dev >= 31 and n_big >= 6
    n_div = 0
    for v in pure_golden["divide"]:
        if "N" not in v:
            continue
        assert pkg.dividePolynomials(v["a"], v["b"], v["p"], engine=eng) == v["out"]
        n_div += 1
    assert n_div >= 60
    for v in pure_golden["divide"]:                      # the generic divisors of test/circuits.test.js:165-170
        if "N" in v:
            continue
        if v.get("error"):
            with pytest.raises(ValueError, match=v["error"].replace(".", r"\.")):
                pkg.dividePolynomials(v["a"], v["b"], v["p"], engine=eng)
        else:
            assert pkg.dividePolynomials(v["a"], v["b"], v["p"], engine=eng) == v["out"]


# ---- the generic family (ntru_generic_*): the reference's own algorithms, quirks and errors included -----------------

def _outcome(fn):
    try:
        return {"out": fn()}
    except ValueError as e:                                # ntru.ReferenceError_: str(e) is the reference's message
        return {"error": str(e)}


def _want(c):
    return {k: c[k] for k in ("out", "error") if k in c}


def test_generic_exports_equal_reference(eng):
    from ntru_circom_amd import ntru as host
    with open(os.path.join(ge.ROOT, "tests", "golden", "generic_functions.json")) as fh:
        g = json.load(fh)
    for c in g["modInverse"]:
        assert host.modInverse(c["a"], c["p"]) == c["out"]
    for c in g["subtract"]:
        assert host.subtractPolynomials(c["a"], c["b"], c["p"]) == c["out"]
    for c in g["scalar"]:
        assert host.multiplyPolynomialsByScalar(c["a"], c["s"], c["p"]) == c["out"]
    for c in g["bigintToBits"]:
        assert host.bigintToBits(int(c["v"])) == c["out"]
    for c in g["bitsToBigInt"]:
        assert str(host.bitsToBigInt(c["bits"])) == c["out"]
    for c in g["multiply"]:
        assert host.multiplyPolynomials(c["a"], c["b"], c["p"], engine=eng) == c["out"]
    for c in g["divide"]:
        assert _outcome(lambda: host.dividePolynomials(c["a"], c["b"], c["p"], engine=eng)) == _want(c), c
    assert g["eea"][0]["out"] == {"gcd": [1], "inverse": [5, 8]}           # index.js:411-423
    for c in g["eea"]:
        assert _outcome(lambda: host.extendedEuclideanAlgorithm(c["a"], c["b"], c["p"], engine=eng)) == _want(c), c
    for c in g["polyInv"]:
        assert _outcome(lambda: host.polyInv(c["f"], c["I"], c["mod"], engine=eng)) == _want(c), c


def test_generic_family_batches_equal_oracle(eng):
    """Whole batches per launch (uniform lengths), against the Python restatement: long division and EEA with signed,
    unreduced operands; polyInv at a real key size; a 2^20-modulus product at N = 701."""
    from oracle import ntru_keygen as kg
    rng = np.random.default_rng(99)
    for p, la, lb, B in ((7, 30, 11, 70), (4096, 50, 20, 33), (2, 40, 41, 65), (1048576, 12, 5, 9)):
        a = rng.integers(-p, 2 * p, (B, la)); b = rng.integers(0, p, (B, lb))
        b[:, -1] = rng.integers(0, 2, B)                   # some leading coefficients vanish, some lack an inverse
        quot, rem, st = eng.generic_divide(a, b, p)
        gcd, inv, st2 = eng.generic_eea(a, b, p)
        for i in range(B):
            try:
                qo, ro = kg._divide(a[i], b[i], p)
                assert st[i] == 0 and quot[i] == qo.tolist() and rem[i] == ro.tolist()
            except ZeroDivisionError:
                assert st[i] == 1
            except ArithmeticError:
                assert st[i] == 2
            try:
                go, io = kg.extended_euclid(a[i], b[i], p, True)
                assert st2[i] == 0 and gcd[i] == go.tolist() and inv[i] == io.tolist()
            except kg.InvalidGcd:
                assert st2[i] == 3
            except ZeroDivisionError:
                assert st2[i] == 1
            except ArithmeticError:
                assert st2[i] == 2
    a = rng.integers(0, 1 << 20, (3, 701)); b = rng.integers(0, 1 << 20, (3, 701))
    prod = eng.generic_multiply(a, b, 1 << 20)
    for i in range(3):
        assert prod[i] == kg._multiply(a[i], b[i], 1 << 20).tolist()
    N = 167
    I = [1] + [0] * (N - 1) + [-1]
    f = rng.integers(-1, 2, (4, N))
    for mod in (3, 128):
        inv, st = eng.generic_poly_inv(f, np.tile(I, (4, 1)), mod)
        for i in range(4):
            try:
                want = kg.poly_inv_generic(f[i], I, mod).tolist()
                assert st[i] == 0 and inv[i] == want
            except kg.InvalidGcd:
                assert st[i] == 3


# ---- random batches against the oracle, fixed-stride layout ----------------------------------------------------

@pytest.mark.parametrize("N,q,d", CONFIGS)
def test_encrypt_decrypt_batches_equal_oracle(eng, N, q, d):
    rng = np.random.default_rng(N * 7919 + q)
    p = 3
    B = 5 if N > 1000 else (67 if N > 300 else 203)
    h = rng.integers(0, q, N)
    f = ternary_rows(rng, 1, N, min(d + 1, N), min(d, N - min(d + 1, N)), two=-1)[0]
    fp = rng.integers(0, p, N)
    r = ternary_rows(rng, B, N, d, d)
    m = rng.integers(0, 3, (B, N))
    m[0] = 0
    m[-1] = 255                                             # any byte is added mod q
    e, quot = eng.encrypt_batch(N, q, h, r, m)
    e_o, quot_o = orc.encrypt_batch(N, q, h, r, m)
    assert np.array_equal(e, e_o) and np.array_equal(quot, quot_o)
    e2, none = eng.encrypt_batch(N, q, h, r, m, want_quot=False)
    assert none is None and np.array_equal(e2, e_o)
    # decrypt: fresh ciphertexts plus arbitrary values in [0,q)
    ein = np.concatenate([e_o, rng.integers(0, q, (7, N)), np.full((1, N), q - 1), np.zeros((1, N), np.int64)])
    got = eng.decrypt_batch(N, q, p, f, fp, ein)
    want = orc.decrypt_batch(N, q, p, f, fp, ein)
    for g_, w_, name in zip(got, want, ("value", "quotient1", "remainder1", "quotient2")):
        assert np.array_equal(g_, w_), name
    v_only = eng.decrypt_batch(N, q, p, f, fp, ein, want_witness=False)
    assert np.array_equal(v_only[0], want[0]) and v_only[1] is None


@pytest.mark.parametrize("N,q", [(821, 4096), (701, 8192), (509, 2048), (677, 2048), (449, 8192), (128, 16384),
                                  (384, 32)])
def test_field_overflow_extremes(eng, N, q):
    """Worst cases for the add path's 16-bit field budget: every step adds a window of all (q-1) into the same
    accumulator set (stepping operand all ones / all twos / all -1), on every kernel family."""
    p = 3
    hmax = np.full(N, q - 1)
    r = np.stack([np.ones(N), np.full(N, 2), np.arange(N) % 3, (np.arange(N) + 1) % 2 * 2]).astype(np.int64)
    m = np.full((4, N), 2)
    for path in (0, 1, 2, 3, 4):
        eng.set_kernel_path(path)
        try:
            e, quot = eng.encrypt_batch(N, q, hmax, r, m)
            e_o, quot_o = orc.encrypt_batch(N, q, hmax, r, m)
            assert np.array_equal(e, e_o) and np.array_equal(quot, quot_o), path
            for fvec in (np.ones(N), -np.ones(N), (np.arange(N) % 3) - 1):
                for fpvec in (np.full(N, 2), np.ones(N), np.arange(N) % 3):
                    ein = np.stack([np.full(N, q - 1), np.arange(N) % q, np.full(N, q // 2 + 1), np.zeros(N)]).astype(np.int64)
                    got = eng.decrypt_batch(N, q, p, fvec, fpvec, ein)
                    want = orc.decrypt_batch(N, q, p, fvec, fpvec, ein)
                    for g_, w_ in zip(got, want):
                        assert np.array_equal(g_, w_), path
        finally:
            eng.set_kernel_path(0)


def test_kernel_families_agree(eng):
    rng = np.random.default_rng(99)
    for N, q, d in ((821, 4096, 273), (701, 8192, 233), (509, 2048, 169)):
        h = rng.integers(0, q, N); fp = rng.integers(0, 3, N)
        f = ternary_rows(rng, 1, N, d, d - 1, two=-1)[0]
        r = ternary_rows(rng, 9, N, d, d); m = rng.integers(0, 2, (9, N))
        outs = []
        for path in (1, 2, 3, 4, 5, 0):
            eng.set_kernel_path(path)
            e, quot = eng.encrypt_batch(N, q, h, r, m)
            dec = eng.decrypt_batch(N, q, 3, f, fp, e)
            outs.append((e, quot) + dec)
        eng.set_kernel_path(0)
        for o in outs[1:]:
            for a, b in zip(outs[0], o):
                assert np.array_equal(a, b)


@pytest.mark.parametrize("N,q,d", [(17, 32, 2), (31, 64, 5), (32, 128, 6), (33, 32, 7), (64, 8192, 20), (65, 4096, 21),
                                   (167, 128, 18), (509, 2048, 169), (701, 8192, 233), (821, 4096, 273),
                                   (1021, 4096, 300), (1022, 2048, 300), (1023, 8192, 300), (1024, 8192, 300)])
@pytest.mark.parametrize("path", [4, 5])
def test_matrix_core_path_equals_oracle(eng, N, q, d, path):
    """Family 4 forced (ntru_engine_set_kernel_path 4: two workgroups per CU; 5: lock-step decrypt), including sizes the
    automatic choice leaves to other families, batches that do not fill a 32-row block, and h at the corners of the
    digit-plane range."""
    rng = np.random.default_rng(N * 31 + q)
    p = 3
    eng.set_kernel_path(path)
    two_groups_fit = (N + 31) // 32 < 32                   # 32 column tiles: 160 KB of LDS do not hold two groups
    dma = ("k_encrypt_md",) if N + 3 <= 1024 else ("k_encrypt_md", "k_encrypt_m")   # direct-to-LDS loads: rows that fit one 1024-byte instruction
    try:
        for B in (1, 31, 33, 70):
            h = rng.integers(0, q, N)
            h[:6] = np.array([q // 2 - 65, q // 2 - 64, q // 2 - 1, q // 2, q - 1, 0]) % q
            f = ternary_rows(rng, 1, N, min(d + 1, N), min(d, N - min(d + 1, N)), two=-1)[0]
            fp = rng.integers(0, p, N)
            r = ternary_rows(rng, B, N, d, d)
            m = rng.integers(0, 256, (B, N))
            e, quot = eng.encrypt_batch(N, q, h, r, m)
            assert eng.last_kernel() in {4: ("k_encrypt_m",), 5: dma}[path]
            e_o, quot_o = orc.encrypt_batch(N, q, h, r, m)
            assert np.array_equal(e, e_o) and np.array_equal(quot, quot_o), B
            e_only, _ = eng.encrypt_batch(N, q, h, r, m, want_quot=False)
            assert np.array_equal(e_only, e_o), B
            ein = e_o.copy()
            ein[-1] = rng.integers(0, q, N)
            ein[0, :4] = (q - 1, 0, q // 2, q // 2 + 1)
            got = eng.decrypt_batch(N, q, p, f, fp, ein)
            assert eng.last_kernel() == ("k_decrypt_m8" if path == 5 and two_groups_fit else "k_decrypt_m")
            want = orc.decrypt_batch(N, q, p, f, fp, ein)
            for g_, w_, name in zip(got, want, ("value", "quotient1", "remainder1", "quotient2")):
                assert np.array_equal(g_, w_), (B, name)
            v_only = eng.decrypt_batch(N, q, p, f, fp, ein, want_witness=False)
            assert np.array_equal(v_only[0], want[0])
    finally:
        eng.set_kernel_path(0)


@pytest.mark.parametrize("path", [4, 5])
def test_matrix_core_path_random_parameter_sweep(eng, path):
    """Differential sweep: 40 random (N, q, B) with N in [2, 1024] (odd and even, around the 32-tile boundaries), q any
    power of two up to 8192, ragged B; matrix-core family (forced) against the CPU oracle, all outputs."""
    rng = np.random.default_rng(20240)
    p = 3
    eng.set_kernel_path(path)
    try:
        for trial in range(40):
            N = int(rng.choice([rng.integers(2, 1025), 32 * rng.integers(1, 33) + rng.integers(-1, 2)]))
            N = max(2, min(1024, N))
            q = 1 << int(rng.integers(1, 14))
            B = int(rng.integers(1, 100))
            d = max(0, min(N // 3, N - 1))
            h = rng.integers(0, q, N)
            f = ternary_rows(rng, 1, N, min(d + 1, N), min(d, N - min(d + 1, N)), two=-1)[0]
            fp = rng.integers(0, p, N)
            r = ternary_rows(rng, B, N, d, d)
            m = rng.integers(0, 256, (B, N))
            e, quot = eng.encrypt_batch(N, q, h, r, m)
            assert eng.last_kernel() in {4: ("k_encrypt_m",), 5: ("k_encrypt_md", "k_encrypt_m")}[path]
            e_o, quot_o = orc.encrypt_batch(N, q, h, r, m)
            assert np.array_equal(e, e_o) and np.array_equal(quot, quot_o), (N, q, B)
            ein = np.concatenate([e_o, rng.integers(0, q, (3, N))])
            got = eng.decrypt_batch(N, q, p, f, fp, ein)
            want = orc.decrypt_batch(N, q, p, f, fp, ein)
            for g_, w_, name in zip(got, want, ("value", "quotient1", "remainder1", "quotient2")):
                assert np.array_equal(g_, w_), (N, q, B, name)
    finally:
        eng.set_kernel_path(0)


@pytest.mark.parametrize("N,q,B", [(167, 128, 32 * 256 * 3 + 5), (821, 4096, 32 * 256 * 2 + 33), (65, 64, 32 * 256 + 1),
                                   (65, 64, 32 * 256 * 5 + 9), (33, 32, 32 * 256 * 5 + 3)])   # waves WITHOUT a strip (NT < 4) on their second trip
def test_role_split_kernels_many_row_blocks_per_workgroup(eng, N, q, B):
    """Batches of more than two row blocks per CU: every trip of the persistent loops after the first (k_encrypt_md's rows
    requested into LDS one trip ahead, k_decrypt_m8's two lock-step groups); ragged last row block."""
    rng = np.random.default_rng(N + B)
    p, d = 3, N // 3
    h = rng.integers(0, q, N); fp = rng.integers(0, p, N)
    f = ternary_rows(rng, 1, N, d, d - 1, two=-1)[0]
    r = np.zeros((B, N), np.int64)
    r[:, :d] = 1; r[:, d:2 * d] = 2
    r = rng.permuted(r, axis=1)
    m = rng.integers(0, 3, (B, N))
    e_o, quot_o = orc.encrypt_batch(N, q, h, r, m)
    want = orc.decrypt_batch(N, q, p, f, fp, e_o)
    variants = ((5, "k_encrypt_md", "k_decrypt_m8"),)       # every trip of k_encrypt_md but the first works on rows loaded straight into LDS
    for path, ename, dname in variants:
        eng.set_kernel_path(path)
        try:
            e, quot = eng.encrypt_batch(N, q, h, r, m)
            assert eng.last_kernel() == ename
            got = eng.decrypt_batch(N, q, p, f, fp, e)
            assert eng.last_kernel() == dname
        finally:
            eng.set_kernel_path(0)
        assert np.array_equal(e, e_o) and np.array_equal(quot, quot_o), path
        for g_, w_, name in zip(got, want, ("value", "quotient1", "remainder1", "quotient2")):
            assert np.array_equal(g_, w_), (path, name)


@pytest.mark.parametrize("path", [0])
@pytest.mark.parametrize("N,q", [(821, 4096), (167, 128), (701, 8192), (1021, 2048), (1022, 4096), (1023, 8192), (1024, 1024)])   # N >= 1022: a row + its byte phase exceeds one 1024-byte direct-to-LDS instruction
def test_device_pointers_at_any_alignment(eng, N, q, path):
    """The *_dev entry points take any pointer: the matrix-core kernels read rows through aligned chunks + shifts and
    write through byte/short stores, so buffers that start at odd byte offsets must give the same results."""
    import torch
    dev = torch.device("cuda:0")
    rng = np.random.default_rng(N + q)
    p, B, d = 3, 45, N // 3
    h = rng.integers(0, q, N); f = ternary_rows(rng, 1, N, d, d - 1, two=-1)[0]; fp = rng.integers(0, p, N)
    r = ternary_rows(rng, B, N, d, d); m = rng.integers(0, 256, (B, N))
    e_o, quot_o = orc.encrypt_batch(N, q, h, r, m)
    want = orc.decrypt_batch(N, q, p, f, fp, e_o)
    eng.set_kernel_path(path)
    eng.set_stream(torch.cuda.current_stream().cuda_stream)
    try:
        for off in (1, 2, 3, 5, 14, 15):
            def place(a, dtype, elt):                    # copy `a` into a byte buffer at byte offset off * elt' (u16 stays 2-aligned)
                raw = np.ascontiguousarray(a.astype(dtype)).view(np.uint8).ravel()
                o = off * elt
                buf = torch.zeros(raw.size + 64, dtype=torch.uint8, device=dev)
                buf[o:o + raw.size] = torch.from_numpy(raw).to(dev)
                return buf, buf.data_ptr() + o
            def out(nbytes, elt):
                buf = torch.full((nbytes + 64,), 0xAB, dtype=torch.uint8, device=dev)
                return buf, buf.data_ptr() + off * elt
            hb, hp = place(h, np.uint16, 2); rb, rp = place(r, np.uint8, 1); mb, mp = place(m, np.uint8, 1)
            fb, fpp = place(f, np.int8, 1); fpb, fppp = place(fp, np.uint8, 1)
            eb, ep = out(2 * B * N, 2); qb, qp = out(2 * B * N, 2)
            eng.encrypt_batch_dev(N, q, hp, rp, mp, B, ep, qp)
            vb, vp = out(B * N, 1); q1b, q1p = out(2 * B * N, 2); r1b, r1p = out(2 * B * N, 2); q2b, q2p = out(B * N, 1)
            eng.decrypt_batch_dev(N, q, p, fpp, fppp, ep, B, vp, q1p, r1p, q2p)
            torch.cuda.synchronize()
            def back(buf, elt, dtype, n):
                o = off * elt
                a = buf.cpu().numpy()
                assert (a[:o] == 0xAB).all() and (a[o + n * np.dtype(dtype).itemsize:] == 0xAB).all()   # nothing outside
                return a[o:o + n * np.dtype(dtype).itemsize].view(dtype).reshape(B, N)
            assert np.array_equal(back(eb, 2, np.uint16, B * N), e_o), off
            assert np.array_equal(back(qb, 2, np.uint16, B * N), quot_o), off
            got = (back(vb, 1, np.uint8, B * N), back(q1b, 2, np.uint16, B * N), back(r1b, 2, np.uint16, B * N),
                   back(q2b, 1, np.uint8, B * N))
            for g_, w_ in zip(got, want):
                assert np.array_equal(g_, w_), off
    finally:
        eng.set_kernel_path(0)
        eng.set_stream(None)


@pytest.mark.parametrize("N,q,ld", [(821, 4096, 832), (821, 4096, 822), (821, 4096, 1024), (167, 128, 192), (701, 8192, 704),
                                    (509, 2048, 509), (64, 32, 80), (33, 8192, 47)])
@pytest.mark.parametrize("path", [0])
def test_pitched_rows_equal_oracle(eng, N, q, ld, path):
    """ntru_*_batch_pitched_dev: rows at a pitch of ld >= N elements.  Pad elements of the inputs hold garbage and must
    not reach any result; pad elements of the outputs must stay untouched; a ragged batch (B % 32 != 0) must not write
    past row B - 1."""
    import torch
    dev = torch.device("cuda:0")
    rng = np.random.default_rng(N * 7 + ld)
    p, B, d = 3, 77, N // 3
    h = rng.integers(0, q, N); f = ternary_rows(rng, 1, N, d, d - 1, two=-1)[0]; fp = rng.integers(0, p, N)
    r = ternary_rows(rng, B, N, d, d); m = rng.integers(0, 256, (B, N))
    e_o, quot_o = orc.encrypt_batch(N, q, h, r, m)
    want = orc.decrypt_batch(N, q, p, f, fp, e_o)

    def pitched(a, dtype, hi):                            # [B][ld] with random pads, plus two guard rows behind the batch
        buf = rng.integers(0, hi, (B + 2, ld)).astype(dtype)
        buf[:B, :N] = a
        return torch.from_numpy(buf).to(dev)

    def outbuf(dtype, fill):
        return torch.full((B + 2, ld), fill, dtype=dtype, device=dev)

    def check(t, want_rows, fill, what):
        a = t.cpu().numpy().astype(np.int64) & (0xFFFF if t.dtype == torch.int16 else 0xFF)
        assert np.array_equal(a[:B, :N], want_rows), what
        assert (a[:B, N:] == fill).all() and (a[B:] == fill).all(), what + ": wrote outside the rows"

    dh = torch.from_numpy(h.astype(np.int16)).to(dev); df = torch.from_numpy(f.astype(np.int8)).to(dev)
    dfp = torch.from_numpy(fp.astype(np.uint8)).to(dev)
    dr = pitched(r, np.uint8, 256); dm = pitched(m, np.uint8, 256)
    de = outbuf(torch.int16, 0x5A5A); dq = outbuf(torch.int16, 0x5A5A)
    eng.set_kernel_path(path)
    eng.set_stream(torch.cuda.current_stream().cuda_stream)
    try:
        eng.encrypt_batch_dev(N, q, dh.data_ptr(), dr.data_ptr(), dm.data_ptr(), B, de.data_ptr(), dq.data_ptr(), ld=ld)
        torch.cuda.synchronize()
        check(de, e_o, 0x5A5A, "e"); check(dq, quot_o, 0x5A5A, "quotE")
        # decrypt reads the pitched ciphertext it just got (pads = 0x5A5A garbage)
        dv = outbuf(torch.uint8, 0xA5); dq2 = outbuf(torch.uint8, 0xA5)
        dq1 = outbuf(torch.int16, 0x5A5A); dr1 = outbuf(torch.int16, 0x5A5A)
        eng.decrypt_batch_dev(N, q, p, df.data_ptr(), dfp.data_ptr(), de.data_ptr(), B, dv.data_ptr(), dq1.data_ptr(),
                              dr1.data_ptr(), dq2.data_ptr(), ld=ld)
        torch.cuda.synchronize()
        check(dv, want[0], 0xA5, "value"); check(dq1, want[1], 0x5A5A, "quot1")
        check(dr1, want[2], 0x5A5A, "rem1"); check(dq2, want[3], 0xA5, "quot2")
        # value-only mode on pitched rows
        dv2 = outbuf(torch.uint8, 0xA5)
        eng.decrypt_batch_dev(N, q, p, df.data_ptr(), dfp.data_ptr(), de.data_ptr(), B, dv2.data_ptr(), ld=ld)
        torch.cuda.synchronize()
        check(dv2, want[0], 0xA5, "value (value-only)")
    finally:
        eng.set_kernel_path(0)
        eng.set_stream(None)


def test_pitched_rows_are_refused_off_the_matrix_core_path(eng):
    """Only the matrix-core kernels take a pitch: anything else must fail loudly, not fall back to dense rows."""
    import torch
    dev = torch.device("cuda:0")
    N, q, ld, B = 167, 128, 192, 4
    z8 = torch.zeros((B, ld), dtype=torch.uint8, device=dev); z16 = torch.zeros((B, ld), dtype=torch.int16, device=dev)
    dh = torch.zeros(N, dtype=torch.int16, device=dev)
    eng.set_kernel_path(2)
    try:
        with pytest.raises(pkg.EngineError):
            eng.encrypt_batch_dev(N, q, dh.data_ptr(), z8.data_ptr(), z8.data_ptr(), B, z16.data_ptr(), None, ld=ld)
    finally:
        eng.set_kernel_path(0)
    with pytest.raises(pkg.EngineError):                  # ld < N
        eng.encrypt_batch_dev(N, q, dh.data_ptr(), z8.data_ptr(), z8.data_ptr(), B, z16.data_ptr(), None, ld=N - 1)
    with pytest.raises(pkg.EngineError):                  # q too wide for two int8 digit planes
        eng.encrypt_batch_dev(N, 16384, dh.data_ptr(), z8.data_ptr(), z8.data_ptr(), B, z16.data_ptr(), None, ld=ld)


def test_public_key_batch_equals_reference_and_oracle(eng, scheme_golden):
    """generatePublicKeyH on the device: captured keys (through the host mirror and the batch entry point) and random
    per-item operands against the oracle."""
    o = scheme_golden["options"]
    N, q, p = o["N"], o["q"], o["p"]
    pad = lambda a: list(a) + [0] * (N - len(a))
    keys = scheme_golden["keys"]
    for key in keys:
        n = pkg.NTRU(dict(o, f=key["f"], fq=key["fq"], g=key["g"]), engine=eng)
        n.generatePublicKeyH()
        assert n.h == key["h"]
    h = eng.public_key_batch(N, q, p, [pad(k["fq"]) for k in keys], [pad(k["g"]) for k in keys])
    assert eng.last_kernel().startswith("k_public_key")
    for row, key in zip(h, keys):
        assert orc.trim(row.tolist()) == list(key["h"])
    rng = np.random.default_rng(N + q)
    B = 77
    fq = rng.integers(0, q, (B, N)); g = ternary_rows(rng, B, N, N // 4, N // 4, two=-1)
    assert np.array_equal(eng.public_key_batch(N, q, p, fq, g), orc.public_key_batch(N, q, p, fq, g))
    with pytest.raises(ValueError, match="missing private key G"):
        pkg.NTRU(dict(o, f=keys[0]["f"], fq=keys[0]["fq"]), engine=eng).generatePublicKeyH()


def test_key_inversion_equals_reference_keys(eng, scheme_golden):
    """loadPrivateKeyF on the device (ntru_invert_key_batch): fq and fp of every captured key from its f, then the public
    key from (fq, g): the whole key schedule except the random draws."""
    o = scheme_golden["options"]
    N, q, p = o["N"], o["q"], o["p"]
    pad = lambda a: list(a) + [0] * (N - len(a))
    keys = scheme_golden["keys"]
    fq, fp, flags = eng.invert_key_batch(N, q, p, [pad(k["f"]) for k in keys])
    assert not flags.any()
    for i, key in enumerate(keys):
        assert fq[i].tolist() == pad(key["fq"]) and fp[i].tolist() == pad(key["fp"])
        n = pkg.NTRU(dict(o, g=key["g"]), engine=eng)
        n.loadPrivateKeyF(key["f"])
        assert n.fq == key["fq"] and n.fp == key["fp"]
        n.generatePublicKeyH()
        assert n.h == key["h"]
        assert n.verifyKeysInputs() == key["verifyKeysInputs"]


def test_fresh_key_round_trip_like_reference_test(eng):
    """test/reference.test.js:6-14 with nothing supplied: generatePrivateKeyF + generateNewPublicKeyGH on the device,
    verifyKeysInputs accepts the key, a string survives encrypt + decrypt (q = 128 is 2 mod 3: SURVEY 0.4)."""
    n = pkg.NTRU(dict(N=167, q=128, p=3, df=61, dg=20, dr=18), engine=eng)
    n.generatePrivateKeyF()
    n.generateNewPublicKeyGH()
    n.verifyKeysInputs()
    assert n.decryptStr(n.encryptStr("Hello World")) == "Hello World"


def test_key_inversion_captured_cases_and_random_keys(eng):
    """tests/golden/keygen_cases.json: for every f that IS a unit mod 2 and mod 3 the device equals the reference; for the
    others the matching flag is set (the host mirrors then run the reference's own sequence on the generic family).
    Random keys at BASELINE sizes: f * fq = 1 mod q and f * fp = 1 mod p through the product entry point."""
    from oracle import ntru_keygen as kg
    with open(os.path.join(os.path.dirname(__file__), "golden", "keygen_cases.json")) as fh:
        cases = json.load(fh)["cases"]
    by = {}
    for c in cases:
        by.setdefault((c["N"], c["q"], c["p"]), []).append(c)
    n_unit = n_flag = 0
    for (N, q, p), cs in by.items():
        fq, fp, flags = eng.invert_key_batch(N, q, p, [c["f"] for c in cs])
        for i, c in enumerate(cs):
            u2, u3 = kg.is_unit(c["f"], N, 2), kg.is_unit(c["f"], N, 3)
            assert bool(flags[i] & pkg.engine.FLAG_NOT_UNIT_MOD2) == (not u2), (N, c["f"])
            assert bool(flags[i] & pkg.engine.FLAG_NOT_UNIT_MODP) == (not u3), (N, c["f"])
            if u2 and u3:
                pad = lambda a: list(a) + [0] * (N - len(a))
                assert "error" not in c
                assert fq[i].tolist() == pad(c["fq"]) and fp[i].tolist() == pad(c["fp"])
                n_unit += 1
            else:
                n_flag += 1
    assert n_unit >= 30 and n_flag >= 40
    rng = np.random.default_rng(8)
    for N, q, d in ((821, 4096, 273), (701, 8192, 233), (509, 2048, 169), (1024, 65536, 341)):
        B = 70
        f = ternary_rows(rng, B, N, d, d - 1, two=-1)
        fq, fp, flags = eng.invert_key_batch(N, q, 3, f)
        ok = flags == 0
        assert ok.any()
        for i in np.nonzero(~ok)[0][:2]:                     # a flagged key really is a non-unit (slow CPU check: two per size)
            assert not (kg.is_unit(f[i], N, 2) and kg.is_unit(f[i], N, 3))
            assert bool(flags[i] & pkg.engine.FLAG_NOT_UNIT_MOD2) == (not kg.is_unit(f[i], N, 2))
        one = np.zeros(N, np.int64); one[0] = 1
        _, rem = eng.polymul_split(N, q, (f % q).astype(np.uint16), fq)
        assert all(np.array_equal(rem[i], one) for i in range(B) if ok[i])
        _, rem3 = orc.polymul_split_batch(N, 3, f % 3, fp)
        assert all(np.array_equal(rem3[i], one) for i in range(B) if ok[i])


def test_products_modulo_x_n_minus_1_on_one_matrix_instruction_per_distance(eng):
    """`pi_product_cyc` (k_product_tern_m: the public key; k_newton_round_m: the lifting of the inverse modulo 2): every class of N --
    two tiles, a multiple of 32 (nothing moved), one past it (31 places), one short of it, 1024 -- on one and on two digit planes.
    Public keys against the oracle and the vector-ALU kernel; inverses through f * fq = 1 (the split product) and the oracle's polyInv."""
    from oracle import ntru_keygen as kg
    rng = np.random.default_rng(55)
    one_of = lambda N: np.eye(1, N, dtype=np.int64)[0]
    for N in (64, 65, 95, 96, 97, 127, 128, 167, 509, 640, 677, 701, 821, 992, 993, 1023, 1024):
        for q in (128, 2048, 8192):
            B = int(rng.integers(3, 70)); d = N // 3
            fq = rng.integers(0, q, (B, N)); g = ternary_rows(rng, B, N, d, d, two=-1)
            fq[0] = q - 1; g[0] = -1; fq[1] = 0; fq[1, N - 1] = q - 1; g[1] = 0; g[1, N - 1] = 1      # extremes; x^(N-1) * x^(N-1) wraps to x^(N-2)
            eng.set_kernel_path(4)
            got = eng.public_key_batch(N, q, 3, fq, g)
            assert eng.last_kernel() == "k_public_key_m", (N, q, eng.last_kernel())
            eng.set_kernel_path(1)
            alt = eng.public_key_batch(N, q, 3, fq, g)
            eng.set_kernel_path(0)
            want = orc.public_key_batch(N, q, 3, fq, g)
            assert np.array_equal(got, want), (N, q)
            assert np.array_equal(alt, want), (N, q, "vector-ALU kernel")
        q = 4096
        B = 40
        f = ternary_rows(rng, B, N, N // 3, N // 3 - 1, two=-1)
        eng.set_kernel_path(4)
        fq, fp, flags = eng.invert_key_batch(N, q, 3, f)
        eng.set_kernel_path(0)
        ok = flags == 0
        assert ok.sum() >= (1 if N % 2 == 0 else 5), (N, int(ok.sum()))
        _, rem = orc.polymul_split_batch(N, q, f % q, fq)
        assert all(np.array_equal(rem[i], one_of(N)) for i in range(B) if ok[i]), N
        i = int(np.nonzero(ok)[0][0])
        if N <= 200:                                         # the oracle's polyInv (slow): one key per small size
            wq, wp = kg.load_private_key(f[i], N, q, 3)
            assert np.array_equal(fq[i], wq % q) and np.array_equal(fp[i], wp % 3), N


def test_key_inversion_whole_block_output_equals_the_per_coefficient_path(eng):
    """k_invert_key writes a whole block of 64 keys through LDS as one contiguous run when the outputs are 16-byte aligned, and one
    coefficient at a time otherwise (unaligned outputs, the partial last block, N < 32): both on the same keys -- with non-units
    among them, whose rows are zero -- must agree byte for byte, for register planes (N = 107, 509, 821; N = 1000: GF(2) only) and LDS
    planes (N = 1024, 1919)."""
    import torch
    dev = torch.device("cuda", 0)
    rng = np.random.default_rng(77)
    for N, q, d in ((107, 64, 35), (509, 2048, 169), (821, 4096, 273), (1000, 2048, 333), (1024, 2048, 341), (1919, 2048, 600), (17, 32, 5)):
        B = 64 * 3 + 5
        f = ternary_rows(rng, B, N, d, d - 1, two=-1).astype(np.int8)
        f[3] = 0                                             # not a unit modulo anything
        f[70] = 0; f[70, 0] = 1; f[70, 1] = 1                # 1 + x: f(1) = 2, not a unit modulo 2
        f[130] = 0; f[130, 0] = 1; f[130, 1] = 1; f[130, 2] = 1   # 1 + x + x^2: f(1) = 3, not a unit modulo 3
        f[140:150] = rng.integers(-128, 128, size=(10, N), dtype=np.int64).astype(np.int8)   # any int8 is reduced modulo 2 / 3
        fd = torch.from_numpy(f).to(dev)
        out = {}
        for shift in (0, 1):                                 # element offset of the outputs: 0 = aligned, 1 = 2 / 1 byte(s) off
            fq = torch.zeros(B * N + 8, dtype=torch.int16, device=dev); fp = torch.zeros(B * N + 16, dtype=torch.uint8, device=dev)
            fl = torch.zeros(B, dtype=torch.uint8, device=dev)
            assert fq.data_ptr() % 16 == 0 and fp.data_ptr() % 16 == 0
            eng.invert_key_batch_dev(N, q, 3, fd.data_ptr(), B, fq.data_ptr() + 2 * shift, fp.data_ptr() + shift, fl.data_ptr())
            torch.cuda.synchronize()
            out[shift] = (fq[shift:shift + B * N].cpu().numpy().reshape(B, N), fp[shift:shift + B * N].cpu().numpy().reshape(B, N),
                          fl.cpu().numpy())
            assert int(fq[shift + B * N:].abs().sum()) == 0 and int(fp[shift + B * N:].sum()) == 0     # nothing past the last row
        # ... and the same for the INPUT side (16-byte pieces of the block's run through LDS, or a byte per coefficient): f one byte off
        fpad = torch.zeros(B * N + 16, dtype=torch.int8, device=dev)
        fpad[1:1 + B * N] = fd.reshape(-1)
        fq = torch.zeros(B * N, dtype=torch.int16, device=dev); fp = torch.zeros(B * N, dtype=torch.uint8, device=dev)
        fl = torch.zeros(B, dtype=torch.uint8, device=dev)
        eng.invert_key_batch_dev(N, q, 3, fpad.data_ptr() + 1, B, fq.data_ptr(), fp.data_ptr(), fl.data_ptr())
        torch.cuda.synchronize()
        out[2] = (fq.cpu().numpy().reshape(B, N), fp.cpu().numpy().reshape(B, N), fl.cpu().numpy())
        for other in (1, 2):
            for a, b in zip(out[0], out[other]):
                assert np.array_equal(a, b), (N, other)
        fq, fp, fl = out[0]
        assert fl[3] & pkg.engine.FLAG_NOT_UNIT_MOD2 and fl[3] & pkg.engine.FLAG_NOT_UNIT_MODP
        assert fl[70] & pkg.engine.FLAG_NOT_UNIT_MOD2 and fl[130] & pkg.engine.FLAG_NOT_UNIT_MODP
        assert not fp[3].any() and not fp[130].any()         # (fq of a mod-2 non-unit is whatever Newton makes of zero: only fp is pinned)
        ok = fl == 0
        assert ok.sum() >= 20                                # (x^N - 1 has many factors for some of these N: units are not the rule)
        one = np.zeros(N, np.int64); one[0] = 1
        _, rem3 = orc.polymul_split_batch(N, 3, f.astype(np.int64) % 3, fp)
        tern = range(B)                                      # (rows 140..149 too: every Newton round takes an int8 f by its value)
        assert all(np.array_equal(rem3[i], one) for i in range(B) if not fl[i] & pkg.engine.FLAG_NOT_UNIT_MODP)
        _, rem = orc.polymul_split_batch(N, q, f.astype(np.int64) % q, fq.astype(np.int64) % q)
        assert all(np.array_equal(rem[i], one) for i in tern if ok[i])


def test_load_private_key_equals_reference_on_every_captured_f(eng):
    """loadPrivateKeyF through the host mirror on all 123 captured f (tests/golden/keygen_cases.json): the reference's fq
    and fp where it returns, its message where it throws -- including the non-units its `&&` checks accept, which the
    inversion kernels flag and the generic family then reproduces step by step."""
    with open(os.path.join(os.path.dirname(__file__), "golden", "keygen_cases.json")) as fh:
        cases = json.load(fh)["cases"]
    n_ok = n_err = 0
    for c in cases:
        n = pkg.NTRU(dict(N=c["N"], q=c["q"], p=c["p"]), engine=eng)
        if "error" in c:
            with pytest.raises(ValueError) as ei:
                n.loadPrivateKeyF(c["f"])
            assert str(ei.value) == c["error"] and n.f == c["f"]       # index.js:33 assigns f before anything can throw
            n_err += 1
        else:
            assert n.loadPrivateKeyF(c["f"]) is True
            assert n.fq == c["fq"] and n.fp == c["fp"], c["f"]
            n_ok += 1
    assert n_ok >= 60 and n_err >= 40


@pytest.mark.parametrize("B", [1, 2, 3, 6, 7, 8, 13, 29, 257])
def test_ragged_batch_sizes(eng, B):
    # N=17 packs 7 items per wavefront, N=167 two: batches that do not fill a wave / a workgroup
    for N, q, d in ((17, 32, 2), (167, 128, 18), (821, 4096, 273)):
        rng = np.random.default_rng(B * 31 + N)
        h = rng.integers(0, q, N)
        r = ternary_rows(rng, B, N, d, d)
        m = rng.integers(0, 2, (B, N))
        e, quot = eng.encrypt_batch(N, q, h, r, m)
        e_o, quot_o = orc.encrypt_batch(N, q, h, r, m)
        assert np.array_equal(e, e_o) and np.array_equal(quot, quot_o)


def test_empty_batch_is_a_noop(eng):
    e, quot = eng.encrypt_batch(17, 32, np.zeros(17), np.zeros((0, 17)), np.zeros((0, 17)))
    assert e.shape == (0, 17)


@pytest.mark.parametrize("N,mod", [(17, 32), (167, 128), (821, 4096), (701, 8192), (509, 65536), (1920, 2),
                                   (821, 3), (167, 3), (167, 7), (64, 5), (2, 3), (1000, 3)])
def test_polymul_split_equals_oracle(eng, N, mod):
    rng = np.random.default_rng(N + mod)
    B = 9 if N > 1000 else 41
    pow2 = mod & (mod - 1) == 0
    hi = 65536 if pow2 else mod                             # unreduced operands are legal for power-of-two moduli
    a = rng.integers(0, hi, (B, N)); b = rng.integers(0, hi, (B, N))
    a[0] = hi - 1; b[0] = hi - 1                            # worst-case magnitudes
    a[1] = 0
    b[2] = 0; b[2, 0] = 1                                   # times 1
    quot, rem = eng.polymul_split(N, mod, a, b)
    quot_o, rem_o = orc.polymul_split_batch(N, mod, a % mod, b % mod)
    assert np.array_equal(quot, quot_o) and np.array_equal(rem, rem_o)


def test_polymul_split_matrix_core_kernel_sweep(eng):
    """k_polymul_m (generic per-item product on the matrix cores, power-of-two moduli <= 8192): random (N, mod) with
    unreduced operands and worst-case magnitudes, against the oracle and against the vector-ALU kernel."""
    rng = np.random.default_rng(4242)
    cases = [(64, 2), (64, 8192), (128, 4096), (1024, 8192), (1023, 2048), (821, 4096), (701, 8192), (257, 4), (640, 1024)]
    cases += [(int(rng.integers(64, 1025)), 1 << int(rng.integers(1, 14))) for _ in range(8)]
    for N, mod in cases:
        B = int(rng.integers(1, 30))
        a = rng.integers(0, 65536, (B, N)); b = rng.integers(0, 65536, (B, N))
        a[0] = 65535; b[0] = 65535
        if B > 2:
            a[1] = mod - 1; b[1] = mod - 1; b[2] = 0; b[2, N - 1] = 1      # all (mod - 1); times x^(N-1)
        eng.set_kernel_path(4)
        quot, rem = eng.polymul_split(N, mod, a, b)
        assert eng.last_kernel() == "k_polymul_m", (N, mod, eng.last_kernel())
        eng.set_kernel_path(1)
        quot1, rem1 = eng.polymul_split(N, mod, a, b)
        assert eng.last_kernel() != "k_polymul_m"
        eng.set_kernel_path(0)
        quot_o, rem_o = orc.polymul_split_batch(N, mod, a % mod, b % mod)
        assert np.array_equal(quot, quot_o) and np.array_equal(rem, rem_o), (N, mod)
        assert np.array_equal(quot1, quot_o) and np.array_equal(rem1, rem_o), (N, mod, "vector-ALU kernel")


@pytest.mark.parametrize("N,q,d", [(17, 32, 2), (167, 128, 18), (509, 2048, 169), (821, 4096, 273), (701, 8192, 233)])
def test_verify_keys_batch_equals_oracle(eng, N, q, d, ):
    # synthetic per-item operands: outputs are fully defined, flags mostly "invalid"
    rng = np.random.default_rng(N)
    p, B = 3, 37
    f = ternary_rows(rng, B, N, d, max(d - 1, 0), two=-1)
    g = ternary_rows(rng, B, N, d, d, two=-1)
    fq = rng.integers(0, q, (B, N)); fp = rng.integers(0, p, (B, N)); h = rng.integers(0, q, (B, N))
    h[3, N // 2:] = 0                                       # short h: only indices below its trimmed length count
    h[4] = 0
    got = eng.verify_keys_batch(N, q, p, f, g, fq, fp, h)
    want = orc.verify_keys_batch(N, q, p, f, g, fq, fp, h)
    for k in want:
        assert np.array_equal(got[k], want[k]), k


def test_verify_keys_matrix_core_kernel_sweep(eng):
    """k_verify_keys_m (per-item products on the matrix cores): random (N, q) incl. N = 64 / multiples of 32 / 1024 and
    q from 2 to 8192, against the oracle and against the vector-ALU kernels."""
    rng = np.random.default_rng(2024)
    cases = [(64, 2), (64, 8192), (96, 64), (128, 4096), (1024, 8192), (1023, 2048), (821, 4096), (257, 4), (640, 1024)]
    cases += [(int(rng.integers(64, 1025)), 1 << int(rng.integers(1, 14))) for _ in range(10)]
    p = 3
    for N, q in cases:
        B = int(rng.integers(1, 40)); d = N // 3
        f = ternary_rows(rng, B, N, d, max(d - 1, 0), two=-1); g = ternary_rows(rng, B, N, d, d, two=-1)
        fq = rng.integers(0, q, (B, N)); fp = rng.integers(0, p, (B, N)); h = rng.integers(0, q, (B, N))
        if B > 2:
            h[1, N // 3:] = 0; h[2] = 0
            fq[0, :] = 0; fq[0, 0] = 1; f[0, :] = 0; f[0, 0] = 1            # fq * f = 1: no 'invalid fq' flag
        eng.set_kernel_path(4)
        got = eng.verify_keys_batch(N, q, p, f, g, fq, fp, h)
        assert eng.last_kernel() == "k_verify_keys_m", (N, q, eng.last_kernel())
        eng.set_kernel_path(1)
        alt = eng.verify_keys_batch(N, q, p, f, g, fq, fp, h)
        assert eng.last_kernel() != "k_verify_keys_m"
        eng.set_kernel_path(0)
        want = orc.verify_keys_batch(N, q, p, f, g, fq, fp, h)
        for k in want:
            assert np.array_equal(got[k], want[k]), (N, q, k)
            assert np.array_equal(alt[k], want[k]), (N, q, k, "vector-ALU kernel")
    # the automatic choice takes it from N = 128
    N, q, B = 509, 2048, 5
    f = ternary_rows(rng, B, N, 100, 99, two=-1); g = ternary_rows(rng, B, N, 100, 100, two=-1)
    eng.verify_keys_batch(N, q, p, f, g, rng.integers(0, q, (B, N)), rng.integers(0, p, (B, N)), rng.integers(0, q, (B, N)))
    assert eng.last_kernel() == "k_verify_keys_m"


def test_verify_keys_h_comparison_boundaries_and_unreduced_fp(eng):
    """index.js:165 compares h with the remainder below h's TRIMMED length: the kernel finds h's last non-zero coefficient and its
    first difference from the remainder (one ballot + one v_readlane each) -- exercised at the boundaries: h equal to the remainder,
    truncated at every kind of position (chunk and lane boundaries, 0, 1, N - 1), a single coefficient changed below / at / above
    the top, the zero polynomial.  fp arrives unreduced (bytes 0..255: the byte-wise mod 3 behind the wave-wide test)."""
    rng = np.random.default_rng(77)
    p = 3
    for N, q in ((821, 4096), (509, 2048), (64, 8192), (1024, 4096), (167, 128)):
        d = N // 3
        cuts = sorted({0, 1, 2, 15, 16, 17, 31, 32, 33, 255, 256, 257, N // 2, N - 17, N - 16, N - 2, N - 1, N} & set(range(N + 1)))
        B = 4 * len(cuts) + 2
        f = ternary_rows(rng, B, N, d, max(d - 1, 0), two=-1); g = ternary_rows(rng, B, N, d, d, two=-1)
        fq = rng.integers(0, q, (B, N)); fp = rng.integers(0, 256, (B, N))
        base = eng.verify_keys_batch(N, q, p, f, g, fq, fp % 3, np.zeros((B, N), np.int64))
        rem = base["rem_h"].astype(np.int64)
        h = rem.copy()
        for i, c in enumerate(cuts):
            h[4 * i, c:] = 0                                   # truncated at c: equal below its own length -> valid
            h[4 * i + 1, c:] = 0
            if c > 0: h[4 * i + 1, rng.integers(0, c)] ^= 1     # ... with one coefficient below the cut changed
            h[4 * i + 2, min(c, N - 1)] = (h[4 * i + 2, min(c, N - 1)] + 1) % q     # one coefficient changed, everything else equal
            h[4 * i + 3, c:] = 0
            if c < N: h[4 * i + 3, rng.integers(c, N)] = 1      # a lone non-zero coefficient above a matching prefix
        h[B - 1] = 0                                          # the zero polynomial: length 1, compares index 0
        got = eng.verify_keys_batch(N, q, p, f, g, fq, fp, h)
        want = orc.verify_keys_batch(N, q, p, f, g, fq, fp, h)
        for k in want:
            assert np.array_equal(got[k], want[k]), (N, q, k, np.nonzero(got[k] != want[k]))
        assert (want["flags"][0::4][1:len(cuts)] & 4 == 0).all()            # the truncated copies are valid h (cut 0 = the zero
                                                                             # polynomial, which still compares index 0)
        assert np.array_equal(got["rem_fp"], base["rem_fp"])                 # unreduced fp = reduced fp


@pytest.mark.parametrize("N,q,path,kernel", [(17, 32, 0, "k_verify_keys<1>"), (65, 2048, 0, "k_verify_keys_t<1,2>"),
                                             (193, 2048, 1, "k_verify_keys<3>"), (193, 2048, 2, "k_verify_keys_t<3,6>")])
def test_verify_keys_h_boundaries_valu_kernels(eng, N, q, path, kernel):
    """The construction of test_verify_keys_h_comparison_boundaries_and_unreduced_fp through the vector-ALU kernels, which share
    one set of flag helpers: N = 17 packs seven items into a wave (per-item lane mask, partial last group), N = 65 has one pair
    per lane, N = 193 three (a cut can fall inside a lane).  Cuts sit at 0, 1, 2, around a lane's 2K outputs, around N / 2 and
    the lane boundaries next to it, and at the top.  Every array byte for byte against the oracle."""
    rng = np.random.default_rng(1000 * N + path)
    p, K = 3, int(kernel.split("<")[1].split(",")[0].rstrip(">"))
    lane = N // 2 // (2 * K) * (2 * K)
    cuts = sorted({0, 1, 2, 2 * K - 1, 2 * K, 2 * K + 1, N // 2, lane, lane + 2 * K, N - 2, N - 1, N} & set(range(N + 1)))
    B = 4 * len(cuts) + 2
    d = N // 3
    f = ternary_rows(rng, B, N, d, max(d - 1, 0), two=-1); g = ternary_rows(rng, B, N, d, d, two=-1)
    fq = rng.integers(0, q, (B, N)); fp = rng.integers(0, 256, (B, N))
    h = orc.verify_keys_batch(N, q, p, f, g, fq, fp % 3, np.zeros((B, N), np.int64))["rem_h"].astype(np.int64)
    for i, c in enumerate(cuts):
        h[4 * i, c:] = 0                                   # truncated at c: equal below its own length -> valid
        h[4 * i + 1, c:] = 0
        if c > 0: h[4 * i + 1, rng.integers(0, c)] ^= 1     # ... with one coefficient below the cut changed
        h[4 * i + 2, min(c, N - 1)] = (h[4 * i + 2, min(c, N - 1)] + 1) % q     # one coefficient changed, everything else equal
        h[4 * i + 3, c:] = 0
        if c < N: h[4 * i + 3, rng.integers(c, N)] = 1      # a lone non-zero coefficient above a matching prefix
    h[B - 1] = 0                                          # the zero polynomial: length 1, compares index 0
    want = orc.verify_keys_batch(N, q, p, f, g, fq, fp, h)
    eng.set_kernel_path(path)
    try:
        got = eng.verify_keys_batch(N, q, p, f, g, fq, fp, h)
        assert eng.last_kernel() == kernel
    finally:
        eng.set_kernel_path(0)
    for k in want:
        assert np.array_equal(got[k], want[k]), (k, np.nonzero(got[k] != want[k]))
    assert (want["flags"][0::4][1:len(cuts)] & 4 == 0).all()            # the truncated copies are valid h


def test_verify_keys_device_pointers_at_any_alignment(eng):
    """ntru_verify_keys_batch_dev with every array at an odd byte offset (uint16 arrays stay 2-aligned): the matrix-core
    kernel reads rows through aligned chunks + shifts and must neither read garbage nor write outside its rows."""
    import torch
    dev = torch.device("cuda:0")
    rng = np.random.default_rng(77)
    N, q, p, B = 821, 4096, 3, 19
    f = ternary_rows(rng, B, N, 270, 269, two=-1); g = ternary_rows(rng, B, N, 270, 270, two=-1)
    fq = rng.integers(0, q, (B, N)); fp = rng.integers(0, p, (B, N)); h = rng.integers(0, q, (B, N))
    want = orc.verify_keys_batch(N, q, p, f, g, fq, fp, h)
    eng.set_stream(torch.cuda.current_stream().cuda_stream)
    try:
        for off in (1, 3, 6, 13):
            def place(a, dtype):
                raw = np.ascontiguousarray(a.astype(dtype)).view(np.uint8).ravel()
                o = off * np.dtype(dtype).itemsize
                buf = torch.full((raw.size + 64,), 0x7F, dtype=torch.uint8, device=dev)
                buf[o:o + raw.size] = torch.from_numpy(raw).to(dev)
                return buf, buf.data_ptr() + o
            def out(dtype, n):
                o = off * np.dtype(dtype).itemsize
                buf = torch.full((n * np.dtype(dtype).itemsize + 64,), 0xAB, dtype=torch.uint8, device=dev)
                return buf, buf.data_ptr() + o
            ins = [place(f, np.int8), place(g, np.int8), place(fq, np.uint16), place(fp, np.uint8), place(h, np.uint16)]
            spec = [("quot_fq", np.uint16), ("rem_fq", np.uint16), ("quot_fp", np.uint8), ("rem_fp", np.uint8),
                    ("quot_h", np.uint16), ("rem_h", np.uint16)]
            outs = [out(dt, B * N) for _, dt in spec]
            fl = out(np.uint8, B)
            eng.verify_keys_batch_dev(N, q, p, *[x[1] for x in ins], B, *[x[1] for x in outs], fl[1])
            torch.cuda.synchronize()
            assert eng.last_kernel() == "k_verify_keys_m"
            for (name, dt), (buf, _) in zip(spec, outs):
                a = buf.cpu().numpy(); o = off * np.dtype(dt).itemsize; n = B * N * np.dtype(dt).itemsize
                assert (a[:o] == 0xAB).all() and (a[o + n:] == 0xAB).all(), (off, name, "wrote outside")
                assert np.array_equal(a[o:o + n].view(dt).reshape(B, N), want[name]), (off, name)
            a = fl[0].cpu().numpy()
            assert np.array_equal(a[off:off + B], want["flags"]) and (a[:off] == 0xAB).all() and (a[off + B:] == 0xAB).all()
    finally:
        eng.set_stream(None)


def test_verify_keys_true_keys_and_corruptions(eng, scheme_golden):
    opts = scheme_golden["options"]
    N, q, p = opts["N"], opts["q"], opts["p"]
    key = scheme_golden["keys"][0]
    pad = lambda a, dt: np.array(list(a) + [0] * (N - len(a)), dtype=dt)
    k = dict(f=pad(key["f"], np.int8), g=pad(key["g"], np.int8), fq=pad(key["fq"], np.uint16),
             fp=pad(key["fp"], np.uint8), h=pad(key["h"], np.uint16))
    rows = {name: np.stack([v] * 6) for name, v in k.items()}
    rows["fq"][1, 0] ^= 1; rows["fq"][1, 1] ^= 1
    rows["fp"][2, 0] = (rows["fp"][2, 0] + 1) % p; rows["fp"][2, 2] = (rows["fp"][2, 2] + 1) % p
    rows["h"][3, 0] ^= 1
    rows["g"][4] = np.roll(rows["g"][4], 1)
    rows["f"][5] = np.roll(rows["f"][5], 3)
    got = eng.verify_keys_batch(N, q, p, rows["f"], rows["g"], rows["fq"], rows["fp"], rows["h"])
    want = orc.verify_keys_batch(N, q, p, rows["f"], rows["g"], rows["fq"], rows["fp"], rows["h"])
    for name in want:
        assert np.array_equal(got[name], want[name]), name
    assert got["flags"][0] == 0 and got["flags"][3] == 4 and got["flags"][4] & 4


def test_split_and_add_kernels(eng):
    rng = np.random.default_rng(5)
    for N, mod in ((17, 32), (821, 4096), (821, 3), (701, 8192), (5, 7)):
        B = 23
        a = rng.integers(0, mod, (B, 2 * N)); a[:, 2 * N - 1] = 0
        a[0, N:] = 0
        quot, rem = eng.split_by_I(N, mod, a)
        assert np.array_equal(quot, (mod - a[:, N:]) % mod) and np.array_equal(rem, (a[:, :N] + a[:, N:]) % mod)
        for row in (1, 2):   # and against the reference-equivalent long division
            ref = orc.divide(a[row].tolist(), [1] + [0] * (N - 1) + [-1], mod)
            assert orc.trim(quot[row, :N - 1]) == ref["quotient"] and orc.trim(rem[row]) == ref["remainder"]
        x = rng.integers(0, mod, (B, N)); y = rng.integers(0, mod, (B, N))
        assert np.array_equal(eng.add_batch(N, mod, x, y), (x + y) % mod)


@pytest.mark.parametrize("N,n1,n2", [(821, 273, 273), (701, 233, 233), (509, 169, 169), (167, 18, 18), (17, 2, 2),
                                     (17, 17, 0), (5, 0, 0), (2, 1, 1), (1000, 1, 998)])
@pytest.mark.parametrize("rounds", [20, 12, 8])
def test_device_sampler_equals_oracle(eng, N, n1, n2, rounds):
    """generateCustomArray on the device: same Fisher-Yates procedure on the same draw stream -- ChaCha20 (RFC 8439, the default) or
    the reduced-round variants ntru_engine_set_sampler_rounds offers (12, 8): the oracle replays whichever the caller asked for."""
    key = (np.arange(8, dtype=np.uint64) * 0x9E3779B9 + 12345).astype(np.uint32)
    assert eng.sampler_rounds() == 20                               # the default is RFC 8439's
    eng.set_sampler_rounds(rounds)
    try:
        assert eng.sampler_rounds() == rounds
        for first, B in ((0, 1), (7, 64), (2 ** 33 + 5, 65), (123456, 200)):
            got = eng.sample_ternary(N, n1, n2, 2, key, first, B)
            want = orc.sample_ternary_batch(N, n1, n2, 2, key, first, B, rounds=rounds)
            assert np.array_equal(got, want), (first, B)
            assert ((got == 1).sum(axis=1) == n1).all() and ((got == 2).sum(axis=1) == n2).all()
            if rounds != 20 and N > 2 and n1 + n2 not in (0, N) and B > 1:    # and it is NOT the 20-round stream
                assert not np.array_equal(got, orc.sample_ternary_batch(N, n1, n2, 2, key, first, B))
        with pytest.raises(pkg.EngineError, match="cannot exceed the array length"):
            eng.sample_ternary(4, 3, 2, 2, key, 0, 1)
        with pytest.raises(pkg.EngineError, match="sampler rounds must be"):
            eng.set_sampler_rounds(10)
    finally:
        eng.set_sampler_rounds(20)


@pytest.mark.parametrize("N", [16, 17, 31, 33, 100, 821, 2046, 2047, 2100])
def test_device_sampler_output_paths(eng, N):
    """The sampler's two output paths (aligned 16-byte pieces over a whole block of 64 rows; one byte per lane for unaligned pointers and
    the partial last block), `other` != 2, and both reciprocal sources (constant table below N = 2047, LDS table from there on)."""
    import torch
    key = (np.arange(8, dtype=np.uint64) * 0x85EBCA6B + 99).astype(np.uint32)
    n1, n2, B = N // 3, N // 4, 130                                  # two whole blocks and two rows
    for other, off, first in ((2, 0, 0), (255, 0, 5), (7, 3, 2 ** 32 - 64), (2, 16, 11)):
        buf = torch.full((B * N + 64,), 0xEE, dtype=torch.uint8, device="cuda:0")
        eng.sample_ternary_dev(N, n1, n2, other, key, first, B, buf.data_ptr() + off)
        torch.cuda.synchronize()
        got = buf.cpu().numpy()
        want = orc.sample_ternary_batch(N, n1, n2, other, key, first, B)
        assert np.array_equal(got[off:off + B * N].reshape(B, N), want), (other, off)
        assert (got[:off] == 0xEE).all() and (got[off + B * N:] == 0xEE).all()          # nothing outside the rows


def test_sampled_encrypt_matches_reference_semantics(eng, scheme_golden):
    """sample r on the device, encrypt, and replay on the CPU: r from the oracle's sampler on the same stream, then the
    oracle's encryptBits -- the witness must match bit for bit."""
    opts = scheme_golden["options"]
    N, q, d = opts["N"], opts["q"], opts["dr"]
    key = np.array([1, 2, 3, 4, 5, 6, 7, 8], np.uint32) * 0x01000193
    h = np.array(list(scheme_golden["keys"][0]["h"]) + [0] * (N - len(scheme_golden["keys"][0]["h"])))
    B = 33
    m = np.random.default_rng(N).integers(0, 2, (B, N))
    r = eng.sample_ternary(N, d, d, 2, key, 1000, B)
    e, quot = eng.encrypt_batch(N, q, h, r, m)
    r_o = orc.sample_ternary_batch(N, d, d, 2, key, 1000, B)
    e_o, quot_o = orc.encrypt_batch(N, q, h, r_o, m)
    assert np.array_equal(r, r_o) and np.array_equal(e, e_o) and np.array_equal(quot, quot_o)


def test_field_packing_equals_reference_and_oracle(eng):
    from conftest import load_golden
    g = load_golden("pack_functions.json")
    for v in g["packOutput"]:
        got = pkg.packOutput(v["maxVal"], v["dataLen"], v["data"], engine=eng)
        want = {k: v[k] for k in ("maxInputBits", "maxOutputBits", "outputSize", "arrLen")}
        want["expected"] = [int(x, 16) for x in v["expected"]]
        assert got == want
    for v in g["unpackInput"]:
        got = pkg.unpackInput(v["maxVal"], v["packedBits"], [int(x, 16) for x in v["data"]], engine=eng)
        assert got == {k: v[k] for k in ("maxInputBits", "packedBits", "packedSize", "unpackedSize", "unpacked")}
    rng = np.random.default_rng(8)
    for max_val, n in ((8192, 701), (4096, 821), (3, 821), (65535, 100), (1, 9)):
        data = rng.integers(0, min(max_val + 1, 65536), (57, n))
        limbs = eng.pack_batch(max_val, n, data)
        assert np.array_equal(limbs, orc.pack_batch(max_val, n, data))
        pr = eng.pack_params(max_val, n)
        back = eng.unpack_batch(max_val, pr["numInputsPerOutput"] * pr["maxInputBits"], limbs)
        assert np.array_equal(back[:, :n], data) and not back[:, n:].any()          # pack -> unpack round trip
        assert np.array_equal(back, orc.unpack_batch(max_val, pr["numInputsPerOutput"] * pr["maxInputBits"], limbs))


# ---- error behaviour ------------------------------------------------------------------------------------------

def test_error_behaviour(eng):
    z = np.zeros((1, 17))
    with pytest.raises(pkg.EngineError) as ei:
        eng.encrypt_batch(17, 48, np.zeros(17), z, z)               # q must be a power of two
    assert ei.value.code == 3
    with pytest.raises(pkg.EngineError):
        eng.decrypt_batch(17, 32, 4, np.zeros(17), np.zeros(17), z)  # p must not be a power of two
    with pytest.raises(pkg.EngineError):
        eng.polymul_split(2000, 2048, np.zeros((1, 2000)), np.zeros((1, 2000)))
    n = pkg.NTRU({"N": 17, "q": 32, "dr": 2, "h": [1] * 17}, engine=eng)
    with pytest.raises(ValueError, match="Invalid array length"):       # expandArray overflow, index.js:535
        n.encryptBits([1] * 18)
    with pytest.raises(TypeError):                                      # this.f is null, index.js:112
        n.decryptBits([1, 2, 3])
    for missing, msg in (("f", "missing private key F"), ("fq", "missing private key Fq"),
                         ("fp", "missing private key Fp"), ("g", "missing private key G"),
                         ("h", "missing public key H")):
        full = dict(N=17, q=32, f=[1] * 17, fq=[1], fp=[1], g=[1] * 17, h=[1])
        full[missing] = None
        with pytest.raises(ValueError, match=msg):
            pkg.NTRU(full, engine=eng).verifyKeysInputs()
    with pytest.raises(ValueError, match="invalid h"):
        pkg.NTRU(dict(N=17, q=32, f=[1] + [0] * 16, fq=[1], fp=[1], g=[1] + [0] * 16, h=[5]), engine=eng).verifyKeysInputs()


# ---- BASELINE.json sizes: device-resident buffers, size-independent properties ----------------------------------

def _golden_key(name):
    with open(os.path.join(ge.ROOT, "tests", "golden", "scheme_%s.json" % name)) as fh:
        g = json.load(fh)
    return g["options"], g["keys"][0]


@pytest.mark.parametrize("profile,logB", [("n821_q4096", 20), ("n509_q2048", 20), ("n701_q8192", 18)])
def test_full_size_batch_properties(eng, profile, logB):
    import torch
    opts, key = _golden_key(profile)
    N, q, p, d = opts["N"], opts["q"], opts["p"], opts["dr"]
    B = 1 << logB
    dev = torch.device("cuda:0")
    gen = torch.Generator(device=dev); gen.manual_seed(1234)
    pad = lambda a: list(a) + [0] * (N - len(a))
    h = torch.tensor(pad(key["h"]), dtype=torch.int32, device=dev).to(torch.int16)   # 16-bit patterns; q <= 2^15 here
    f = torch.tensor(pad(key["f"]), dtype=torch.int8, device=dev)
    fp = torch.tensor(pad(key["fp"]), dtype=torch.uint8, device=dev)
    r = torch.zeros((B, N), dtype=torch.uint8, device=dev)
    chunk = 1 << 16
    for o in range(0, B, chunk):
        idx = torch.rand((chunk, N), device=dev, generator=gen).argsort(dim=1)
        r[o:o + chunk].scatter_(1, idx[:, :d], 1)
        r[o:o + chunk].scatter_(1, idx[:, d:2 * d], 2)
    m1 = torch.randint(0, 2, (B, N), dtype=torch.uint8, device=dev, generator=gen)
    m2 = torch.randint(0, 3, (B, N), dtype=torch.uint8, device=dev, generator=gen)
    new16 = lambda: torch.empty((B, N), dtype=torch.int16, device=dev)    # raw u16 patterns
    u = lambda t: t.to(torch.int32) & 0xFFFF                                 # widen as unsigned
    new8 = lambda: torch.empty((B, N), dtype=torch.uint8, device=dev)
    e1, qe1, e2, e3 = new16(), new16(), new16(), new16()
    eng.set_stream(torch.cuda.current_stream().cuda_stream)
    try:
        eng.encrypt_batch_dev(N, q, h.data_ptr(), r.data_ptr(), m1.data_ptr(), B, e1.data_ptr(), qe1.data_ptr())
        eng.encrypt_batch_dev(N, q, h.data_ptr(), r.data_ptr(), m2.data_ptr(), B, e2.data_ptr(), None)
        torch.cuda.synchronize()
        # sanity of the synthetic r: d ones and d twos in every row
        assert int((r == 1).sum()) == B * d and int((r == 2).sum()) == B * d
        # linearity in m for a fixed r: e(m1) - e(m2) = m1 - m2 (mod q), on the whole batch
        lhs = (u(e1) - u(e2)) % q
        rhs = (m1.to(torch.int32) - m2.to(torch.int32)) % q
        assert torch.equal(lhs, rhs)
        # quotient/remainder identity of the circuit (ntru.circom:155-186) folded at x = 1:
        #   sum(m) + sum(r)*sum(h) = sum(rem) + (1 - 1)*sum(quot)  (mod q)
        s = lambda t: t.to(torch.int64).sum(dim=1)
        assert torch.equal((s(m1) + s(r) * int(u(h).sum())) % q, s(u(e1)) % q)
        # witness mode and value-only mode agree; decrypt of the whole batch
        val, q1, r1, q2, val2 = new8(), new16(), new16(), new8(), new8()
        eng.decrypt_batch_dev(N, q, p, f.data_ptr(), fp.data_ptr(), e1.data_ptr(), B, val.data_ptr(), q1.data_ptr(),
                              r1.data_ptr(), q2.data_ptr())
        eng.decrypt_batch_dev(N, q, p, f.data_ptr(), fp.data_ptr(), e1.data_ptr(), B, val2.data_ptr())
        torch.cuda.synchronize()
        assert torch.equal(val, val2)
        assert int(val.max()) <= 2 and int(q2.max()) <= 2 and int(u(r1).max()) < q and int(u(q1).max()) < q
        if q % 3 == 2:   # the reference's lift only round-trips for q = 2 mod 3
            assert torch.equal(val, m1)
        # a strided sample of 4097 rows, all outputs, against the oracle (incl. the last row)
        rows = torch.tensor(sorted(set(list(range(0, B, B // 4096)) + [B - 1])), device=dev)
        host = lambda t: (lambda a: a.view(np.uint16) if a.dtype == np.int16 else a)(t[rows].cpu().numpy())
        e_o, qe_o = orc.encrypt_batch(N, q, h.cpu().numpy().view(np.uint16), host(r), host(m1))
        assert np.array_equal(host(e1), e_o) and np.array_equal(host(qe1), qe_o)
        v_o, q1_o, r1_o, q2_o = orc.decrypt_batch(N, q, p, f.cpu().numpy(), fp.cpu().numpy(), e_o)
        assert np.array_equal(host(val), v_o) and np.array_equal(host(q1), q1_o)
        assert np.array_equal(host(r1), r1_o) and np.array_equal(host(q2), q2_o)
        # homomorphic add on device: e1 + e2 decrypts like the oracle says
        eng.add_batch_dev(N, q, e1.data_ptr(), e2.data_ptr(), B, e3.data_ptr())
        torch.cuda.synchronize()
        assert torch.equal(u(e3), (u(e1) + u(e2)) % q)
    finally:
        eng.set_stream(None)


@pytest.mark.parametrize("pinned", [False, True])
def test_host_pipeline_many_chunks_equal_oracle(eng, pinned):
    """The host-pointer entry points (ntru_host.hip) cut a batch into chunks that rotate through three buffer sets (pinned
    arena, device arena): 150 001 items = five chunks, ragged last one, with pageable numpy arrays (staged through the pinned
    arenas) and with arrays from ntru_host_alloc (DMA'd in place); every output array against the oracle.  Then a smaller and a
    larger batch through the same engine: the arenas only grow and are reused."""
    N, q, p, d = 167, 128, 3, 18
    rng = np.random.default_rng(4242)
    h = rng.integers(0, q, N); fp = rng.integers(0, p, N)
    f = ternary_rows(rng, 1, N, 61, 60, two=-1)[0]
    for B in (150001, 7, 70000):
        base = np.zeros(N, np.uint8); base[:d] = 1; base[d:2 * d] = 2
        r_src = rng.permuted(np.tile(base, (B, 1)), axis=1)
        m_src = rng.integers(0, 3, (B, N)).astype(np.uint8)
        if pinned:
            r = eng.pinned_empty((B, N), np.uint8); r[:] = r_src
            m = eng.pinned_empty((B, N), np.uint8); m[:] = m_src
        else:
            r, m = r_src, m_src
        e, quot = eng.encrypt_batch(N, q, h, r, m)
        e_o, quot_o = orc.encrypt_batch(N, q, h, r_src, m_src)
        assert np.array_equal(e, e_o) and np.array_equal(quot, quot_o), (B, pinned)
        if pinned:
            ein = eng.pinned_empty((B, N), np.uint16); ein[:] = e_o
        else:
            ein = e_o
        got = eng.decrypt_batch(N, q, p, f, fp, ein)
        want = orc.decrypt_batch(N, q, p, f, fp, e_o)
        for g_, w_, name in zip(got, want, ("value", "quotient1", "remainder1", "quotient2")):
            assert np.array_equal(g_, w_), (B, pinned, name)
        v_only = eng.decrypt_batch(N, q, p, f, fp, ein, want_witness=False)
        assert np.array_equal(v_only[0], want[0])
    # per-item entry points through the same pipeline (several chunks as well)
    B = 9000
    a = rng.integers(0, q, (B, N)); b = rng.integers(0, q, (B, N))
    quot, rem = eng.polymul_split(N, q, a, b)
    qo, ro = orc.polymul_split_batch(N, q, a, b)
    assert np.array_equal(quot, qo) and np.array_equal(rem, ro)
    key = np.arange(8, dtype=np.uint32) + 3
    s = eng.sample_ternary(N, d, d, 2, key, 10, B)
    assert np.array_equal(s[B - 1], orc.sample_ternary_batch(N, d, d, 2, key, 10 + B - 1, 1)[0])      # first_item advances per chunk
    assert np.array_equal(s[0], orc.sample_ternary_batch(N, d, d, 2, key, 10, 1)[0])


def test_generic_family_random_differential(eng):
    """300 random (lengths, modulus, signed / unreduced coefficients) per operation against the Python restatement: long
    division, the Euclidean algorithm and polyInv with every status the reference can raise; moduli prime, composite, powers
    of two, 1; operands shorter and longer than each other, zero polynomials, trailing zeros."""
    from oracle import ntru_keygen as kg
    rng = np.random.default_rng(777)
    mods = [1, 2, 3, 4, 5, 7, 8, 9, 11, 12, 15, 16, 31, 32, 64, 97, 128, 255, 256, 1000, 4096, 65537, 1 << 20, (1 << 26)]
    seen = set()
    for trial in range(300):
        p = int(rng.choice(mods))
        la, lb = int(rng.integers(0, 24)), int(rng.integers(1, 24))
        span = min(int(rng.choice([1, 2, p, 3 * p])), 1 << 26)     # the family's documented operand bound
        a = rng.integers(-span, span + 1, la)
        b = rng.integers(-span if trial % 3 == 0 else 0, span + 1, lb)
        if trial % 7 == 0:
            b[lb // 2:] = 0                                  # degree below the length; sometimes the zero polynomial
        if trial % 11 == 0 and la:
            a[la // 2:] = 0
        quot, rem, st = eng.generic_divide(a, b, p)
        try:
            qo, ro = kg._divide(a, b, p)
            assert st[0] == 0 and quot[0] == qo.tolist() and rem[0] == ro.tolist(), (trial, p, a, b)
        except ZeroDivisionError:
            assert st[0] == 1, (trial, p, a, b)
        except ArithmeticError:
            assert st[0] == 2, (trial, p, a, b)
        seen.add(int(st[0]))
        gcd, inv, st2 = eng.generic_eea(a, b, p)
        try:
            go, io = kg.extended_euclid(a, b, p, True)
            assert st2[0] == 0 and gcd[0] == go.tolist() and inv[0] == io.tolist(), (trial, p, a, b)
        except kg.InvalidGcd:
            assert st2[0] == 3, (trial, p, a, b)
        except ZeroDivisionError:
            assert st2[0] == 1
        except ArithmeticError:
            assert st2[0] == 2, (trial, p, a, b)
        seen.add(10 + int(st2[0]))
        if lb >= 3 and p <= 4096:
            I = np.zeros(lb, np.int64); I[0] = 1; I[-1] = -1
            f = rng.integers(-1, 2, min(la, lb - 1))
            got, st3 = eng.generic_poly_inv(f, I, p)
            try:
                want = kg.poly_inv_generic(f, I, p).tolist()
                assert st3[0] == 0 and got[0] == want, (trial, p, f)
            except kg.InvalidGcd:
                assert st3[0] == 3, (trial, p, f)
            except ZeroDivisionError:
                assert st3[0] == 1
            except ArithmeticError:
                assert st3[0] == 2, (trial, p, f)
        prod = eng.generic_multiply(a, b, p)
        assert prod[0] == kg._multiply(a, b, p).tolist()
    assert {0, 1, 2, 10, 12, 13} <= seen                     # every status was exercised


def test_multi_device_host_api_shards_equal_oracle():
    """ntru_multi_* (several devices in one process, contiguous shards, one host thread per engine).  The box has one GPU, so
    the device list names it three times: three engines, three threads, three shards of unequal size -- the sharding,
    threading and error plumbing are what is under test; results against the oracle."""
    me = pkg.MultiEngine([0, 0, 0])
    assert me.engines() == 3
    N, q, p, d = 167, 128, 3, 18
    rng = np.random.default_rng(31)
    B = 10001                                               # 3334 + 3334 + 3333
    h = rng.integers(0, q, N); fp = rng.integers(0, p, N)
    f = ternary_rows(rng, 1, N, 61, 60, two=-1)[0]
    base = np.zeros(N, np.uint8); base[:d] = 1; base[d:2 * d] = 2
    r = rng.permuted(np.tile(base, (B, 1)), axis=1)
    m = rng.integers(0, 3, (B, N)).astype(np.uint8)
    e, quot = me.encrypt_batch(N, q, h, r, m)
    e_o, quot_o = orc.encrypt_batch(N, q, h, r, m)
    assert np.array_equal(e, e_o) and np.array_equal(quot, quot_o)
    got = me.decrypt_batch(N, q, p, f, fp, e)
    want = orc.decrypt_batch(N, q, p, f, fp, e_o)
    for g_, w_, name in zip(got, want, ("value", "quotient1", "remainder1", "quotient2")):
        assert np.array_equal(g_, w_), name
    Bk = 50
    kf = ternary_rows(rng, Bk, N, 61, 60, two=-1); kg_ = ternary_rows(rng, Bk, N, 20, 20, two=-1)
    kfq = rng.integers(0, q, (Bk, N)); kfp = rng.integers(0, p, (Bk, N)); kh = rng.integers(0, q, (Bk, N))
    outv = me.verify_keys_batch(N, q, p, kf, kg_, kfq, kfp, kh)
    wantv = orc.verify_keys_batch(N, q, p, kf, kg_, kfq, kfp, kh)
    for k in wantv:
        assert np.array_equal(outv[k], wantv[k]), k
    kfq2, kfp2, fl = me.invert_key_batch(N, q, p, kf)                          # inverses: f fq = 1 mod q, f fp = 1 mod 3
    ok = fl == 0
    assert ok.any()
    one = np.zeros(N, np.int64); one[0] = 1
    _, rq = orc.polymul_split_batch(N, q, kf % q, kfq2)
    _, r3 = orc.polymul_split_batch(N, 3, kf % 3, kfp2)
    assert all(np.array_equal(rq[i], one) and np.array_equal(r3[i], one) for i in range(Bk) if ok[i])
    assert np.array_equal(me.public_key_batch(N, q, p, kfq, kg_), orc.public_key_batch(N, q, p, kfq, kg_))
    pq, pr = me.polymul_split(N, q, kfq, kh)
    pq_o, pr_o = orc.polymul_split_batch(N, q, kfq, kh)
    assert np.array_equal(pq, pq_o) and np.array_equal(pr, pr_o)
    assert me.encrypt_batch(N, q, h, r[:2], m[:2])[0].shape == (2, N)          # fewer items than engines: empty shards
    with pytest.raises(pkg.EngineError, match="device shard 0"):
        me.encrypt_batch(N, 12, h, r[:5], m[:5])                               # q = 12: refused, the message names the shard
    me.close()
    with pytest.raises(pkg.EngineError):
        pkg.MultiEngine([0, 99])                                               # no such device




@pytest.mark.parametrize("N,q,d,B", [(167, 128, 18, 9001), (821, 4096, 273, 300), (509, 2048, 169, 1)])
def test_pipeline_batch_equals_oracle_stage_by_stage(eng, N, q, d, B):
    """ntru_pipeline_batch (sampler -> encryptBits -> decryptBits -> packOutput, device-resident between the stages, chunked through
    the three-stage host pipeline) against the oracle's replay of every stage; every combination of optional outputs."""
    rng = np.random.default_rng(N + B)
    p = 3
    h = rng.integers(0, q, N); fp = rng.integers(0, p, N)
    f = ternary_rows(rng, 1, N, d, d - 1, two=-1)[0]
    m = rng.integers(0, 2, (B, N))
    key = rng.integers(0, 2 ** 32, 8, dtype=np.uint64).astype(np.uint32)
    first = (1 << 33) + 12345
    r_o = orc.sample_ternary_batch(N, d, d, p - 1, key, first, B)
    e_o, _ = orc.encrypt_batch(N, q, h, r_o, m)
    v_o = orc.decrypt_batch(N, q, p, f, fp, e_o)[0]
    out = eng.pipeline_batch(N, q, p, h, m, f=f, fp=fp, key=key, first_item=first, n1=d, n2=d,
                             want_r=True, want_e=True, want_value=True, want_packed=True)
    assert np.array_equal(out["r"], r_o) and np.array_equal(out["e"], e_o) and np.array_equal(out["value"], v_o)
    assert np.array_equal(out["packed"], orc.pack_batch(p - 1, N, v_o.astype(np.uint16)))
    lean = eng.pipeline_batch(N, q, p, h, m, f=f, fp=fp, key=key, first_item=first, n1=d, n2=d, want_value=True)
    assert list(lean) == ["value"] and np.array_equal(lean["value"], v_o)
    enc = eng.pipeline_batch(N, q, p, h, m, r=r_o, want_packed=True)                       # encrypt only, r given, packed ciphertext
    assert list(enc) == ["packed"] and np.array_equal(enc["packed"], orc.pack_batch(q - 1, N, e_o))
    assert (eng.last_kernel() == "k_encrypt_wp") == (q in (2048, 4096, 8192))               # fused where the row-image kernel applies
    for bad in (dict(key=key, r=r_o, want_e=True), dict(want_e=True), dict(key=key, want_value=True), dict(key=key)):
        with pytest.raises(pkg.EngineError):
            eng.pipeline_batch(N, q, p, h, m, n1=d, n2=d, **bad)


def test_plain_device_buffers_round_trip_and_feed_the_dev_entry_points(eng):
    N, q, p, B, d = 167, 128, 3, 77, 18
    rng = np.random.default_rng(5)
    h = rng.integers(0, q, N).astype(np.uint16); r = ternary_rows(rng, B, N, d, d).astype(np.uint8); m = rng.integers(0, 2, (B, N)).astype(np.uint8)
    dh, dr, dm, de = eng.dev_alloc(2 * N), eng.dev_alloc(B * N), eng.dev_alloc(B * N), eng.dev_alloc(2 * B * N)
    try:
        eng.dev_upload(dh, h); eng.dev_upload(dr, r); eng.dev_upload(dm, m)
        assert np.array_equal(eng.dev_download(dr, (B, N), np.uint8), r)
        eng.encrypt_batch_dev(N, q, dh, dr, dm, B, de)
        e = eng.dev_download(de, (B, N), np.uint16)                     # waits for the engine's stream
        assert np.array_equal(e, orc.encrypt_batch(N, q, h, r, m)[0])
        dp = eng.dev_alloc(B * eng.pack_params(2, N)["outputSize"] * 32)
        eng.pack_bytes_batch_dev(2, N, dr, B, dp)
        got = eng.dev_download(dp, (B, eng.pack_params(2, N)["outputSize"], 4), np.uint64)
        assert np.array_equal(got, orc.pack_batch(2, N, r.astype(np.uint16)))
        eng.dev_free(dp)
    finally:
        for x in (dh, dr, dm, de):
            eng.dev_free(x)


def test_python_mirror_pipeline_equals_oracle(eng):
    """ntru.NTRU.pipeline (the Python twin of the shim's ntru.pipeline) on a golden key."""
    from conftest import load_golden
    g = load_golden("scheme_n167_q128.json"); k = g["keys"][0]
    n = pkg.NTRU(dict(g["options"], f=k["f"], fp=k["fp"], fq=k["fq"], g=k["g"], h=k["h"]), engine=eng)
    N = n.N
    m = np.random.default_rng(1).integers(0, 2, (500, N))
    key = np.arange(8, dtype=np.uint32)
    pad = lambda a, dt: np.array(list(a) + [0] * (N - len(a)), dtype=dt)
    r_o = orc.sample_ternary_batch(N, n.dr, n.dr, n.p - 1, key, 7, 500)
    e_o, _ = orc.encrypt_batch(N, n.q, pad(n.h, np.uint16), r_o, m)
    v_o = orc.decrypt_batch(N, n.q, n.p, pad(n.f, np.int8), pad(n.fp, np.uint8), e_o)[0]
    out = n.pipeline(m, sampleR=(key, 7), decrypt=True, want={"r", "e", "value"})
    assert np.array_equal(out["r"], r_o) and np.array_equal(out["e"], e_o) and np.array_equal(out["value"], v_o)
    assert list(n.pipeline(m, r=r_o)) == ["e"]
    packed = n.pipeline(m, r=r_o, decrypt=True, pack=True)
    assert list(packed) == ["packed"] and np.array_equal(packed["packed"], orc.pack_batch(n.p - 1, N, v_o.astype(np.uint16)))


def test_generic_family_waits_for_the_scratch_buffers_previous_stream(eng):
    """The engine's temporaries are ONE buffer shared by every *_dev call that needs them.  Key inversion enqueued on stream A
    (Newton rounds: milliseconds of work that reads and writes the buffer), then ntru_engine_set_stream(B) and a generic product
    whose staging copies land in the same bytes: stream B has to wait for A's use (ntru_scratch_acquire / _release in
    run_generic), or the inverses come out wrong."""
    import torch
    N, q, p, B = 821, 4096, 3, 1 << 14
    dev = torch.device("cuda:0")
    g = torch.Generator(device=dev); g.manual_seed(77)
    f = torch.zeros((B, N), dtype=torch.int8, device=dev)
    idx = torch.rand((B, N), device=dev, generator=g).argsort(dim=1)
    f.scatter_(1, idx[:, :274], 1)
    f.scatter_(1, idx[:, 274:547], -1)
    fq = torch.empty((B, N), dtype=torch.int16, device=dev); fq2 = torch.empty_like(fq)
    flags = torch.empty(B, dtype=torch.uint8, device=dev); flags2 = torch.empty_like(flags)
    rng = np.random.default_rng(5)
    ga, gb = rng.integers(-1000, 1000, (4096, 64)), rng.integers(-1000, 1000, (4096, 64))
    sa, sb = torch.cuda.Stream(), torch.cuda.Stream()
    try:
        eng.set_stream(sa.cuda_stream)
        eng.invert_key_batch_dev(N, q, p, f.data_ptr(), B, fq2.data_ptr(), None, flags2.data_ptr())   # reference run, alone
        torch.cuda.synchronize()
        want = eng.generic_multiply(ga, gb, 1 << 20)
        torch.cuda.synchronize()
        eng.set_stream(sa.cuda_stream)
        eng.invert_key_batch_dev(N, q, p, f.data_ptr(), B, fq.data_ptr(), None, flags.data_ptr())     # in flight on A ...
        eng.set_stream(sb.cuda_stream)
        got = eng.generic_multiply(ga, gb, 1 << 20)                                                    # ... while B wants the buffer
        torch.cuda.synchronize()
        assert torch.equal(fq, fq2) and torch.equal(flags, flags2)
        assert got == want
        a0, b0 = [int(x) for x in ga[0]], [int(x) for x in gb[0]]
        ref = [0] * 127
        for i, x in enumerate(a0):
            for j, y in enumerate(b0):
                ref[i + j] = (ref[i + j] + x * y) % (1 << 20)
        while len(ref) > 1 and ref[-1] == 0:
            ref.pop()
        assert got[0] == ref
    finally:
        eng.set_stream(None)


@pytest.mark.parametrize("N,q", [(821, 4096), (701, 8192), (509, 2048), (1021, 4096), (64, 2048), (821, 1024), (1100, 4096)])
def test_encrypt_with_fused_pack_output_equals_oracle(eng, N, q):
    """ntru_encrypt_pack_batch_dev: encryptBits + packOutput(q - 1, N, e) (index.js:87-110, :572-596) in ONE kernel (k_encrypt_wp: the
    row block's raw image drained as field elements) when e itself is not asked for and q is 2048 / 4096 / 8192; the two-launch form
    with e as the intermediate otherwise; 11-, 12- and 13-bit fields, a row's last element of 1 .. per fields, ragged batches, several
    row blocks per workgroup; against the oracle's encrypt + pack.  Outside the fused range without e: NTRU_ERR_ARG."""
    import torch
    p = 3
    dev = torch.device("cuda:0")
    rng = np.random.default_rng(N * 7 + q)
    h = rng.integers(0, q, N).astype(np.uint16)
    th = torch.from_numpy(h.view(np.int16)).to(dev)
    can_fuse = q in (2048, 4096, 8192) and N <= 1024         # ... and the row block's image fits the LDS (N <= ~890)
    must_fuse = can_fuse and N <= 850
    fused = refused = 0
    for B in (1, 33, 777, 2 * 32 * 256 + 5):
        r = ternary_rows(rng, B, N, N // 3, N // 3, two=p - 1).astype(np.uint8)
        m = rng.integers(0, 2, (B, N)).astype(np.uint8)
        tr, tm = torch.from_numpy(r).to(dev), torch.from_numpy(m).to(dev)
        e_o = orc.encrypt_batch(N, q, h, r, m, want_quot=False)[0]
        want = orc.pack_batch(q - 1, N, e_o).view(np.uint64)
        for with_e in (True, False):
            packed = torch.full(want.shape, -1, dtype=torch.int64, device=dev)
            te = torch.full((B, N), 9, dtype=torch.int16, device=dev)
            try:
                eng.encrypt_pack_batch_dev(N, q, th.data_ptr(), tr.data_ptr(), tm.data_ptr(), B, te.data_ptr() if with_e else None, packed.data_ptr())
            except pkg.engine.EngineError:
                assert not with_e and not must_fuse         # outside the fused kernel's range e is needed as the intermediate
                refused += 1
                continue
            torch.cuda.synchronize()
            fused += eng.last_kernel() == "k_encrypt_wp"
            assert np.array_equal(packed.cpu().numpy().view(np.uint64), want.reshape(packed.shape)), (B, with_e, eng.last_kernel())
            if with_e:
                assert np.array_equal(te.cpu().numpy().view(np.uint16), e_o), B
            else:
                assert int(te.min()) == 9 and int(te.max()) == 9      # e was not written
    assert fused + refused == 4 and (fused == 4 if must_fuse else True) and (fused == 0 if not can_fuse else True)


@pytest.mark.parametrize("N,q", [(821, 4096), (701, 8192), (509, 2048), (252, 256), (253, 256), (378, 512), (1000, 1024), (127, 64)])
def test_decrypt_with_fused_pack_output_equals_oracle(eng, N, q):
    """ntru_decrypt_pack_batch_dev: decryptBits + packOutput(p - 1, N, value) (index.js:111-140, :572-596) in ONE kernel where the
    matrix path applies (k_decrypt_mp: 2-bit image of the second product's values -> packed dwords), with and without the plain
    values; sizes around the 126-column element boundary, ragged batches; against the oracle's decrypt + pack."""
    import torch
    p = 3
    dev = torch.device("cuda:0")
    rng = np.random.default_rng(N + q)
    f = ternary_rows(rng, 1, N, N // 3, N // 3 - 1, two=-1)[0].astype(np.int8)
    fp = rng.integers(0, p, N).astype(np.uint8)
    tf, tfp = torch.from_numpy(f).to(dev), torch.from_numpy(fp).to(dev)
    fused = 0
    for B in (1, 33, 777, 2 * 32 * 256 + 5):            # the last one: several row blocks per workgroup (image wiped and reused)
        e = rng.integers(0, q, (B, N)).astype(np.uint16)
        te = torch.from_numpy(e.view(np.int16)).to(dev)
        v_o = orc.decrypt_batch(N, q, p, f, fp, e, want_witness=False)[0]
        want = orc.pack_batch(p - 1, N, v_o.astype(np.uint16)).view(np.uint64)
        for with_value in (True, False):
            packed = torch.full(want.shape, -1, dtype=torch.int64, device=dev)
            val = torch.full((B, N), 9, dtype=torch.uint8, device=dev)
            eng.decrypt_pack_batch_dev(N, q, p, tf.data_ptr(), tfp.data_ptr(), te.data_ptr(), B, val.data_ptr() if with_value else None,
                                       packed.data_ptr())
            torch.cuda.synchronize()
            fused += eng.last_kernel() == "k_decrypt_mp"
            assert np.array_equal(packed.cpu().numpy().view(np.uint64), want.reshape(packed.shape)), (B, with_value, eng.last_kernel())
            if with_value:
                assert np.array_equal(val.cpu().numpy(), v_o), B
            elif eng.last_kernel() == "k_decrypt_mp":
                assert int(val.min()) == 9                  # the plain values were not written
    assert fused == 8 or N < 256                            # the fused kernel is what ran (tiny N: the image does not fit behind the tables)
