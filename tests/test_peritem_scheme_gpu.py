"""ntru_encrypt_peritem_batch[_dev] / ntru_decrypt_peritem_batch[_dev] on the GPU: every row against a per-item oracle built from
oracle.ntru_oracle.polymul_split_batch, against the shared-key oracle with B = 1 per key, across the parameter domain and the kernel
paths, at every N of the matrix kernels on edge operands, on ragged and offset batches, against the shared-key calls when every key is the same, and at full size on keys generated on
the device."""
import ctypes as C
import json
import os

import numpy as np
import pytest

import __graft_entry__ as ge
from oracle import ntru_oracle as orc
from peritem_ref import decrypt_operands, encrypt_operands, oracle_decrypt, oracle_encrypt

pytestmark = pytest.mark.gpu
pkg = ge.load_package()

ERR_ARG, ERR_UNSUPPORTED = 2, 3
NS = [2, 17, 63, 64, 127, 128, 167, 509, 701, 821, 864, 1024, 1025, 1920]
QS = [32, 256, 2048, 4096, 8192, 16384, 65536]


@pytest.fixture(scope="module")
def eng():
    e = pkg.Engine(0)
    yield e
    e.set_kernel_path(0)


@pytest.fixture(scope="module")
def torch_dev():
    import torch
    return torch, torch.device("cuda:0")


def options(name):
    with open(os.path.join(ge.ROOT, "tests", "golden", "scheme_%s.json" % name)) as fh:
        return json.load(fh)["options"]


def inputs(N, q, p, B, seed):
    """Per-item keys and messages inside the symbol preconditions: h, e < q; r in {0,1,2}; any byte of m; f in {-1,0,1}; fp < p."""
    g = np.random.default_rng(seed)
    return {"h": g.integers(0, q, (B, N), dtype=np.uint16), "r": g.integers(0, 3, (B, N), dtype=np.uint8),
            "m": g.integers(0, 256, (B, N), dtype=np.uint8), "f": g.integers(-1, 2, (B, N), dtype=np.int8),
            "fp": g.integers(0, p, (B, N), dtype=np.uint8), "e": g.integers(0, q, (B, N), dtype=np.uint16)}


def matrix_expected(path, N, q, p=3):
    return path in (0, 4) and q <= 8192 and N <= 1024 and N >= (64 if path == 4 else 128) and p == 3


def check_rows(got, want, what):
    for g_, w_, name in zip(got, want, what):
        bad = np.nonzero((g_ != w_).any(axis=1))[0]
        assert bad.size == 0, (name, bad[:8].tolist())


# ---- the parameter domain x kernel paths, against the per-item oracle ----------------------------------------------------------------
@pytest.mark.parametrize("N", NS)
@pytest.mark.parametrize("q", QS)
def test_sweep_against_the_oracle(eng, N, q):
    B = 37
    for path in (0, 1, 4):
        eng.set_kernel_path(path)
        x = inputs(N, q, 3, B, seed=N * 131 + q + path)
        e, quot = eng.encrypt_peritem_batch(N, q, x["h"], x["r"], x["m"])
        lk = eng.last_kernel()
        assert (lk == "k_encrypt_pi_m") == matrix_expected(path, N, q), (path, lk)
        check_rows((e, quot), oracle_encrypt(N, q, x["h"], x["r"], x["m"]), ("e", "quotE"))
        for p in (3, 5):
            xp = inputs(N, q, p, B, seed=N * 7 + q + p + path)
            got = eng.decrypt_peritem_batch(N, q, p, xp["f"], xp["fp"], xp["e"])
            lk = eng.last_kernel()
            assert (lk == "k_decrypt_pi_m") == matrix_expected(path, N, q, p), (path, p, lk)
            assert "k_encrypt_pi_m" not in lk
            check_rows(got, oracle_decrypt(N, q, p, xp["f"], xp["fp"], xp["e"]), ("value", "quot1", "rem1", "quot2"))
    eng.set_kernel_path(0)


# ---- every N of the matrix kernels: NT = ceil(N / 32), the column mask at N mod 16, the split diagonal -------------------------------
EVERY_N = [r.tolist() for r in np.array_split(np.arange(64, 1025), 20)]
FILL = 0xA5


@pytest.mark.parametrize("ns", EVERY_N, ids=["%d-%d" % (r[0], r[-1]) for r in EVERY_N])
def test_peritem_every_n(eng, ns):
    """Every N from 64 to 1024 at kernel path 4 and from 128 at path 0, q = 256 (one digit plane) and 8192 (two), B = 3: row 0 the
    extremes, row 1 f = x^(N-1) against an e row of 0, q/2, q/2 + 1, q - 1 (rem1 is its rotation: the strict `>` of the lift at q/2),
    row 2 random.  Encrypt and decrypt with every witness, every output bit against the oracle; outputs start as FILL bytes."""
    B, NMAX = 3, 1024
    rng = np.random.default_rng(ns[0])
    bufs = [eng.dev_alloc(B * NMAX * 2) for _ in range(7)]                   # device buffers of the whole sweep, sized for N = 1024
    fill = np.full(B * NMAX * 2, FILL, np.uint8)

    def call(fn, head, ins, out_dts):
        N = ins[0].shape[1]
        outs = bufs[len(ins):len(ins) + len(out_dts)]
        for ptr, a in zip(bufs, ins):
            eng.dev_upload(ptr, np.ascontiguousarray(a))
        for ptr, dt in zip(outs, out_dts):
            eng.dev_upload(ptr, fill[:B * N * np.dtype(dt).itemsize])
        fn(*head, *bufs[:len(ins)], B, *outs)
        return [eng.dev_download(ptr, (B, N), dt) for ptr, dt in zip(outs, out_dts)]

    try:
        for N in ns:
            for path in ((4, 0) if N >= 128 else (4,)):
                eng.set_kernel_path(path)
                for q in (256, 8192):
                    h, r, m = encrypt_operands(rng, N, q, B)
                    got = call(eng.encrypt_peritem_batch_dev, (N, q), (h, r, m), (np.uint16, np.uint16))
                    assert eng.last_kernel() == "k_encrypt_pi_m", (N, q, path, eng.last_kernel())
                    check_rows(got, oracle_encrypt(N, q, h, r, m), [(name, N, q, path) for name in ("e", "quotE")])
                    f, fp, e = decrypt_operands(rng, N, q, 3, B)
                    want = oracle_decrypt(N, q, 3, f, fp, e)
                    assert (want[2][1] == q // 2).any() and (want[2][1] == q // 2 + 1).any(), (N, q)     # row 1: the lift's edge
                    got = call(eng.decrypt_peritem_batch_dev, (N, q, 3), (f, fp, e), (np.uint8, np.uint16, np.uint16, np.uint8))
                    assert eng.last_kernel() == "k_decrypt_pi_m", (N, q, path, eng.last_kernel())
                    check_rows(got, want, [(name, N, q, path) for name in ("value", "quot1", "rem1", "quot2")])
    finally:
        eng.set_kernel_path(0)
        eng.synchronize()
        for ptr in bufs:
            eng.dev_free(ptr)


@pytest.mark.parametrize("name", ["n17_q32", "n167_q128", "n509_q2048", "n821_q4096", "n701_q8192"])
def test_loop_of_shared_key_oracle_calls(eng, name):
    """Row b equals the shared-key oracle (orc.encrypt_batch / orc.decrypt_batch) called with B = 1 under key b."""
    o = options(name)
    N, q, p = o["N"], o["q"], o["p"]
    B = 24
    x = inputs(N, q, p, B, seed=N)
    x["m"] %= 3
    e, quot = eng.encrypt_peritem_batch(N, q, x["h"], x["r"], x["m"])
    value, q1, r1, q2 = eng.decrypt_peritem_batch(N, q, p, x["f"], x["fp"], e)
    for b in range(B):
        eo, qo = orc.encrypt_batch(N, q, x["h"][b], x["r"][b:b + 1], x["m"][b:b + 1])
        assert np.array_equal(e[b], eo[0]) and np.array_equal(quot[b], qo[0]), b
        vo, q1o, r1o, q2o = orc.decrypt_batch(N, q, p, x["f"][b], x["fp"][b], e[b:b + 1])
        for got, want in ((value, vo), (q1, q1o), (r1, r1o), (q2, q2o)):
            assert np.array_equal(got[b], want[0]), b


# ---- batch edges: ragged B, a batch that wraps the resident grid more than once, pointers off by one element --------------------------
def _dev(torch, dev, a, offset=0):
    """a on the device starting `offset` elements into its allocation; returns (tensor, pointer)."""
    dt = {np.dtype(np.uint16): torch.int16, np.dtype(np.uint8): torch.uint8, np.dtype(np.int8): torch.int8}[a.dtype]
    t = torch.zeros(a.size + offset, dtype=dt, device=dev)
    t[offset:] = torch.from_numpy(a.reshape(-1).view({np.dtype(np.uint16): np.int16}.get(a.dtype, a.dtype)).copy()).to(dev)
    return t, t.data_ptr() + offset * a.itemsize


def _run_dev(eng, torch, dev, N, q, p, x, B, offset):
    keep = []
    def put(a):
        t, ptr = _dev(torch, dev, a, offset)
        keep.append(t)
        return ptr
    def out(dt, bytes_):
        t = torch.zeros(B * N * bytes_ + offset * bytes_, dtype=torch.uint8, device=dev)
        keep.append(t)
        return t, t.data_ptr() + offset * bytes_
    te, pe = out(None, 2); tq, pq = out(None, 2)
    eng.encrypt_peritem_batch_dev(N, q, put(x["h"]), put(x["r"]), put(x["m"]), B, pe, pq)
    lk_enc = eng.last_kernel()
    tv, pv = out(None, 1); t1, p1 = out(None, 2); t2, p2 = out(None, 2); t3, p3 = out(None, 1)
    eng.decrypt_peritem_batch_dev(N, q, p, put(x["f"]), put(x["fp"]), put(x["e"]), B, pv, p1, p2, p3)
    lk_dec = eng.last_kernel()
    torch.cuda.synchronize()
    host = lambda t, n, dt: t.cpu().numpy()[offset * n:].view(dt).reshape(B, N)
    return ((host(te, 2, np.uint16), host(tq, 2, np.uint16)),
            (host(tv, 1, np.uint8), host(t1, 2, np.uint16), host(t2, 2, np.uint16), host(t3, 1, np.uint8)), lk_enc, lk_dec)


@pytest.mark.parametrize("N,q", [(167, 128), (821, 4096), (1024, 8192), (1920, 65536)])
@pytest.mark.parametrize("B,offset", [(1, 0), (3, 1), (257, 1), (1001, 0)])
def test_ragged_and_offset_batches(eng, torch_dev, N, q, B, offset):
    torch, dev = torch_dev
    x = inputs(N, q, 3, B, seed=B * 3 + offset + N)
    enc, dec, lk_enc, lk_dec = _run_dev(eng, torch, dev, N, q, 3, x, B, offset)
    assert (lk_enc == "k_encrypt_pi_m") == (lk_dec == "k_decrypt_pi_m") == matrix_expected(0, N, q)
    check_rows(enc, oracle_encrypt(N, q, x["h"], x["r"], x["m"]), ("e", "quotE"))
    check_rows(dec, oracle_decrypt(N, q, 3, x["f"], x["fp"], x["e"]), ("value", "quot1", "rem1", "quot2"))


@pytest.mark.parametrize("N,q", [(128, 256), (509, 2048)])
def test_batch_wrapping_the_resident_grid(eng, torch_dev, N, q):
    """More items than co-resident waves several times over (every wave walks many items), a ragged tail; a seeded sample of rows."""
    torch, dev = torch_dev
    B = 3 * 65536 + 7
    x = inputs(N, q, 3, B, seed=N + q)
    enc, dec, lk_enc, lk_dec = _run_dev(eng, torch, dev, N, q, 3, x, B, 1)
    assert lk_enc == "k_encrypt_pi_m" and lk_dec == "k_decrypt_pi_m"
    rows = np.unique(np.concatenate([np.random.default_rng(5).choice(B, 1500, replace=False), np.arange(B - 40, B), np.arange(40)]))
    sub = {k: v[rows] for k, v in x.items()}
    check_rows([a[rows] for a in enc], oracle_encrypt(N, q, sub["h"], sub["r"], sub["m"]), ("e", "quotE"))
    check_rows([a[rows] for a in dec], oracle_decrypt(N, q, 3, sub["f"], sub["fp"], sub["e"]), ("value", "quot1", "rem1", "quot2"))


# ---- every key equal: bit for bit the shared-key calls, at 2^18 items ---------------------------------------------------------------
@pytest.mark.parametrize("N,q,path", [(821, 4096, 0), (701, 8192, 0), (167, 128, 0), (821, 4096, 1), (1920, 65536, 0)])
def test_all_keys_equal_matches_the_shared_key_calls(eng, torch_dev, N, q, path):
    torch, dev = torch_dev
    B = 1 << 18 if N <= 1024 and path == 0 else 1 << 13
    g = torch.Generator(device=dev).manual_seed(N + q)
    rnd = lambda hi, shape, dt: torch.randint(0, hi, shape, generator=g, device=dev, dtype=torch.int32).to(dt)
    h1, f1, fp1 = rnd(q, (N,), torch.int32), (rnd(3, (N,), torch.int32) - 1).to(torch.int8), rnd(3, (N,), torch.uint8)
    h1 = h1.to(torch.int16)
    r, m = rnd(3, (B, N), torch.uint8), rnd(256, (B, N), torch.uint8)
    H, F, FP = h1.expand(B, N).contiguous(), f1.expand(B, N).contiguous(), fp1.expand(B, N).contiguous()
    z16, z8 = lambda: torch.empty((B, N), dtype=torch.int16, device=dev), lambda: torch.empty((B, N), dtype=torch.uint8, device=dev)
    eng.set_kernel_path(path)
    try:
        e1, qe1, e2, qe2 = z16(), z16(), z16(), z16()
        eng.encrypt_peritem_batch_dev(N, q, H.data_ptr(), r.data_ptr(), m.data_ptr(), B, e1.data_ptr(), qe1.data_ptr())
        eng.encrypt_batch_dev(N, q, h1.data_ptr(), r.data_ptr(), m.data_ptr(), B, e2.data_ptr(), qe2.data_ptr())
        outs = [[z8(), z16(), z16(), z8()] for _ in range(2)]
        eng.decrypt_peritem_batch_dev(N, q, 3, F.data_ptr(), FP.data_ptr(), e1.data_ptr(), B, *[t.data_ptr() for t in outs[0]])
        eng.decrypt_batch_dev(N, q, 3, f1.data_ptr(), fp1.data_ptr(), e1.data_ptr(), B, *[t.data_ptr() for t in outs[1]])
        torch.cuda.synchronize()
    finally:
        eng.set_kernel_path(0)
    assert torch.equal(e1, e2) and torch.equal(qe1, qe2)
    for a, b in zip(*outs):
        assert torch.equal(a, b)


# ---- optional outputs -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("N,q", [(821, 4096), (167, 128), (1920, 65536), (64, 2048)])
def test_null_witness_outputs(eng, N, q):
    B = 300
    x = inputs(N, q, 3, B, seed=99)
    e, quot = eng.encrypt_peritem_batch(N, q, x["h"], x["r"], x["m"])
    e0, none = eng.encrypt_peritem_batch(N, q, x["h"], x["r"], x["m"], want_quot=False)
    assert none is None and np.array_equal(e, e0)
    full = eng.decrypt_peritem_batch(N, q, 3, x["f"], x["fp"], e)
    lean = eng.decrypt_peritem_batch(N, q, 3, x["f"], x["fp"], e, want_witness=False)
    assert lean[1] is None and np.array_equal(full[0], lean[0])
    # one witness array at a time, through the raw ABI
    lib, h = eng._lib, eng._h
    ptr = lambda a: a.ctypes.data_as(C.c_void_p)
    for k in range(3):
        outs = [np.zeros((B, N), dt) if i == k else None for i, dt in enumerate((np.uint16, np.uint16, np.uint8))]
        v = np.zeros((B, N), np.uint8)
        assert lib.ntru_decrypt_peritem_batch(h, N, q, 3, ptr(x["f"]), ptr(x["fp"]), ptr(e), B, ptr(v),
                                              *[None if o is None else ptr(o) for o in outs]) == 0
        assert np.array_equal(v, full[0]) and np.array_equal(outs[k], full[1 + k])


# ---- host form = _dev form across chunk boundaries, ordinary and pinned arrays ----------------------------------------------------------
@pytest.mark.parametrize("N,q", [(821, 4096), (1920, 65536)])
def test_host_form_equals_dev_form(eng, torch_dev, N, q):
    torch, dev = torch_dev
    B = 9001                                                  # four pipeline chunks, a ragged last one
    x = inputs(N, q, 3, B, seed=4)
    enc_d, dec_d, _, _ = _run_dev(eng, torch, dev, N, q, 3, x, B, 0)
    enc_h = eng.encrypt_peritem_batch(N, q, x["h"], x["r"], x["m"])
    dec_h = eng.decrypt_peritem_batch(N, q, 3, x["f"], x["fp"], x["e"])
    check_rows(enc_h, enc_d, ("e", "quotE"))
    check_rows(dec_h, dec_d, ("value", "quot1", "rem1", "quot2"))
    # pinned inputs and outputs: DMA'd in place
    pin = {}
    for k, a in x.items():
        pin[k] = eng.pinned_empty(a.shape, a.dtype)
        pin[k][...] = a
    lib, hd = eng._lib, eng._h
    ptr = lambda a: a.ctypes.data_as(C.c_void_p)
    e, qe = eng.pinned_empty((B, N), np.uint16), eng.pinned_empty((B, N), np.uint16)
    assert lib.ntru_encrypt_peritem_batch(hd, N, q, ptr(pin["h"]), ptr(pin["r"]), ptr(pin["m"]), B, ptr(e), ptr(qe)) == 0
    check_rows((e, qe), enc_d, ("e", "quotE"))
    v, q1, r1, q2 = (eng.pinned_empty((B, N), dt) for dt in (np.uint8, np.uint16, np.uint16, np.uint8))
    assert lib.ntru_decrypt_peritem_batch(hd, N, q, 3, ptr(pin["f"]), ptr(pin["fp"]), ptr(pin["e"]), B, ptr(v), ptr(q1), ptr(r1),
                                          ptr(q2)) == 0
    check_rows((v, q1, r1, q2), dec_d, ("value", "quot1", "rem1", "quot2"))


# ---- argument errors: refused before any launch ------------------------------------------------------------------------------------
def test_argument_errors(eng):
    lib, h = eng._lib, eng._h
    N, q, B = 167, 128, 4
    x = inputs(N, q, 3, B, seed=1)
    ptr = lambda a: a.ctypes.data_as(C.c_void_p)
    e, quot, v = np.zeros((B, N), np.uint16), np.zeros((B, N), np.uint16), np.zeros((B, N), np.uint8)
    eng.encrypt_peritem_batch(N, q, x["h"], x["r"], x["m"])
    assert eng.last_kernel() == "k_encrypt_pi_m"
    for form in ("", "_dev"):
        enc = getattr(lib, "ntru_encrypt_peritem_batch" + form)
        dec = getattr(lib, "ntru_decrypt_peritem_batch" + form)
        E = lambda h_=h, N_=N, q_=q, B_=B, hh=ptr(x["h"]), r=ptr(x["r"]), m=ptr(x["m"]), out=ptr(e): enc(h_, N_, q_, hh, r, m, B_, out, ptr(quot))
        D = lambda h_=h, N_=N, q_=q, p_=3, B_=B, f=ptr(x["f"]), fp=ptr(x["fp"]), ee=ptr(x["e"]), out=ptr(v): dec(
            h_, N_, q_, p_, f, fp, ee, B_, out, None, None, None)
        for call in (E, D):
            assert call(h_=None) == ERR_ARG
            assert call(B_=-1) == ERR_ARG
            for bad_n in (1, 0, -5, 1921):
                assert call(N_=bad_n) == ERR_UNSUPPORTED, bad_n
            for bad_q in (3000, 1, 131072, 0):
                assert call(q_=bad_q) == ERR_UNSUPPORTED, bad_q
            assert call(B_=0) == 0
        assert E(hh=None) == ERR_ARG and E(r=None) == ERR_ARG and E(m=None) == ERR_ARG and E(out=None) == ERR_ARG
        assert D(f=None) == ERR_ARG and D(fp=None) == ERR_ARG and D(ee=None) == ERR_ARG and D(out=None) == ERR_ARG
        for bad_p in (2, 4, 1, 0, 255):
            assert D(p_=bad_p) == ERR_UNSUPPORTED, bad_p
        assert D(N_=1920, p_=7) == ERR_UNSUPPORTED                # N (p - 1)^2 >= 65536
        # B == 0 with every buffer NULL is a no-op
        assert enc(h, N, q, None, None, None, 0, None, None) == 0
        assert dec(h, N, q, 3, None, None, None, 0, None, None, None, None) == 0
    assert eng.last_kernel() == "k_encrypt_pi_m"                # nothing above launched


# ---- full size: keys generated on the device, r sampled on the device --------------------------------------------------------------
@pytest.mark.parametrize("name", ["n821_q4096", "n701_q8192"])
def test_full_size_on_generated_keys(eng, torch_dev, name):
    """2^18 key pairs (ntru_keygen_batch_dev), r from ntru_sample_ternary_dev, per-item encrypt then per-item decrypt.  A seeded sample of
    4096 rows equals the oracle; VerifyEncrypt flags no row, VerifyDecrypt none of the sample.  The round trip value == m holds where
    the reference's lift `x > q/2 ? (x+1)%p : x%p` is the centred one, q = 2 mod 3 (8192); at q = 4096 (1 mod 3) it is off by the
    reference's own quirk, so there parity with the oracle is what is asserted."""
    torch, dev = torch_dev
    o = options(name)
    N, q, p, df, dg, dr = o["N"], o["q"], o["p"], o["df"], o["dg"], o["dr"]
    B = 1 << 18
    key = np.array([0x51ED2701 * (i + 3) & 0xFFFFFFFF for i in range(8)], np.uint32)
    rkey = np.array([0x2545F491 * (i + 5) & 0xFFFFFFFF for i in range(8)], np.uint32)
    d = lambda dt, shape=(B, N): torch.empty(shape, dtype=dt, device=dev)
    f, g, fq, fp, h = d(torch.int8), d(torch.int8), d(torch.int16), d(torch.uint8), d(torch.int16)
    flags, work = d(torch.uint8, (B,)), d(torch.uint8, (eng.keygen_workspace_bytes(N, B),))
    eng.keygen_batch_dev(N, q, p, df, dg, key, 0, 100, B, work.data_ptr(), f.data_ptr(), g.data_ptr(), fq.data_ptr(), fp.data_ptr(),
                         h.data_ptr(), None, flags.data_ptr())
    del work
    r = d(torch.uint8)
    eng.sample_ternary_dev(N, dr, dr, p - 1, rkey, 0, B, r.data_ptr())
    m = torch.randint(0, 3, (B, N), generator=torch.Generator(device=dev).manual_seed(3), device=dev, dtype=torch.int32).to(torch.uint8)
    e, qe = d(torch.int16), d(torch.int16)
    eng.encrypt_peritem_batch_dev(N, q, h.data_ptr(), r.data_ptr(), m.data_ptr(), B, e.data_ptr(), qe.data_ptr())
    assert eng.last_kernel() == "k_encrypt_pi_m"
    v, q1, r1, q2 = d(torch.uint8), d(torch.int16), d(torch.int16), d(torch.uint8)
    eng.decrypt_peritem_batch_dev(N, q, p, f.data_ptr(), fp.data_ptr(), e.data_ptr(), B, v.data_ptr(), q1.data_ptr(), r1.data_ptr(),
                                  q2.data_ptr())
    assert eng.last_kernel() == "k_decrypt_pi_m"
    torch.cuda.synchronize()
    assert not flags.any().item()
    if q % 3 == 2:
        assert torch.equal(v, m)
    # VerifyEncrypt over every row (device-resident checker), VerifyDecrypt over the sample
    nq, np_ = int(np.ceil(np.log2(float(q) * q * N))), int(np.ceil(np.log2(float(p) * p * N)))
    u16 = lambda t: t.to(torch.int32).bitwise_and(0xFFFF).to(torch.int32)
    pad = lambda t: torch.cat([t.to(torch.int32), torch.zeros((t.shape[0], 1), dtype=torch.int32, device=dev)], 1)
    to16 = lambda t: t.to(torch.int16).contiguous()
    enc_in = [to16(r), to16(m), h, to16(pad(u16(qe))), to16(pad(u16(e)))]
    fl = d(torch.uint8, (B,))
    eng.check_encrypt_batch_dev(N, q, nq, *[t.data_ptr() for t in enc_in], B, fl.data_ptr())
    torch.cuda.synchronize()
    assert not fl.any().item()
    del enc_in
    rows = torch.from_numpy(np.sort(np.random.default_rng(11).choice(B, 4096, replace=False))).to(dev)
    host = lambda t: t.index_select(0, rows).cpu().numpy()
    hh, rr, mm = host(h).view(np.uint16), host(r), host(m)
    fh, fph, eh = host(f), host(fp), host(e).view(np.uint16)
    check_rows((eh, host(qe).view(np.uint16)), oracle_encrypt(N, q, hh, rr, mm), ("e", "quotE"))
    dec = (host(v), host(q1).view(np.uint16), host(r1).view(np.uint16), host(q2))
    check_rows(dec, oracle_decrypt(N, q, p, fh, fph, eh), ("value", "quot1", "rem1", "quot2"))
    ext = lambda a: np.concatenate([a.astype(np.uint16), np.zeros((a.shape[0], 1), np.uint16)], 1)
    f_q = (fh.astype(np.int64) % q).astype(np.uint16)
    flags_d = eng.check_decrypt_batch(N, q, nq, p, np_, f_q, fph, eh, ext(dec[1]), ext(dec[2]), ext(dec[3]), ext(dec[0]))
    assert not flags_d.any()


# ---- the Python shim ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["n167_q128", "n509_q2048", "n17_q32"])
def test_python_shim_rows_equal_single_key_calls(eng, name):
    o = options(name)
    N, q, p = o["N"], o["q"], o["p"]
    B = 200
    nt = pkg.ntru.NTRU(dict(o), engine=eng)
    keys = nt.generateKeysBatch(B, np.arange(1, 9, dtype=np.uint32))
    B = int(np.argmax(keys["flags"] != 0)) if keys["flags"].any() else B     # the used items are the unflagged ones in front
    assert B > 20
    g = np.random.default_rng(2)
    r = g.integers(-1, 2, (B, N)).astype(np.int8)
    m = g.integers(0, 3, (B, N)).astype(np.uint8)
    enc = nt.encryptBatchPerKey(keys, r, m)
    dec = nt.decryptBatchPerKey(keys, enc["e"])
    for i in list(range(0, B, max(1, B // 12))) + [B - 1]:
        one = pkg.ntru.NTRU(dict(o), engine=eng).loadKeyFromBatch(keys, i)
        wi = one.encryptBits(m[i].tolist(), r[i].tolist())["inputs"]
        assert wi["remainderE"][:N] == enc["e"][i].tolist() and wi["quotientE"][:N] == enc["quotientE"][i].tolist(), i
        wd = one.decryptBits(enc["e"][i].tolist())["inputs"]
        for k_ in ("quotient1", "remainder1", "quotient2"):
            assert wd[k_][:N] == dec[k_][i].tolist(), (i, k_)
        assert wd["remainder2"][:N] == dec["value"][i].tolist(), i
    bad = dict(keys)
    bad["flags"] = keys["flags"].copy()
    bad["flags"][B - 1] = 1
    with pytest.raises(ValueError, match="Could not find invertible f"):
        nt.encryptBatchPerKey(bad, r, m)
    with pytest.raises(ValueError, match="Could not find invertible f"):
        nt.decryptBatchPerKey(bad, enc["e"])
