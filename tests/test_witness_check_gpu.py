"""Witness checks on the MI355X (ntru_check_*_batch): the kernels' flags against the closed-form evaluator of tests/witness_circuit.py,
byte for byte -- golden witnesses, single-entry mutations, range edges, engine-produced batches, batch sizes and N at the limits."""
import numpy as np
import pytest

import __graft_entry__ as ge
import witness_circuit as wc
from conftest import PROFILES, load_golden

pkg = ge.load_package()
pytestmark = pytest.mark.gpu
U16 = np.uint16


@pytest.fixture(scope="module")
def eng():
    return pkg.Engine(0)


@pytest.fixture(scope="module")
def golden():
    return wc.golden_witnesses(load_golden, PROFILES)


def gpu_check(eng, template, params, arrays):
    a = [np.asarray(x, U16) for x in arrays]
    if template == "VerifyEncrypt":
        out = eng.check_encrypt_batch(params[2], params[0], params[1], *a)
    elif template == "VerifyDecrypt":
        out = eng.check_decrypt_batch(params[4], params[0], params[1], params[2], params[3], *a)
    else:
        out = eng.check_inverse_batch(params[2], params[0], params[1], *a)
    assert eng.last_kernel() == {"VerifyEncrypt": "k_check_encrypt", "VerifyDecrypt": "k_check_decrypt",
                                 "VerifyInverse": "k_check_inverse"}[template]
    return out


def agree(eng, template, params, arrays):
    got = gpu_check(eng, template, params, arrays)
    want = wc.numpy_check(template, params, arrays)
    bad = np.nonzero(got != want)[0]
    assert bad.size == 0, (template, params, bad[:8].tolist(), got[bad[:8]].tolist(), want[bad[:8]].tolist())
    return got


def test_golden_witnesses_are_accepted(eng, golden):
    for template, ws in golden.items():
        for params, grp in wc.by_params(ws).items():
            p, arrays = wc.stack(template, grp)
            assert gpu_check(eng, template, p, arrays).tolist() == [0] * len(grp), (template, params)


@pytest.mark.parametrize("template", wc.TEMPLATES)
def test_mutations_match_the_evaluator(eng, golden, template):
    rng = np.random.default_rng(3)
    seen = set()
    for params, ws in wc.by_params(golden[template]).items():
        batch = []
        for w in ws[:3]:
            batch += wc.mutations(template, w, rng)
        p, arrays = wc.stack(template, batch)
        seen |= set(agree(eng, template, p, arrays).tolist())
    assert 0 in seen and len(seen) >= 4, seen


def test_range_edges(eng):
    """x = T - 1 passes ltQ, x = T fails it: the product's x through one entry of fq (f = 1), then a quotient / remainder side at T."""
    rng = np.random.default_rng(9)
    for M, n in ((4096, 12), (3, 2), (1000, 10), (3000, 11), (65536, 16), (7, 5), (2, 1), (40000, 15)):
        T = wc.T_bound(M, n)
        N = 5
        for x in (T - 1, T):
            if x > 65535:
                continue
            f = np.zeros((2, N), np.int64); f[:, 0] = 1
            fq = np.zeros((2, N), np.int64); fq[0, 0] = x; fq[1, N - 1] = x          # a coefficient k < N and k = N - 1
            arrays = wc.honest_inverse(M, N, f, fq)
            got = agree(eng, "VerifyInverse", (M, n, N), arrays)
            assert got.tolist() == ([wc.RANGE] * 2 if x == T else [0] * 2) or (M - (1 << n) > 0), (M, n, x, got)
            # encrypt: x = h_0 + m_0 with r = 1 at 0
            r = np.zeros((1, N), np.int64); r[0, 0] = 1
            h = np.zeros((1, N), np.int64); h[0, 0] = x // 2
            m = np.zeros((1, N), np.int64); m[0, 0] = x - x // 2
            agree(eng, "VerifyEncrypt", (M, n, N), wc.honest_encrypt(M, N, r, m, h))
            # P side: quotient + remainder at T (k < N), (M - 1) Q_0 + Q_N + R_N (k = N)
            Q = np.zeros((2, N + 1), np.int64); R = np.zeros((2, N + 1), np.int64)
            Q[0, 1] = min(x, 65535); R[0, 1] = x - Q[0, 1]
            Q[1, N] = x // 2; R[1, N] = x - x // 2
            agree(eng, "VerifyInverse", (M, n, N), [np.zeros((2, N), np.int64), np.zeros((2, N), np.int64), Q, R])
    # decrypt's LessThan(nq)(q / 2, remainder1[i]): valid iff q/2 - 2^nq < x <= q/2 + 2^nq
    q, p, N = 64, 3, 4
    for nq in (3, 4, 5):
        for x in (q // 2 - (1 << nq), q // 2 - (1 << nq) + 1, q // 2, q // 2 + 1, q // 2 + (1 << nq), q // 2 + (1 << nq) + 1):
            arrays = wc.honest_decrypt(q, p, N, np.zeros((1, N), np.int64), rng.integers(0, p, (1, N)), rng.integers(0, q, (1, N)))
            arrays[4][0, 1] = x
            agree(eng, "VerifyDecrypt", (q, nq, p, 4, N), arrays)


def _keys(eng, N, q, B, rng):
    """B key pairs from the engine: f ternary (units only), fq / fp its inverses, h = p fq g."""
    df = max(1, N // 3)
    f = np.zeros((B, N), np.int8)
    for b in range(B):
        perm = rng.permutation(N)
        f[b, perm[:df + 1]] = 1
        f[b, perm[df + 1:2 * df + 1]] = -1
    fq, fp, flags = eng.invert_key_batch(N, q, 3, f)
    g = rng.choice(np.array([-1, 0, 1], np.int8), (B, N))
    h = eng.public_key_batch(N, q, 3, fq, g)
    return f, g, fq, fp, h, flags


def _pad(a):
    a = np.asarray(a, np.int64)
    return np.concatenate([a, np.zeros((a.shape[0], 1), np.int64)], 1)


def _mutate_eighth(template, params, arrays, rng):
    """One random entry changed in a random eighth of the items; returns the changed item indices."""
    B = arrays[0].shape[0]
    items = rng.choice(B, B // 8, replace=False)
    sig = rng.integers(0, len(arrays), items.size)
    for it, s in zip(items, sig):
        L = arrays[s].shape[1]
        idx = int(rng.integers(0, L))
        arrays[s][it, idx] = int(rng.choice([arrays[s][it, idx] + 1, arrays[s][it, idx] + params[0], 0, 65535,
                                             int(rng.integers(0, 65536))])) % 65536
    return items


def _honest_then_mutated(eng, template, params, arrays, rng):
    got = gpu_check(eng, template, params, arrays)
    assert not got.any(), (template, params, np.nonzero(got)[0][:8])
    assert not wc.numpy_check(template, params, [a[:256] for a in arrays]).any()
    items = _mutate_eighth(template, params, arrays, rng)
    got = gpu_check(eng, template, params, arrays)
    want = np.zeros_like(got)
    want[items] = wc.numpy_check(template, params, [a[items] for a in arrays])
    bad = np.nonzero(got != want)[0]
    assert bad.size == 0, (template, params, bad[:8].tolist(), got[bad[:8]].tolist(), want[bad[:8]].tolist())
    assert want.any()


@pytest.mark.parametrize("N,q", [(821, 4096), (701, 8192), (509, 2048)])
def test_engine_produced_batches(eng, N, q):
    B = 1 << 16
    rng = np.random.default_rng(N)
    nq = wc.calc_nbits(q, N)
    # the whole honest batch through the evaluator once per template (closed form, all items)
    f, g, fq, fp, h, kflags = _keys(eng, N, q, 64, rng)
    key = int(np.nonzero(kflags == 0)[0][0])
    r = np.zeros((B, N), np.uint8)
    dr = N // 3
    for b in range(B):
        perm = rng.permutation(N)
        r[b, perm[:dr]] = 1
        r[b, perm[dr:2 * dr]] = 2
    m = rng.integers(0, 2, (B, N), dtype=np.uint8)
    e, quotE = eng.encrypt_batch(N, q, h[key], r, m)
    enc = [r.astype(np.int64), m.astype(np.int64), np.broadcast_to(h[key].astype(np.int64), (B, N)).copy(), _pad(quotE), _pad(e)]
    assert not wc.numpy_check("VerifyEncrypt", (q, nq, N), enc).any()
    _honest_then_mutated(eng, "VerifyEncrypt", (q, nq, N), enc, rng)
    fmodq = np.where(f[key] < 0, q - 1, f[key].astype(np.int64))
    for p in (3, 5, 7):
        fpp = rng.integers(0, p, N).astype(np.uint8) if p != 3 else fp[key]
        value, q1, r1, q2 = eng.decrypt_batch(N, q, p, f[key], fpp, e)
        dec = [np.broadcast_to(fmodq, (B, N)).copy(), np.broadcast_to(fpp.astype(np.int64), (B, N)).copy(), e.astype(np.int64),
               _pad(q1), _pad(r1), _pad(q2), _pad(value)]
        params = (q, nq, p, wc.calc_nbits(p, N), N)
        if p == 3:
            assert not wc.numpy_check("VerifyDecrypt", params, dec).any()
        _honest_then_mutated(eng, "VerifyDecrypt", params, dec, rng)
    # verifyKeysInputs: fq, fp and h witnesses of B per-item key pairs
    f, g, fq, fp, h, kflags = _keys(eng, N, q, B, rng)
    out = eng.verify_keys_batch(N, q, 3, f, g, fq, fp, h)
    f, g = f.astype(np.int64), g.astype(np.int64)                        # -1 -> q - 1 / p - 1 as verifyKeysInputs maps it
    wit = {"fq": ((q, nq, N), [np.where(f < 0, q - 1, f), fq, out["quot_fq"], out["rem_fq"]]),
           "fp": ((3, wc.calc_nbits(3, N), N), [np.where(f < 0, 2, f), fp, out["quot_fp"], out["rem_fp"]]),
           "h": ((q, nq, N), [np.where(g < 0, q - 1, g), fq.astype(np.int64) * 3, out["quot_h"], out["rem_h"]])}
    for name, (params, (a, b, qq, rr)) in wit.items():
        arrays = [np.asarray(a, np.int64), np.asarray(b, np.int64), _pad(qq), _pad(rr)]
        _honest_then_mutated(eng, "VerifyInverse", params, arrays, rng)


@pytest.mark.parametrize("N,B", [(2, 1), (3, 63), (64, 65), (65, (1 << 16) + 1), (64, (1 << 16) + 1), (1920, 65), (1920, 1), (3, 65)])
def test_batch_sizes_and_extreme_N(eng, N, B):
    rng = np.random.default_rng(N * 7 + B)
    q, p = 2048, 3
    nq, np_ = wc.calc_nbits(q, N), wc.calc_nbits(p, N)
    enc = wc.honest_encrypt(q, N, rng.integers(0, 3, (B, N)), rng.integers(0, 3, (B, N)), rng.integers(0, q, (B, N)))
    dec = wc.honest_decrypt(q, p, N, rng.choice([0, 1, q - 1], (B, N)), rng.integers(0, p, (B, N)), rng.integers(0, q, (B, N)))
    inv = wc.honest_inverse(q, N, rng.integers(0, 65536, (B, N)), rng.integers(0, 65536, (B, N)))     # dense full-range operands
    for template, params, arrays in (("VerifyEncrypt", (q, nq, N), enc), ("VerifyDecrypt", (q, nq, p, np_, N), dec),
                                     ("VerifyInverse", (q, nq, N), inv)):
        for a in arrays:
            flip = rng.random(a.shape[0]) < 0.125
            idx = rng.integers(0, a.shape[1], a.shape[0])
            a[flip, idx[flip]] = (a[flip, idx[flip]] + 1) % 65536
        agree(eng, template, params, arrays)


def test_host_and_dev_forms_agree(eng):
    rng = np.random.default_rng(21)
    N, q, p, B = 509, 2048, 3, 1000
    nq, np_ = wc.calc_nbits(q, N), wc.calc_nbits(p, N)
    cases = {"VerifyEncrypt": ((q, nq, N), wc.honest_encrypt(q, N, rng.integers(0, 3, (B, N)), rng.integers(0, 2, (B, N)),
                                                              rng.integers(0, q, (B, N)))),
             "VerifyDecrypt": ((q, nq, p, np_, N), wc.honest_decrypt(q, p, N, rng.choice([0, 1, q - 1], (B, N)),
                                                                     rng.integers(0, p, (B, N)), rng.integers(0, q, (B, N)))),
             "VerifyInverse": ((q, nq, N), wc.honest_inverse(q, N, rng.integers(0, 3, (B, N)), rng.integers(0, q, (B, N))))}
    for template, (params, arrays) in cases.items():
        _mutate_eighth(template, params, arrays, rng)
        host = gpu_check(eng, template, params, arrays)
        ptrs = []
        try:
            for a in arrays:
                a16 = np.ascontiguousarray(a, U16)
                d = eng.dev_alloc(a16.nbytes)
                ptrs.append(d)
                eng.dev_upload(d, a16)
            d_flags = eng.dev_alloc(B)
            ptrs.append(d_flags)
            if template == "VerifyEncrypt":
                eng.check_encrypt_batch_dev(N, q, nq, *ptrs[:5], B, d_flags)
            elif template == "VerifyDecrypt":
                eng.check_decrypt_batch_dev(N, q, nq, p, np_, *ptrs[:7], B, d_flags)
            else:
                eng.check_inverse_batch_dev(N, q, nq, *ptrs[:4], B, d_flags)
            dev = eng.dev_download(d_flags, (B,), np.uint8)
        finally:
            for d in ptrs:
                eng.dev_free(d)
        assert np.array_equal(host, dev), template
        assert host.any() and not host.all()
