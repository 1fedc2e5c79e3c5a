"""ntru_sum_groups[_dev] / ntru_tally_decrypt_batch[_dev] on the GPU: the reference-captured tallies bit for bit, the numpy restatement
(tests/ciphertext_sum_ref.py) across the parameter domain, uniform and ragged groups, weights, kernel paths and alignments, the tally
against sum + decrypt, and one device-resident tally pipeline checked by the witness kernels."""
import numpy as np
import pytest

import __graft_entry__ as ge
import ciphertext_sum_ref as ref

pytestmark = pytest.mark.gpu
pkg = ge.load_package()

NS = [2, 17, 167, 509, 701, 821, 1920]
MODS = [2, 3, 128, 2048, 4096, 65536, 65521]
KS = [1, 2, 3, 64, 4097]


@pytest.fixture(scope="module")
def eng():
    e = pkg.Engine(0)
    yield e
    e.set_kernel_path(0)


class Dev:
    """Device copies of host arrays through the engine's own allocator; `shift` elements off a 256-byte boundary."""

    def __init__(self, eng):
        self.eng, self.held = eng, []

    def put(self, a, shift=0):
        a = np.ascontiguousarray(a)
        p = self.eng.dev_alloc(a.nbytes + 64)
        self.held.append(p)
        p += shift * a.itemsize
        if a.nbytes:
            self.eng.dev_upload(p, a)
        return p

    def empty(self, shape, dt, shift=0):
        return self.put(np.zeros(shape, dt), shift)

    def free(self):
        self.eng.synchronize()
        for p in self.held:
            self.eng.dev_free(p)
        self.held = []


def sum_dev(eng, N, mod, rows, offsets=None, K=None, weights=None, shift=0):
    d = Dev(eng)
    G = len(offsets) - 1 if offsets is not None else rows.shape[0] // K
    try:
        out = d.empty((G, N), np.uint16, shift)
        eng.sum_groups_dev(N, mod, d.put(rows, shift), out, G, d_offsets=None if offsets is None else d.put(np.asarray(offsets, np.int64)),
                           K=K, d_weights=None if weights is None else d.put(weights, shift))
        return eng.dev_download(out, (G, N), np.uint16)
    finally:
        d.free()


def rand(N, mod, B, seed, weighted):
    g = np.random.default_rng(seed)
    rows = g.integers(0, mod, (B, N), dtype=np.uint16)
    return rows, (g.integers(0, mod, B, dtype=np.uint16) if weighted else None)


def test_fixture_sums_and_tallies_are_the_references(eng):
    cases = ref.load_cases()
    assert len(cases) >= 12
    for c in cases:
        N, q, p, f, fp, rows, w, total = ref.case_arrays(c)
        K = rows.shape[0]
        tag = (c["set"], K, c["weights"])
        assert np.array_equal(eng.sum_groups(N, q, rows, K=K, weights=w)[0], total), tag
        assert np.array_equal(sum_dev(eng, N, q, rows, offsets=[0, K], weights=w)[0], total), tag
        got_sum, value, q1, r1, q2 = eng.tally_decrypt_batch(N, q, p, f, fp, rows, K=K, weights=w)
        inp = c["decrypt"]["inputs"]
        for got, name in ((got_sum, "e"), (q1, "quotient1"), (r1, "remainder1"), (q2, "quotient2"), (value, "remainder2")):
            assert got[0].tolist() + [0] * (len(inp[name]) - N) == inp[name], (tag, name)
        if c["recovered"]:
            assert value[0].tolist() == c["expected"], tag
        # the Python mirror of the reference's interface
        assert pkg.sumCiphertexts(c["e"], q, weights=c["weights"], engine=eng) == pkg.trimPolynomial(c["sum"])
        ntru = pkg.NTRU(dict(c["options"], f=c["key"]["f"], fp=c["key"]["fp"], h=c["key"]["h"]), engine=eng)
        t = ntru.tallyBatch(c["e"], weights=c["weights"])
        assert t["sum"][0].tolist() == c["sum"] and pkg.trimPolynomial(t["value"][0].tolist()) == c["decrypt"]["value"]
        assert t["quotient2"][0].tolist() + [0] == inp["quotient2"]


@pytest.mark.parametrize("N", NS)
def test_uniform_groups_equal_numpy(eng, N):
    for mod in MODS:
        for K in KS:
            G = max(1, 4100 // K)
            for weighted in (False, True):
                rows, w = rand(N, mod, G * K, N * 131 + mod + K, weighted)
                want = ref.np_sum(rows, mod, K=K, weights=w)
                assert np.array_equal(eng.sum_groups(N, mod, rows, K=K, weights=w), want), (N, mod, K, weighted, "host")
                assert np.array_equal(sum_dev(eng, N, mod, rows, K=K, weights=w), want), (N, mod, K, weighted, "dev")


def ragged_offsets(B, seed):
    """Empty groups, single rows, one group over most of the batch, small groups; rows before the first and behind the last offset."""
    g = np.random.default_rng(seed)
    big = B * 3 // 5
    cuts = [3, 3, 4, 5, 5, 5, 5 + big]
    rest = np.sort(g.integers(5 + big, B - 2, 40))
    return np.array(cuts + rest.tolist() + [B - 2, B - 2], np.int64)


@pytest.mark.parametrize("N,mod", [(821, 4096), (509, 2048), (167, 65521), (17, 3), (1920, 65536), (2, 2), (701, 128)])
def test_ragged_groups_equal_numpy(eng, N, mod):
    B = 20000
    off = ragged_offsets(B, N)
    for weighted in (False, True):
        rows, w = rand(N, mod, B, N + mod, weighted)
        want = ref.np_sum(rows, mod, offsets=off, weights=w)
        assert not want[0].any() and not want[-1].any()                      # empty groups give zero rows
        assert np.array_equal(eng.sum_groups(N, mod, rows, offsets=off, weights=w), want), (weighted, "host")
        assert np.array_equal(sum_dev(eng, N, mod, rows, offsets=off, weights=w), want), (weighted, "dev")
        assert np.array_equal(sum_dev(eng, N, mod, rows, offsets=off, weights=w, shift=1), want), (weighted, "dev, 2 bytes off")
        assert np.array_equal(sum_dev(eng, N, mod, rows, offsets=off, weights=w, shift=3), want), (weighted, "dev, 6 bytes off")


def test_all_groups_empty(eng):
    rows = np.ones((8, 17), np.uint16)
    off = [4] * 6
    assert not sum_dev(eng, 17, 32, rows, offsets=off).any() and not eng.sum_groups(17, 32, rows, offsets=off).any()


def test_one_group_of_2e20_rows(eng):
    N, mod, B = 821, 4096, 1 << 20
    rows, w = rand(N, mod, B, 5, True)
    for weights in (None, w):
        want = ref.np_sum(rows, mod, K=B, weights=weights)
        assert np.array_equal(sum_dev(eng, N, mod, rows, K=B, weights=weights), want)
        assert np.array_equal(eng.sum_groups(N, mod, rows, K=B, weights=weights), want)      # one group over many chunks


def test_2e18_groups_of_three(eng):
    N, mod, G = 167, 2048, 1 << 18
    rows, w = rand(N, mod, 3 * G, 6, True)
    for weights in (None, w):
        want = ref.np_sum(rows, mod, K=3, weights=weights)
        assert np.array_equal(sum_dev(eng, N, mod, rows, K=3, weights=weights), want)
        assert np.array_equal(sum_dev(eng, N, mod, rows, offsets=np.arange(0, 3 * G + 1, 3), weights=weights), want)
    assert np.array_equal(eng.sum_groups(N, mod, rows, K=3), ref.np_sum(rows, mod, K=3))


@pytest.mark.parametrize("mod", [65536, 65521])
def test_largest_weights_on_a_long_group(eng, mod):
    """w = mod - 1 on every row, entries up to mod - 1, 2^17 rows: the sum passes 2^48 before the reduction."""
    N, B = 509, 1 << 17
    rows = np.random.default_rng(9).integers(mod - 4, mod, (B, N)).astype(np.uint16)
    w = np.full(B, mod - 1, np.uint16)
    want = ref.np_sum(rows, mod, K=B, weights=w)
    assert np.array_equal(sum_dev(eng, N, mod, rows, K=B, weights=w), want)
    assert np.array_equal(eng.sum_groups(N, mod, rows, K=B, weights=w), want)


def test_kernel_paths_and_unit_weights_give_the_same_bytes(eng):
    N, mod, B = 821, 4096, 6000
    off = ragged_offsets(B, 2)
    rows, _ = rand(N, mod, B, 3, False)
    want = ref.np_sum(rows, mod, offsets=off)
    try:
        for path in (0, 1, 4):
            eng.set_kernel_path(path)
            assert sum_dev(eng, N, mod, rows, offsets=off).tobytes() == want.tobytes(), path
    finally:
        eng.set_kernel_path(0)
    assert sum_dev(eng, N, mod, rows, offsets=off, weights=np.ones(B, np.uint16)).tobytes() == want.tobytes()


def test_pairs_equal_add_batch(eng):
    N, mod, G = 701, 8192, 3000
    a, _ = rand(N, mod, G, 1, False)
    b, _ = rand(N, mod, G, 2, False)
    inter = np.stack([a, b], axis=1).reshape(2 * G, N)
    assert np.array_equal(eng.sum_groups(N, mod, inter, K=2), eng.add_batch(N, mod, a, b))


@pytest.mark.parametrize("N,q", [(821, 4096), (509, 2048)])
def test_tally_dev_is_sum_then_decrypt(eng, N, q):
    import torch
    g = np.random.default_rng(N)
    B, p = 4096, 3
    off = np.array([0, 16, 16, 1000, 1001, 4096], np.int64)
    G = off.size - 1
    rows, w = rand(N, q, B, 4, True)
    f, fp = g.integers(-1, 2, N).astype(np.int8), g.integers(0, 3, N).astype(np.uint8)
    d = Dev(eng)
    try:
        dr, dw, do, df, dfp = d.put(rows), d.put(w), d.put(off), d.put(f), d.put(fp)
        outs = [[d.empty((G, N), dt) for dt in (np.uint16, np.uint8, np.uint16, np.uint16, np.uint8)] for _ in range(3)]
        eng.sum_groups_dev(N, q, dr, outs[0][0], G, d_offsets=do, d_weights=dw)
        eng.decrypt_batch_dev(N, q, p, df, dfp, outs[0][0], G, outs[0][1], outs[0][2], outs[0][3], outs[0][4])
        s, v, q1, r1, q2 = outs[1]
        eng.tally_decrypt_batch_dev(N, q, p, df, dfp, dr, s, v, G, d_offsets=do, d_weights=dw, d_quot1=q1, d_rem1=r1, d_quot2=q2)
        eng.tally_decrypt_batch_dev(N, q, p, df, dfp, dr, outs[2][0], outs[2][1], G, d_offsets=do, d_weights=dw)      # value only
        dts = (np.uint16, np.uint8, np.uint16, np.uint16, np.uint8)
        ref_out = [eng.dev_download(x, (G, N), dt) for x, dt in zip(outs[0], dts)]
        got = [eng.dev_download(x, (G, N), dt) for x, dt in zip(outs[1], dts)]
        for a, b in zip(ref_out, got):
            assert a.tobytes() == b.tobytes()
        assert np.array_equal(ref_out[0], ref.np_sum(rows, q, offsets=off, weights=w))
        assert eng.dev_download(outs[2][1], (G, N), np.uint8).tobytes() == ref_out[1].tobytes()
        host = eng.tally_decrypt_batch(N, q, p, f, fp, rows, offsets=off, weights=w)
        for a, b in zip(ref_out, host):
            assert a.tobytes() == b.tobytes()
        with pytest.raises(pkg.EngineError) as ei:
            eng.tally_decrypt_batch_dev(N, q, p, df, dfp, dr, None, v, G, d_offsets=do, d_weights=dw)
        assert ei.value.code == 2 and "d_sum" in str(ei.value)
        # the _dev forms only enqueue: behind a long-running kernel on the same stream they return while it still runs
        eng.set_stream(torch.cuda.current_stream().cuda_stream)
        torch.cuda.synchronize()
        torch.cuda._sleep(200_000_000)
        eng.sum_groups_dev(N, q, dr, outs[2][0], G, d_offsets=do, d_weights=dw)
        eng.tally_decrypt_batch_dev(N, q, p, df, dfp, dr, s, v, G, d_offsets=do, d_weights=dw, d_quot1=q1, d_rem1=r1, d_quot2=q2)
        still_running = not torch.cuda.current_stream().query()
        torch.cuda.synchronize()
        assert still_running
    finally:
        eng.set_stream(None)
        d.free()


def test_host_form_refuses_bad_groups(eng):
    rows = np.zeros((8, 17), np.uint16)
    lib = pkg.load_library()
    import ctypes as C
    out = np.zeros((2, 17), np.uint16)
    ptr = lambda a: a.ctypes.data_as(C.c_void_p)
    for off in ([0, 5, 4], [-1, 2, 8]):
        o = np.array(off, np.int64)
        assert lib.ntru_sum_groups(eng._h, 17, 32, ptr(rows), None, ptr(o), 0, 2, ptr(out)) == 2
    w = np.full(8, 40, np.uint16)
    assert lib.ntru_sum_groups(eng._h, 17, 32, ptr(rows), ptr(w), None, 4, 2, ptr(out)) == 2 and b"weight" in lib.ntru_last_error()


def test_device_resident_tally_pipeline(eng):
    """Sample r on the device, encrypt 2^16 ternary plaintexts, tally in groups of 16, check the tallies' decrypt witnesses with the
    VerifyDecrypt kernel.  The share of tallies that decrypt to the sum of the plaintexts is reported, not asserted beyond > 0: it is a
    property of the scheme's noise."""
    import torch
    c = next(c for c in ref.load_cases() if c["set"] == "n509_q2048")
    o = c["options"]
    N, q, p, dr = o["N"], o["q"], o["p"], o["dr"]
    B, K = 1 << 16, 16
    G = B // K
    dev = torch.device("cuda:0")
    eng.set_stream(torch.cuda.current_stream().cuda_stream)
    try:
        up = lambda a: torch.from_numpy(a.view(np.int16) if a.dtype == np.uint16 else a).to(dev)
        h, f, fp = up(ref.pad(c["key"]["h"], N, np.uint16)), up(ref.pad(c["key"]["f"], N, np.int8)), up(ref.pad(c["key"]["fp"], N, np.uint8))
        d = lambda dt, shape: torch.empty(shape, dtype=dt, device=dev)
        r = d(torch.uint8, (B, N))
        eng.sample_ternary_dev(N, dr, dr, p - 1, np.arange(8, dtype=np.uint32), 0, B, r.data_ptr())
        m = torch.randint(0, 3, (B, N), generator=torch.Generator(device=dev).manual_seed(3), device=dev, dtype=torch.int32).to(torch.uint8)
        e = d(torch.int16, (B, N))
        eng.encrypt_batch_dev(N, q, h.data_ptr(), r.data_ptr(), m.data_ptr(), B, e.data_ptr())
        s, q1, r1 = d(torch.int16, (G, N)), d(torch.int16, (G, N)), d(torch.int16, (G, N))
        v, q2 = d(torch.uint8, (G, N)), d(torch.uint8, (G, N))
        eng.tally_decrypt_batch_dev(N, q, p, f.data_ptr(), fp.data_ptr(), e.data_ptr(), s.data_ptr(), v.data_ptr(), G, K=K,
                                    d_quot1=q1.data_ptr(), d_rem1=r1.data_ptr(), d_quot2=q2.data_ptr())
        torch.cuda.synchronize()
        ntru = pkg.NTRU(o)
        nq, np_ = ntru.calculateNq(), ntru.calculateNp()
        pad1 = lambda t: torch.nn.functional.pad(t.to(torch.int32), (0, 1)).to(torch.int16).contiguous()
        f16 = torch.where(f < 0, f.to(torch.int32) + q, f.to(torch.int32)).to(torch.int16).repeat(G, 1).contiguous()
        fp16 = fp.to(torch.int16).repeat(G, 1).contiguous()
        wit = [f16, fp16, s, pad1(q1), pad1(r1), pad1(q2), pad1(v)]
        flags = d(torch.uint8, (G,))
        eng.check_decrypt_batch_dev(N, q, nq, p, np_, *[t.data_ptr() for t in wit], G, flags.data_ptr())
        torch.cuda.synchronize()
        assert not flags.any().item()
        want = (m.view(G, K, N).to(torch.int32).sum(1) % p).to(torch.uint8)
        share = (v == want).all(1).float().mean().item()
        print("tallies of %d at N=%d q=%d: %.4f decrypt to the sum of the plaintexts" % (K, N, q, share))
        assert share > 0
    finally:
        eng.set_stream(None)
