"""Re-randomising and shuffling ciphertexts on the GPU (ntru_reencrypt_batch, csrc/matrix_reencrypt.hip), byte for byte: the fixture of
the unmodified reference through the three interfaces, every shape that takes another path against the restatement (tests/mix_ref.py),
the persistent loop against the composition it replaces, the refusals, and the indices the _dev form must not follow."""
import ctypes as C

import numpy as np
import pytest

import __graft_entry__ as ge
import mix_ref as ref

pytestmark = pytest.mark.gpu
pkg = ge.load_package()
U16 = np.uint16


@pytest.fixture(scope="module")
def eng():
    e = pkg.Engine(0)
    yield e
    e.set_kernel_path(0)


@pytest.fixture(scope="module")
def cases():
    return ref.load_cases()


class Dev:
    """Device copies of host arrays through the engine's own allocator (256-byte aligned); `shift` elements off that boundary."""

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

    def free(self):
        self.eng.synchronize()
        for p in self.held:
            self.eng.dev_free(p)
        self.held = []


def run_dev(eng, d, N, q, h, r, e_in, src, want_quot=True, shifts=(0, 0, 0), in_place=False):
    """One _dev call on fresh device copies; shifts: byte offset of d_r, element offsets of d_e_in and d_e_out.  Returns (e_out, quotE)
    with a guard row behind each checked."""
    B, B_in = r.shape[0], e_in.shape[0]
    d_h, d_r, d_in = d.put(h.astype(U16)), d.put(r.astype(np.uint8), shifts[0]), d.put(e_in.astype(U16), shifts[1])
    d_src = None if src is None else d.put(np.asarray(src, np.int64))
    guard = np.full((1, N), 0xABCD, U16)
    if in_place:
        d_out = d_in
    else:
        d_out = d.put(np.concatenate([np.full((B, N), 0x5A5A, U16), guard]), shifts[2])
    d_quot = d.put(np.concatenate([np.full((B, N), 0x5A5A, U16), guard])) if want_quot else None
    pkg.reencrypt_batch_dev(eng, N, q, d_h, d_r, d_in, B_in, d_out, B, d_src=d_src, d_quotE=d_quot)
    if in_place:
        got = eng.dev_download(d_out, (B_in, N), U16)
        assert got[B:].tobytes() == e_in[B:].astype(U16).tobytes()          # rows past B are left alone
        out = got[:B]
    else:
        got = eng.dev_download(d_out, (B + 1, N), U16)
        assert got[B:].tobytes() == guard.tobytes()
        out = got[:B]
    quot = None
    if want_quot:
        gq = eng.dev_download(d_quot, (B + 1, N), U16)
        assert gq[B:].tobytes() == guard.tobytes()
        quot = gq[:B]
    return out, quot


# ---- the fixture ----------------------------------------------------------------------------------------------------------------------
def test_fixture_through_every_interface(eng, cases):
    eng.set_kernel_path(0)
    for c in cases:
        o = c["options"]
        N, q, p = o["N"], o["q"], o["p"]
        h, f, fp = c["key"]["h"].astype(U16), c["key"]["f"].astype(np.int8), c["key"]["fp"].astype(np.uint8)
        ntru = pkg.NTRU({**o, "h": h.tolist(), "f": f.tolist(), "fp": fp.tolist()}, engine=eng)
        nq = ntru.calculateNq()
        cur, plain = c["e"], c["m"]
        d = Dev(eng)
        try:
            for rd in c["rounds"]:
                src, r, B = rd["src"], rd["r"], len(rd["src"])
                want_e, want_q = rd["remainder"].astype(U16), rd["quotient"].astype(U16)
                a = pkg.mix.reencrypt_batch(eng, N, q, h, r, cur, src=src)
                b = ntru.reencryptBatch(cur, r=r, src=src)
                cdev = run_dev(eng, d, N, q, h, r, cur, src)
                for got_e, got_q in (a, (b["value"], b["quotientE"]), cdev):
                    assert got_e.tobytes() == want_e.tobytes() and got_q.tobytes() == want_q.tobytes(), c["set"]
                assert b["m"].tobytes() == cur[src].astype(U16).tobytes()
                assert pkg.mix.reencrypt_batch(eng, N, q, h, r, cur, src=src, want_quot=False)[1] is None
                value = eng.decrypt_batch(N, q, p, f, fp, want_e, want_witness=False)[0]
                assert value.tobytes() == rd["value"].astype(np.uint8).tobytes(), c["set"]
                plain = plain[src]
                assert np.array_equal((value == plain).all(axis=1), rd["recovered"].astype(bool)), c["set"]
                pad = lambda x: np.concatenate([x.astype(U16), np.zeros((B, 1), U16)], axis=1)
                flags = eng.check_encrypt_batch(N, q, nq, r.astype(U16), b["m"], np.tile(h, (B, 1)), pad(want_q), pad(want_e))
                assert not flags.any(), c["set"]
                cur = rd["remainder"]
            drawn = ntru.reencryptBatch(cur)                     # r drawn as encryptBits draws it
            assert drawn["r"].shape == (9, N) and ((drawn["r"] == 1).sum(axis=1) == o["dr"]).all()
            assert ((drawn["r"] == p - 1).sum(axis=1) == o["dr"]).all()
            e2, q2 = ref.reencrypt(N, q, h, drawn["r"], cur)
            assert drawn["value"].tobytes() == e2.tobytes() and drawn["quotientE"].tobytes() == q2.tobytes()
        finally:
            d.free()


# ---- shapes ---------------------------------------------------------------------------------------------------------------------------
# N, q, kernel path, the kernel a dword-aligned call must report
SHAPES = [(17, 32, 4, "k_reencrypt_m"), (64, 64, 0, "k_reencrypt_md"), (167, 128, 0, "k_reencrypt_md"), (509, 2048, 0, "k_reencrypt_md"),
          (701, 8192, 0, "k_reencrypt_md"), (821, 4096, 0, "k_reencrypt_md"), (1022, 8192, 0, "k_reencrypt_m"),
          (1024, 8192, 0, None), (167, 65536, 0, "k_add_gathered_rows"), (1100, 2048, 0, "k_add_gathered_rows")]


@pytest.mark.parametrize("N,q,path,kernel", SHAPES)
def test_shapes_equal_the_restatement(eng, N, q, path, kernel):
    g = np.random.default_rng(N * 31 + q)
    eng.set_kernel_path(path)
    h = g.integers(0, q, N)
    d = Dev(eng)

    def check(r, e_in, src, **kw):
        want_e, want_q = ref.reencrypt(N, q, kw.pop("h", h), r, e_in, src)
        got_e, got_q = run_dev(eng, d, N, q, kw.pop("h_dev", h), r, e_in, src, **kw)
        assert got_e.tobytes() == want_e.tobytes(), (N, q, r.shape[0], kw)
        if got_q is not None:
            assert got_q.tobytes() == want_q.tobytes(), (N, q, r.shape[0], kw)

    try:
        for B in (1, 31, 32, 33, 97):
            r, e_in = g.integers(0, 3, (B, N)), g.integers(0, 65536, (B + 2, N))
            check(r, e_in, None)                                                   # src == NULL, B < B_in
            if kernel and B == 97:
                assert eng.last_kernel() == kernel
            check(r, e_in[:B], g.permutation(B), want_quot=B % 2 == 0)              # a permutation
            check(r, e_in, None, in_place=True, want_quot=B % 2 == 1)              # in place
            check(r, e_in, g.integers(0, B + 2, B), shifts=(1 + B % 3, 1, 1))      # r off the dword, e_in and e_out at odd elements
        if N == 1024:                                                              # rows too long for the one-instruction DMA
            assert eng.last_kernel() == "k_reencrypt_m"
        # a gather with repeats (5 -> 70) and a shrink (70 -> 3)
        check(g.integers(0, 3, (70, N)), g.integers(0, q, (5, N)), g.integers(0, 5, 70))
        check(g.integers(0, 3, (3, N)), g.integers(0, q, (70, N)), np.array([69, 0, 33]), want_quot=False)
        # the extremes: the largest accumulators, then the largest addend
        B = 33
        top = np.full(N, q - 1)
        check(np.full((B, N), 2), np.full((B, N), q - 1), None, h=top, h_dev=top)
        check(np.full((B, N), 2), np.full((B, N), 65535), g.permutation(B), h=top, h_dev=top)
        check(g.integers(0, 3, (B, N)), np.full((B, N), 65535), None, shifts=(3, 1, 0))
    finally:
        eng.set_kernel_path(0)
        d.free()


def test_kernel_paths_agree(eng):
    """Paths 0, 4, 5 (matrix cores: k_reencrypt_md / _m) and 1 (vector ALUs + the add kernel) write the same bytes."""
    N, q, B = 167, 128, 97
    g = np.random.default_rng(5)
    h, r, e_in, src = g.integers(0, q, N), g.integers(0, 3, (B, N)), g.integers(0, 65536, (40, N)), g.integers(0, 40, B)
    want = ref.reencrypt(N, q, h, r, e_in, src)
    d = Dev(eng)
    try:
        for path, kernel in ((0, "k_reencrypt_md"), (4, "k_reencrypt_m"), (5, "k_reencrypt_md"), (1, "k_add_gathered_rows")):
            eng.set_kernel_path(path)
            got = run_dev(eng, d, N, q, h, r, e_in, src)
            assert eng.last_kernel() == kernel
            assert got[0].tobytes() == want[0].tobytes() and got[1].tobytes() == want[1].tobytes(), path
            host = pkg.mix.reencrypt_batch(eng, N, q, h, r, e_in, src=src)
            assert host[0].tobytes() == want[0].tobytes() and host[1].tobytes() == want[1].tobytes(), path
    finally:
        eng.set_kernel_path(0)
        d.free()


# ---- the persistent loop --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("N,q", [(167, 128), (821, 4096)])
def test_persistent_loop_equals_the_composition(eng, N, q):
    """B = 32805: more than two passes of the 512 resident workgroups (16384 rows each), so the prefetch of the next row block's r rows
    runs.  The whole batch against encrypt (zero m) + gather + add, 128 strided rows against the restatement."""
    import torch
    eng.set_kernel_path(0)
    B = 32805
    g = np.random.default_rng(N)
    h = g.integers(0, q, N).astype(U16)
    r = g.integers(0, 3, (B, N), dtype=np.uint8)
    e_in = g.integers(0, q, (B, N), dtype=U16)
    src = g.permutation(B).astype(np.int64)
    per_pass = 32 * 2 * torch.cuda.get_device_properties(0).multi_processor_count
    d = Dev(eng)
    try:
        d_h, d_r, d_in, d_src = d.put(h), d.put(r), d.put(e_in), d.put(src)
        d_out, d_quot = d.put(np.zeros((B, N), U16)), d.put(np.zeros((B, N), U16))
        pkg.reencrypt_batch_dev(eng, N, q, d_h, d_r, d_in, B, d_out, B, d_src=d_src, d_quotE=d_quot)
        assert eng.last_kernel() == "k_reencrypt_md"
        got_e, got_q = eng.dev_download(d_out, (B, N), U16), eng.dev_download(d_quot, (B, N), U16)
        # the composition
        d_zero, d_gathered = d.put(np.zeros((B, N), np.uint8)), d.put(e_in[src])
        d_e0, d_q0, d_sum = d.put(np.zeros((B, N), U16)), d.put(np.zeros((B, N), U16)), d.put(np.zeros((B, N), U16))
        eng.encrypt_batch_dev(N, q, d_h, d_r, d_zero, B, d_e0, d_q0)
        eng.add_batch_dev(N, q, d_e0, d_gathered, B, d_sum)
        assert got_e.tobytes() == eng.dev_download(d_sum, (B, N), U16).tobytes()
        assert got_q.tobytes() == eng.dev_download(d_q0, (B, N), U16).tobytes()
    finally:
        d.free()
    edges = {0, B - 1, 32767, 32768, 32799, 32800}                             # the first and last row of every pass, the partial block
    for edge in range(per_pass, B, per_pass):
        edges |= {edge - 1, edge}
    strided = [x for x in range(7, B, 271) if x not in edges]
    rows = np.array(sorted(edges) + strided[:128 - len(edges)])
    assert rows.size == 128
    want_e, want_q = ref.reencrypt(N, q, h, r[rows], e_in, src[rows])
    assert got_e[rows].tobytes() == want_e.tobytes() and got_q[rows].tobytes() == want_q.tobytes()


# ---- refusals -------------------------------------------------------------------------------------------------------------------------
def test_bad_arguments_launch_nothing(eng):
    lib = pkg.load_library()
    N, q = 17, 32
    ptr = lambda a: None if a is None else a.ctypes.data_as(C.c_void_p)
    h, r = np.ones(N, U16), np.ones((4, N), np.uint8)
    e_in, e_out = np.full((4, N), 7, U16), np.full((6, N), 0x1234, U16)
    eng.add_batch(2, 4, [[1, 1]], [[1, 1]])
    before = eng.last_kernel()
    for src in ([0, 1, 4, 2], [0, -1, 1, 2]):                                   # the host form checks every index
        s = np.array(src, np.int64)
        assert lib.ntru_reencrypt_batch(eng._h, N, q, ptr(h), ptr(r), ptr(e_in), 4, ptr(s), 4, ptr(e_out), None) == 2
        assert b"outside" in lib.ntru_last_error()
    r6 = np.ones((6, N), np.uint8)
    assert lib.ntru_reencrypt_batch(eng._h, N, q, ptr(h), ptr(r6), ptr(e_in), 4, None, 6, ptr(e_out), None) == 2          # B > B_in
    assert lib.ntru_reencrypt_batch(eng._h, N, q, ptr(h), ptr(r), ptr(e_in), -1, None, 0, ptr(e_out), None) == 2
    assert lib.ntru_reencrypt_batch(eng._h, N, q, ptr(h), ptr(r), ptr(e_in), 4, None, -1, ptr(e_out), None) == 2
    assert lib.ntru_reencrypt_batch(eng._h, N, q, ptr(h), ptr(r), None, 4, None, 4, ptr(e_out), None) == 2                 # NULL buffer
    s = np.arange(4, dtype=np.int64)
    both = np.zeros((8, N), U16)
    for out in (both, both[2:]):                                                # overlapping ranges with src
        assert lib.ntru_reencrypt_batch(eng._h, N, q, ptr(h), ptr(r), ptr(both), 4, ptr(s), 4, ptr(out), None) == 2
        assert b"overlap" in lib.ntru_last_error()
    d = Dev(eng)
    try:
        d_h, d_r, d_buf, d_src = d.put(h), d.put(r6), d.put(np.full((12, N), 0x1234, U16)), d.put(s)
        call = lambda d_in, B_in, d_s, B, d_out: lib.ntru_reencrypt_batch_dev(eng._h, N, q, d_h, d_r, d_in, B_in, d_s, B, d_out, None)
        assert call(d_buf, 4, None, 6, d_buf + 6 * N * 2) == 2                  # B > B_in without src
        assert call(d_buf, 4, d_src, 4, d_buf) == 2                             # in place with src
        assert call(d_buf, 4, d_src, 4, d_buf + 3 * N * 2) == 2                 # partial overlap with src
        assert call(d_buf, 4, None, 4, d_buf + N * 2) == 2                      # shifted overlap without src
        assert call(d_buf, 4, None, 4, None) == 2
        assert call(d_buf, 4, None, 0, d_buf + 6 * N * 2) == 0                  # B = 0 is fine
        assert call(None, 0, d_src, 0, None) == 0
        assert eng.last_kernel() == before
        assert eng.dev_download(d_buf, (12, N), U16).tobytes() == np.full((12, N), 0x1234, U16).tobytes()
    finally:
        d.free()
    assert e_out.tobytes() == np.full((6, N), 0x1234, U16).tobytes()
    out, quot = pkg.mix.reencrypt_batch(eng, N, q, h, r[:0], e_in)              # B = 0 through the binding
    assert out.shape == (0, N)
    with pytest.raises(ValueError):
        pkg.NTRU({"N": N, "q": q, "h": [1]}, engine=eng).reencryptBatch(e_in, src=[4])


# ---- indices the _dev form must not follow ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("N,q,path", [(167, 128, 0), (167, 128, 4), (821, 4096, 0), (167, 65536, 0)])
def test_out_of_range_index_adds_nothing(eng, N, q, path):
    """d_e_in points inside a larger allocation, with a sentinel row before and after it: rows whose index is -1 or B_in equal Enc(0; r)
    -- the sentinels are not read -- and the others are unaffected."""
    g = np.random.default_rng(q + N)
    B_in, B = 5, 40
    h, r = g.integers(0, q, N), g.integers(0, 3, (B, N))
    buf = g.integers(0, q, (B_in + 2, N))
    buf[0], buf[-1] = q // 2 + 1, q // 2 + 3                                     # the sentinels: nonzero mod q
    src = g.integers(0, B_in, B)
    src[[0, 7, 31, 32, 39]] = [-1, B_in, -1, B_in, 1 << 40]
    bad = (src < 0) | (src >= B_in)
    want_e, want_q = ref.reencrypt(N, q, h, r, buf[1:-1], src)
    zero_e, _ = ref.reencrypt(N, q, h, r, np.zeros((B, N), np.int64))
    assert want_e[bad].tobytes() == zero_e[bad].tobytes() and (want_e[~bad] != zero_e[~bad]).any()
    eng.set_kernel_path(path)
    d = Dev(eng)
    try:
        d_buf, d_out, d_quot = d.put(buf.astype(U16)), d.put(np.zeros((B, N), U16)), d.put(np.zeros((B, N), U16))
        pkg.reencrypt_batch_dev(eng, N, q, d.put(h.astype(U16)), d.put(r.astype(np.uint8)), d_buf + N * 2, B_in, d_out, B,
                                d_src=d.put(src.astype(np.int64)), d_quotE=d_quot)
        assert eng.dev_download(d_out, (B, N), U16).tobytes() == want_e.tobytes()
        assert eng.dev_download(d_quot, (B, N), U16).tobytes() == want_q.tobytes()
    finally:
        eng.set_kernel_path(0)
        d.free()
