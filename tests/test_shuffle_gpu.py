"""The mix order drawn on the GPU (csrc/permutation.hip), every comparison exact: the stable argsort against numpy's on the key sets that
take every path of the radix passes, on both sides of the tile and of the offsets round; the ChaCha20 permutation and a whole mix step
from a key against the restatement (tests/shuffle_ref.py) and against the engine's own re-encrypt.  Guard elements of a fixed pattern sit
before and behind every output."""
import functools

import numpy as np
import pytest

import __graft_entry__ as ge
import mix_ref
import shuffle_ref as ref

pytestmark = pytest.mark.gpu
pkg = ge.load_package()
U16, I64 = np.uint16, np.int64
KEY = [(i + 1) * 0x01010101 for i in range(8)]
KEY2 = [0x9E3779B9, 0, 0xFFFFFFFF, 7, 0x80000000, 1, 2, 3]
TILE = 1024                      # keys per tile of k_perm_hist / k_perm_scatter
ROUND = 256 * TILE               # keys behind one round of k_perm_offsets' loop: 2^18
GUARD = 32                       # guard elements on each side of an output (256 bytes of int64: the output keeps its alignment)


@pytest.fixture(scope="module")
def eng():
    e = pkg.Engine(0)
    yield e
    e.set_kernel_path(0)
    e.set_sampler_rounds(20)


class Dev:
    """Device copies of host arrays through the engine's own allocator (256-byte aligned), and guarded outputs."""

    def __init__(self, eng):
        self.eng, self.held = eng, []

    def put(self, a):
        a = np.ascontiguousarray(a)
        p = self.eng.dev_alloc(a.nbytes + 64)
        self.held.append(p)
        if a.nbytes:
            self.eng.dev_upload(p, a)
        return p

    def out(self, shape, dtype, shift=0):
        """(pointer, read): an output of `shape`, `shift` elements off the 256-byte boundary, with GUARD elements of a fixed pattern
        before and behind it; read() downloads it and checks the guards."""
        n, item = int(np.prod(shape)), np.dtype(dtype).itemsize
        fill = np.frombuffer(bytes([0xA5, 0x5A, 0xC3, 0x3C, 0x96, 0x69, 0xF0, 0x0F])[:item] * (n + 2 * GUARD + shift), dtype)
        base = self.put(fill)

        def read():
            got = self.eng.dev_download(base, (fill.size,), dtype)
            lo = GUARD + shift
            assert got[:lo].tobytes() == fill[:lo].tobytes() and got[lo + n:].tobytes() == fill[lo + n:].tobytes(), "guard overwritten"
            return got[lo:lo + n].reshape(shape)
        return base + (GUARD + shift) * item, read

    def free(self):
        self.eng.synchronize()
        for p in self.held:
            self.eng.dev_free(p)
        self.held = []


@pytest.fixture()
def dev(eng):
    d = Dev(eng)
    yield d
    d.free()


# ---- the sort -------------------------------------------------------------------------------------------------------------------------
def key_sets(B):
    g = np.random.default_rng(B + 1)
    i = np.arange(B, dtype=np.uint64)
    top = np.uint64(2**64 - 1)
    return {
        "random": g.integers(0, 2**64, B, dtype=np.uint64),
        "all equal": np.full(B, 0x0123456789ABCDEF, np.uint64),          # the identity: stability
        "ascending": i * np.uint64(0x10001),
        "descending": (np.uint64(B) - i) * np.uint64(0x100000001),
        "top byte": g.integers(0, 256, B, dtype=np.uint64) << np.uint64(56) | np.uint64(0x00A1B2C3D4E5F607),
        "bottom byte": g.integers(0, 256, B, dtype=np.uint64) | np.uint64(0x0FA1B2C3D4E5F600),
        "two values": np.where(i % np.uint64(2) == 0, np.uint64(0xFFFF0000FFFF0000), np.uint64(0x0000FFFF0000FFFF)),
        "0 and 2^64 - 1": np.where(g.integers(0, 2, B) == 1, top, np.uint64(0)),
    }


@pytest.mark.parametrize("B", [0, 1, 2, 63, 64, 65, 255, 256, 257, TILE - 1, TILE, TILE + 1, ROUND - 1, ROUND, ROUND + 1])
def test_argsort_equals_numpy_stable(eng, dev, B):
    for name, keys in key_sets(B).items():
        assert keys.dtype == np.uint64 and keys.shape == (B,)
        want = np.argsort(keys, kind="stable").astype(I64)
        if name == "all equal":
            assert np.array_equal(want, np.arange(B))
        d_keys = dev.put(keys)
        for shift in (0, 1):
            d_order, read = dev.out((B,), I64, shift)
            pkg.argsort_keys_dev(eng, d_keys, B, d_order)
            if B:
                assert eng.last_kernel() == "k_perm_finish"
            assert read().tobytes() == want.tobytes(), (name, B, shift)
        assert eng.dev_download(d_keys, (B,), np.uint64).tobytes() == keys.tobytes(), (name, B)
        dev.free()


# ---- the permutation ------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def want_perm(key, perm_id, B):
    return ref.permutation(list(key), perm_id, B)


PERM_IDS = [0, 1, 2**32, 2**64 - 1]


@pytest.mark.parametrize("B", [1, 7, 8, 9, 64, 1000, 65537])
def test_draw_equals_the_restatement(eng, dev, B):
    for perm_id in PERM_IDS:
        src, dst = want_perm(tuple(KEY), perm_id, B)
        d_src, read_src = dev.out((B,), I64)
        d_dst, read_dst = dev.out((B,), I64)
        pkg.draw_permutation_dev(eng, KEY, perm_id, B, d_src, d_dst)                 # with dst
        assert eng.last_kernel() == "k_perm_finish"
        assert read_src().tobytes() == src.tobytes() and read_dst().tobytes() == dst.tobytes(), (B, perm_id)
        d_src, read_src = dev.out((B,), I64)
        pkg.draw_permutation_dev(eng, KEY, perm_id, B, d_src)                        # without
        assert read_src().tobytes() == src.tobytes(), (B, perm_id)
        d_dst, read_dst = dev.out((B,), I64)
        pkg.draw_permutation_dev(eng, KEY, perm_id, B, None, d_dst)                  # dst only
        assert read_dst().tobytes() == dst.tobytes(), (B, perm_id)
        # the host form
        got = pkg.draw_permutation(eng, KEY, perm_id, B)
        assert got.dtype == I64 and got.tobytes() == src.tobytes(), (B, perm_id)
        got = pkg.draw_permutation(eng, KEY, perm_id, B, want_inverse=True)
        assert got[0].tobytes() == src.tobytes() and got[1].tobytes() == dst.tobytes(), (B, perm_id)
        dev.free()
    other = want_perm(tuple(KEY2), 5, B)[0]
    assert pkg.draw_permutation(eng, KEY2, 5, B).tobytes() == other.tobytes()
    assert pkg.draw_permutation(eng, KEY, 0, 0).shape == (0,)


def test_draw_ignores_sampler_rounds_and_kernel_path(eng):
    B = 1000
    src, dst = want_perm(tuple(KEY), 1, B)
    try:
        eng.set_sampler_rounds(8)
        got = pkg.draw_permutation(eng, KEY, 1, B, want_inverse=True)
        assert got[0].tobytes() == src.tobytes() and got[1].tobytes() == dst.tobytes()
        eng.set_sampler_rounds(20)
        for path in (0, 2):
            eng.set_kernel_path(path)
            assert pkg.draw_permutation(eng, KEY, 1, B).tobytes() == src.tobytes(), path
    finally:
        eng.set_sampler_rounds(20)
        eng.set_kernel_path(0)


# ---- a whole mix step -----------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def mix_case(N, q, n1, n2, B, first_item, perm_id):
    """(h, e_in, want): seeded inputs and the restatement's (e_out, quotE, r, src), computed once."""
    g = np.random.default_rng(N * 1000 + B)
    h, e_in = g.integers(0, q, N).astype(U16), g.integers(0, q, (B, N)).astype(U16)
    return h, e_in, ref.mix(N, q, 3, h, KEY, first_item, n1, n2, perm_id, e_in)


def run_mix_dev(eng, dev, N, q, h, e_in, n1, n2, first_item, perm_id, want_quot=True):
    B = e_in.shape[0]
    d_h, d_in = dev.put(h), dev.put(e_in)
    d_r, read_r = dev.out((B, N), np.uint8)
    d_src, read_src = dev.out((B,), I64)
    d_out, read_out = dev.out((B, N), U16)
    d_quot, read_quot = dev.out((B, N), U16) if want_quot else (None, None)
    pkg.mix_batch_dev(eng, N, q, 3, d_h, KEY, first_item, n1, n2, perm_id, d_in, B, d_r, d_src, d_out, d_quotE=d_quot)
    assert eng.dev_download(d_in, (B, N), U16).tobytes() == e_in.tobytes()
    return read_out(), read_quot() if want_quot else None, read_r(), read_src()


# N, q, (n1, n2), the batch sizes, the kernel paths
MIX_SHAPES = [(17, 32, (3, 2), (1, 5, 97), (0, 2, 4)), (167, 128, (5, 4), (1, 5, 97), (0, 2, 4)), (821, 4096, (30, 29), (97, 300), (0, 4))]


@pytest.mark.parametrize("N,q,n,sizes,paths", MIX_SHAPES)
def test_mix_equals_the_restatement(eng, dev, N, q, n, sizes, paths):
    try:
        for B in sizes:
            for first_item, perm_id in ((0, 0), (2**33 + 5, 2**64 - 1)):
                h, e_in, want = mix_case(N, q, n[0], n[1], B, first_item, perm_id)
                w_e, w_q, w_r, w_src = want
                for path in paths:
                    eng.set_kernel_path(path)
                    got = run_mix_dev(eng, dev, N, q, h, e_in, n[0], n[1], first_item, perm_id)
                    for a, b, what in zip(got, want, ("e_out", "quotE", "r", "src")):
                        assert a.tobytes() == b.tobytes(), (what, N, q, B, first_item, path)
                    # the engine's own re-encrypt fed that r and src
                    own = pkg.reencrypt_batch(eng, N, q, h, got[2], e_in, src=got[3])
                    assert own[0].tobytes() == got[0].tobytes() and own[1].tobytes() == got[1].tobytes(), (N, q, B, path)
                    # the host form, everything asked for
                    host = pkg.mix_batch(eng, N, q, 3, h, KEY, first_item, n[0], n[1], perm_id, e_in)
                    for a, b, what in zip(host, want, ("e_out", "quotE", "r", "src")):
                        assert a.dtype == b.dtype and a.tobytes() == b.tobytes(), ("host", what, N, q, B, first_item, path)
                    dev.free()
                # quotE NULL; r_out, src_out and quotE NULL in the host form
                eng.set_kernel_path(paths[0])
                got = run_mix_dev(eng, dev, N, q, h, e_in, n[0], n[1], first_item, perm_id, want_quot=False)
                assert got[0].tobytes() == w_e.tobytes() and got[2].tobytes() == w_r.tobytes() and got[3].tobytes() == w_src.tobytes()
                host = pkg.mix_batch(eng, N, q, 3, h, KEY, first_item, n[0], n[1], perm_id, e_in, want_r=False, want_src=False, want_quot=False)
                assert host[0].tobytes() == w_e.tobytes() and host[1:] == (None, None, None)
                host = pkg.mix_batch(eng, N, q, 3, h, KEY, first_item, n[0], n[1], perm_id, e_in, want_r=False)
                assert host[0].tobytes() == w_e.tobytes() and host[1].tobytes() == w_q.tobytes() and host[2] is None
                assert host[3].tobytes() == w_src.tobytes()
                dev.free()
    finally:
        eng.set_kernel_path(0)


def test_mix_honours_the_sampler_rounds_and_keeps_the_order(eng, dev):
    """r follows ntru_engine_set_sampler_rounds, the permutation does not."""
    from oracle import ntru_oracle as orc
    N, q, B = 167, 128, 33
    h, e_in, want = mix_case(N, q, 5, 4, B, 9, 4)
    try:
        eng.set_sampler_rounds(8)
        got = run_mix_dev(eng, dev, N, q, h, e_in, 5, 4, 9, 4)
    finally:
        eng.set_sampler_rounds(20)
    r8 = orc.sample_ternary_batch(N, 5, 4, 2, KEY, 9, B, rounds=8)
    assert got[2].tobytes() == r8.tobytes() and got[2].tobytes() != want[2].tobytes()
    assert got[3].tobytes() == want[3].tobytes()
    e8, q8 = mix_ref.reencrypt(N, q, h, r8, e_in, want[3])
    assert got[0].tobytes() == e8.tobytes() and got[1].tobytes() == q8.tobytes()


def test_mix_witness_satisfies_verify_encrypt(eng, dev):
    N, q, B = 167, 128, 97
    h, e_in, _ = mix_case(N, q, 5, 4, B, 0, 0)
    e_out, quot, r, src = run_mix_dev(eng, dev, N, q, h, e_in, 5, 4, 0, 0)
    nq = pkg.NTRU({"N": N, "q": q}).calculateNq()
    pad = lambda x: np.concatenate([x.astype(U16), np.zeros((B, 1), U16)], axis=1)
    flags = eng.check_encrypt_batch(N, q, nq, r.astype(U16), e_in[src], np.tile(h, (B, 1)), pad(quot), pad(e_out))
    assert flags.shape == (B,) and not flags.any()
    bad = e_in[src].copy()
    bad[3, 0] ^= 1                                                     # the check does look at m
    assert eng.check_encrypt_batch(N, q, nq, r.astype(U16), bad, np.tile(h, (B, 1)), pad(quot), pad(e_out))[3] != 0


def test_ntru_mix_batch_returns_the_same_arrays(eng):
    N, q, B = 167, 128, 97
    h, e_in, want = mix_case(N, q, 5, 5, B, 2**33 + 5, 1)
    ntru = pkg.NTRU({"N": N, "q": q, "p": 3, "dr": 5, "h": h.tolist()}, engine=eng)
    got = ntru.mixBatch(e_in, KEY, firstItem=2**33 + 5, permId=1)
    assert list(got) == ["value", "r", "m", "src", "quotientE"]
    assert got["value"].tobytes() == want[0].tobytes() and got["quotientE"].tobytes() == want[1].tobytes()
    assert got["r"].tobytes() == want[2].tobytes() and got["src"].tobytes() == want[3].tobytes()
    assert got["m"].dtype == U16 and got["m"].tobytes() == e_in[want[3]].tobytes()
    assert ntru.mixBatch(e_in, KEY, firstItem=2**33 + 5, permId=1, wantWitness=False)["quotientE"] is None


def test_fixture_plaintexts_come_back_in_the_drawn_order(eng):
    """The keys and ciphertexts of tests/golden/mix_cases.json, a set the fixture records as recovering: one mixBatch, then decryptBits
    returns the plaintexts in the order src gives."""
    c = [c for c in mix_ref.load_cases() if c["mustRecover"]][1]
    o = c["options"]
    N = o["N"]
    assert (N, o["q"]) == (167, 128)
    key = {k: c["key"][k].tolist() for k in ("h", "f", "fp")}
    ntru = pkg.NTRU({**o, **key}, engine=eng)
    mixed = ntru.mixBatch(c["e"], KEY, permId=3)
    src = mixed["src"]
    assert sorted(src.tolist()) == list(range(6)) and src.tolist() != list(range(6))
    assert src.tobytes() == ref.permutation(KEY, 3, 6)[0].tobytes()
    for i in range(6):
        value = ntru.decryptBits(mixed["value"][i].tolist())["value"]
        assert pkg.expandArray(value, N) == c["m"][src[i]].tolist(), i


# ---- refusals with a live engine ------------------------------------------------------------------------------------------------------
def test_bad_arguments_launch_nothing(eng, dev):
    lib = pkg.load_library()
    eng.add_batch(2, 4, [[1, 1]], [[1, 1]])
    before = eng.last_kernel()
    d_keys = dev.put(np.arange(8, dtype=np.uint64))
    d_order, read = dev.out((8,), I64)
    assert lib.ntru_argsort_keys_dev(eng._h, d_keys, 0, d_order) == 0
    assert lib.ntru_argsort_keys_dev(eng._h, d_keys, (1 << 24) + 1, d_order) == 2
    assert lib.ntru_argsort_keys_dev(eng._h, d_order, 8, d_order + 56) == 2 and b"overlap" in lib.ntru_last_error()
    with pytest.raises(pkg.EngineError, match="key is NULL|both NULL"):
        pkg.draw_permutation_dev(eng, KEY, 0, 8, None, None)
    N, q = 17, 32
    d_h, d_in = dev.put(np.ones(N, U16)), dev.put(np.ones((8, N), U16))
    d_r, read_r = dev.out((8, N), np.uint8)
    with pytest.raises(pkg.EngineError, match="overlap"):
        pkg.mix_batch_dev(eng, N, q, 3, d_h, KEY, 0, 2, 2, 0, d_in, 8, d_r, d_order, d_in)
    with pytest.raises(pkg.EngineError, match="cannot exceed"):
        pkg.mix_batch_dev(eng, N, q, 3, d_h, KEY, 0, 9, 9, 0, d_in, 8, d_r, d_order, d_keys)
    with pytest.raises(pkg.EngineError, match="unsupported"):
        pkg.mix_batch(eng, N, 33, 3, np.ones(N, U16), KEY, 0, 2, 2, 0, np.ones((8, N), U16))
    pkg.mix_batch_dev(eng, N, q, 3, d_h, KEY, 0, 2, 2, 0, d_in, 0, d_r, d_order, d_keys)          # B = 0: nothing launched
    assert eng.last_kernel() == before
    read(), read_r()
