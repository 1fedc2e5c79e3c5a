"""Sums, tallies and decrypts of ciphertexts that arrive as packOutput(q - 1, N, e) rows, on the GPU, byte for byte: against the
restatement (tests/packed_ref.py) and against the dense calls on the unpacked rows, at one shape per path of the kernel (packed_ref.SHAPES), with every bit set that a reader must ignore.
Every instantiation of the sum kernel, and its launches with many rows per block, are the variant table's (tests/kernel_variants.py); here
one tally rides on such a launch, and one decrypt takes more than one pass of unpacking."""
import ctypes as C
import json
import os

import numpy as np
import pytest

import __graft_entry__ as ge
import kernel_variants as kv
import packed_ref as ref
from oracle import ntru_oracle as orc

pytestmark = pytest.mark.gpu
pkg = ge.load_package()


@pytest.fixture(scope="module")
def eng():
    return pkg.Engine(0)


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


def rows_of(N, mod, bits, B, seed):
    """Random raw fields (for a modulus that is no power of two: values >= mod among them), packed, every ignored bit set."""
    g = np.random.default_rng(seed)
    rows = g.integers(0, 1 << bits, (B, N), dtype=np.uint16)
    rows[0, :] = (1 << bits) - 1
    packed = ref.set_ignored_bits(mod, N, ref.pack_rows(mod, rows))
    return g, rows, packed


def batch_of(N, mod):
    return 37 + (N * 7 + mod) % 564                    # between 37 and 600 rows, another count for every shape


@pytest.mark.parametrize("N,mod,bits,per,os_", ref.SHAPES)
def test_sums_equal_the_restatement_and_the_dense_sums(eng, N, mod, bits, per, os_):
    B = batch_of(N, mod)
    g, rows, packed = rows_of(N, mod, bits, B, N + mod)
    assert np.array_equal(ref.unpack_rows(mod, N, packed), rows) and not np.array_equal(packed, ref.pack_rows(mod, rows))
    pow2 = mod & (mod - 1) == 0
    # a modulus that is no power of two gets the largest weight on every row; the others random weights
    w = np.full(B, mod - 1, np.uint16) if not pow2 else g.integers(0, mod, B, dtype=np.uint16)
    cut = sorted(g.integers(3, B - 3, 6).tolist())
    forms = {                                          # name: (offsets or None, K, rows used)
        "K=1": (None, 1, B),
        "K=16": (None, 16, B - B % 16),
        "K=B": (None, B, B),
        "one CSR group": ([0, B], None, B),            # one group over every row block: the finish kernels complete it
        "CSR, empty groups first, in the middle and last": ([0, 0, 0, cut[0], cut[1], cut[1], cut[1], cut[2], cut[3], cut[4], B, B, B], None, B),
        "CSR not from row 0": ([cut[0], cut[1], cut[2], cut[2], cut[5]], None, B),
    }
    d = Dev(eng)
    try:
        d_packed, d_off8, d_w = d.put(packed), d.put(packed, shift=1), d.put(w)
        d_out = d.put(np.zeros((B, N), np.uint16))
        for name, (off, K, used) in forms.items():
            G = len(off) - 1 if off is not None else used // K
            d_off = None if off is None else d.put(np.asarray(off, np.int64))
            for weights, dw in ((None, None), (w, d_w)):
                tag = (name, weights is not None)
                want = ref.np_sum_packed(mod, N, packed[:used], offsets=off, K=K, weights=weights)
                dense = eng.sum_groups(N, mod, rows[:used], offsets=off, K=K, weights=None if weights is None else weights[:used])
                assert dense.tobytes() == want.tobytes(), tag
                for base, what in ((d_packed, "16-byte aligned"), (d_off8, "8 bytes off")):
                    eng.dev_upload(d_out, np.full((G, N), 0xABCD, np.uint16))
                    pkg.sum_groups_packed_dev(eng, N, mod, base, d_out, G, d_offsets=d_off, K=K, d_weights=dw)
                    assert eng.last_kernel() == "k_sum_groups_packed<%d,%d,%d>" % (bits, pow2, weights is not None)
                    assert eng.dev_download(d_out, (G, N), np.uint16).tobytes() == want.tobytes(), tag + (what,)
        # G = 0 launches nothing
        marker = np.full((2, N), 0x1234, np.uint16)
        eng.dev_upload(d_out, marker)
        eng.add_batch(2, 4, [[1, 1]], [[1, 1]])
        before = eng.last_kernel()
        pkg.sum_groups_packed_dev(eng, N, mod, d_packed, d_out, 0, K=4)
        pkg.sum_groups_packed_dev(eng, N, mod, d_packed, d_out, 0, d_offsets=d.put(np.zeros(1, np.int64)))
        assert eng.last_kernel() == before and np.array_equal(eng.dev_download(d_out, (2, N), np.uint16), marker)
        assert pkg.sum_groups_packed(eng, N, mod, packed[:0], offsets=[0]).shape == (0, N)
    finally:
        d.free()


@pytest.mark.parametrize("N,mod", [(167, 2048), (821, 4096)])
def test_host_form_equals_the_dev_form(eng, N, mod):
    bits = (mod - 1).bit_length()
    B = 8197                                           # ntru_chunk_items cuts 8197 rows into chunks of 2050
    g, rows, packed = rows_of(N, mod, bits, B, 3 * N)
    w = g.integers(0, mod, B, dtype=np.uint16)
    pinned = eng.pinned_empty(packed.shape, np.uint64)
    pinned[...] = packed
    off = np.array([0, 0, 5, 2049, 2050, 2051, 6000, 6000, B - 1], np.int64)
    d = Dev(eng)
    try:
        d_packed, d_w = d.put(packed), d.put(w)
        for offsets, K in ((None, B), (None, 1), (off, None)):      # one group over every chunk; a group per row; ragged, not to the end
            G = len(offsets) - 1 if offsets is not None else B // K
            d_out = d.put(np.zeros((G, N), np.uint16))
            d_off = None if offsets is None else d.put(offsets)
            for weights, dw in ((None, None), (w, d_w)):
                pkg.sum_groups_packed_dev(eng, N, mod, d_packed, d_out, G, d_offsets=d_off, K=K, d_weights=dw)
                dev = eng.dev_download(d_out, (G, N), np.uint16)
                assert dev.tobytes() == ref.np_sum_packed(mod, N, packed, offsets=offsets, K=K, weights=weights).tobytes()
                for src in (packed, pinned):
                    assert pkg.sum_groups_packed(eng, N, mod, src, offsets=offsets, K=K, weights=weights).tobytes() == dev.tobytes()
    finally:
        d.free()


def test_bad_arguments_get_the_codes_of_the_dense_sum(eng):
    """Every refusal of ntru_sum_groups, through both host entries: the same code and, but for the name, the same message."""
    lib = pkg.load_library()
    N, mod = 17, 32
    rows, packed = np.zeros((8, N), np.uint16), np.zeros((8, 3, 4), np.uint64)
    out = np.zeros((2, N), np.uint16)
    ptr = lambda a: None if a is None else a.ctypes.data_as(C.c_void_p)
    o = lambda *v: np.array(v, np.int64)
    big_w = np.full(8, mod, np.uint16)
    h = eng._h
    cases = [  # engine, N, mod, rows given, weights, offsets, K, G, out given
        (h, 1, mod, True, None, None, 4, 2, True), (h, 1921, mod, True, None, None, 4, 2, True), (h, N, 1, True, None, None, 4, 2, True),
        (h, N, 65537, True, None, None, 4, 2, True), (h, N, mod, True, None, None, 4, -1, True), (h, N, mod, True, None, None, 0, 2, True),
        (h, N, mod, True, None, None, 1 << 62, 4, True), (None, N, mod, True, None, None, 4, 2, True), (h, N, mod, True, None, None, 4, 2, False),
        (h, N, mod, True, None, o(-1, 2, 8), 0, 2, True), (h, N, mod, True, None, o(0, 5, 4), 0, 2, True),
        (h, N, mod, False, None, None, 4, 2, True), (h, N, mod, True, big_w, None, 4, 2, True), (h, N, mod, True, big_w, o(6, 7, 8), 0, 2, True),
    ]
    for e, n, m, has_rows, w, off, K, G, has_out in cases:
        got = []
        for fn, name, data in ((lib.ntru_sum_groups, b"ntru_sum_groups", rows), (lib.ntru_sum_groups_packed, b"ntru_sum_groups_packed", packed)):
            rc = fn(e, n, m, ptr(data) if has_rows else None, ptr(w), ptr(off), K, G, ptr(out) if has_out else None)
            got.append((rc, lib.ntru_last_error().replace(name + b":", b"<name>:")))
        assert got[0][0] == 2 and got[0] == got[1], (n, m, K, G, got)


def private_key(N, seed):
    g = np.random.default_rng(seed)
    return g.integers(-1, 2, N).astype(np.int8), g.integers(0, 3, N).astype(np.uint8)


@pytest.mark.parametrize("N,q,B", [(167, 2048, 70), (821, 4096, 97)])        # B = 97 at N = 821 is in the range of k_decrypt_m8
def test_decrypt_and_tally_equal_the_dense_calls(eng, N, q, B):
    p = 3
    g, rows, packed = rows_of(N, q, (q - 1).bit_length(), B, N)
    f, fp = private_key(N, B)
    assert np.array_equal(pkg.unpack_rows(eng, N, q, packed), rows)
    assert np.array_equal(pkg.pack_rows(eng, N, q, rows), ref.pack_rows(q, rows))
    want = eng.decrypt_batch(N, q, p, f, fp, rows)
    got = pkg.decrypt_packed_batch(eng, N, q, p, f, fp, packed)
    for a, b in zip(want, got):
        assert a.tobytes() == b.tobytes()
    lean = pkg.decrypt_packed_batch(eng, N, q, p, f, fp, packed, want_witness=False)
    assert lean[0].tobytes() == want[0].tobytes() and lean[1:] == (None, None, None)
    w = g.integers(0, q, B, dtype=np.uint16)
    off = np.array([0, 3, 3, 40, B - 1], np.int64)
    G = off.size - 1
    t_want = eng.tally_decrypt_batch(N, q, p, f, fp, rows, offsets=off, weights=w)
    t_got = pkg.tally_decrypt_packed_batch(eng, N, q, p, f, fp, packed, offsets=off, weights=w)
    for a, b in zip(t_want, t_got):
        assert a.tobytes() == b.tobytes()
    assert pkg.tally_decrypt_packed_batch(eng, N, q, p, f, fp, packed, offsets=off, weights=w, want_witness=False)[1].tobytes() \
        == t_want[1].tobytes()
    # the Python mirror of the reference's interface
    ntru = pkg.NTRU({"N": N, "q": q, "p": p, "f": f.tolist(), "fp": fp.tolist()}, engine=eng)
    assert ntru.decryptPackedBatch(packed)["quotient2"].tobytes() == want[3].tobytes()
    t = ntru.tallyPacked(packed, offsets=off, weights=w)
    assert t["sum"].tobytes() == t_want[0].tobytes() and t["value"].tobytes() == t_want[1].tobytes()
    # the _dev forms, with and without the witness arrays
    d = Dev(eng)
    try:
        dts = (np.uint8, np.uint16, np.uint16, np.uint8)
        d_f, d_fp, d_packed, d_w, d_off = d.put(f), d.put(fp), d.put(packed), d.put(w), d.put(off)
        outs = [d.put(np.zeros((B, N), dt)) for dt in dts]
        pkg.decrypt_packed_batch_dev(eng, N, q, p, d_f, d_fp, d_packed, B, *outs)
        for x, dt, a in zip(outs, dts, want):
            assert eng.dev_download(x, (B, N), dt).tobytes() == a.tobytes()
        only = d.put(np.zeros((B, N), np.uint8))
        pkg.decrypt_packed_batch_dev(eng, N, q, p, d_f, d_fp, d_packed, B, only)
        assert eng.dev_download(only, (B, N), np.uint8).tobytes() == want[0].tobytes()
        d_sum = d.put(np.zeros((G, N), np.uint16))
        pkg.tally_decrypt_packed_batch_dev(eng, N, q, p, d_f, d_fp, d_packed, d_sum, outs[0], G, d_offsets=d_off, d_weights=d_w,
                                           d_quot1=outs[1], d_rem1=outs[2], d_quot2=outs[3])
        for x, dt, a in zip([d_sum] + outs, (np.uint16,) + dts, t_want):
            assert eng.dev_download(x, (G, N), dt).tobytes() == a.tobytes()
        with pytest.raises(pkg.EngineError) as ei:
            pkg.tally_decrypt_packed_batch_dev(eng, N, q, p, d_f, d_fp, d_packed, None, outs[0], G, d_offsets=d_off)
        assert ei.value.code == 2 and "d_sum" in str(ei.value)
    finally:
        d.free()
    if (N, q) == (167, 2048):
        tally_with_many_rows_per_block(eng, N, q, p, f, fp)


def tally_with_many_rows_per_block(eng, N, q, p, f, fp):
    """One tally whose packed sum has row blocks of R > SP_BATCH side + side rows (kernel_variants.many_rows_per_block, sized from the
    CU count): the sums come out of the kernel's own loops and lane tree, not of k_sum_groups_finish on one-row partials."""
    import torch
    bits = (q - 1).bit_length()
    first, T, R, Pb, off = kv.many_rows_per_block(bits, N, torch.cuda.get_device_properties(0).multi_processor_count)
    side = kv.packed_layout(bits, N)["side"]
    assert side == 8 and -(-T // Pb) == R and R > kv.SP_BATCH * side + side, (T, Pb, R, side)
    B, G = first + T + 2, off.size - 1
    g, rows, packed = rows_of(N, q, bits, B, 5 * N)
    w = g.integers(0, q, B, dtype=np.uint16)
    t_want = eng.tally_decrypt_batch(N, q, p, f, fp, rows, offsets=off, weights=w)
    assert t_want[0].tobytes() == ref.np_sum_packed(q, N, packed, offsets=off, weights=w).tobytes()
    dts = (np.uint16, np.uint8, np.uint16, np.uint16, np.uint8)
    d = Dev(eng)
    try:
        outs = [d.put(np.zeros((G, N), dt)) for dt in dts]
        pkg.tally_decrypt_packed_batch_dev(eng, N, q, p, d.put(f), d.put(fp), d.put(packed), outs[0], outs[1], G, d_offsets=d.put(off),
                                           d_weights=d.put(w), d_quot1=outs[2], d_rem1=outs[3], d_quot2=outs[4])
        for x, dt, a in zip(outs, dts, t_want):
            assert eng.dev_download(x, (G, N), dt).tobytes() == a.tobytes()
    finally:
        d.free()


def test_decrypt_takes_more_than_one_pass(eng):
    """B = 65536 + 3: the rows are unpacked into scratch 65536 at a time, and the second pass reads and writes at offsets of its own.
    Every row and every output row differs from the one 65536 before it, so a pass at the wrong offset cannot match; guard rows
    behind every output stay as they were."""
    N, q, p, B, FILL = 17, 32, 3, 65536 + 3, 0xA5
    g, rows, packed = rows_of(N, q, 5, B, 65536)
    f, fp = private_key(N, 7)
    want = orc.decrypt_batch(N, q, p, f, fp, ref.unpack_rows(q, N, packed))
    for a in (rows,) + tuple(want):
        assert (a[65536:] != a[:3]).any(axis=1).all()
    dts = (np.uint8, np.uint16, np.uint16, np.uint8)
    d = Dev(eng)
    try:
        d_f, d_fp, d_packed = d.put(f), d.put(fp), d.put(packed)
        for witness in (True, False):
            outs = [d.put(np.full((B + 2, N), FILL, dt)) for dt in dts[:4 if witness else 1]]
            pkg.decrypt_packed_batch_dev(eng, N, q, p, d_f, d_fp, d_packed, B, *outs)
            for x, dt, a in zip(outs, dts, want):
                got = eng.dev_download(x, (B + 2, N), dt)
                assert got[:B].tobytes() == a.tobytes(), (witness, dt)
                assert got[B:].tobytes() == np.full((2, N), FILL, dt).tobytes(), (witness, dt)
    finally:
        d.free()
    for a, b in zip(want, pkg.decrypt_packed_batch(eng, N, q, p, f, fp, packed)):
        assert a.tobytes() == b.tobytes()


def test_the_loop_closes(eng):
    """What ntru_encrypt_pack_batch_dev writes (no dense e at all) goes straight into the packed decrypt and the packed sum."""
    with open(os.path.join(ge.ROOT, "tests", "golden", "scheme_n821_q4096.json")) as fh:
        gold = json.load(fh)
    o, key = gold["options"], gold["keys"][0]
    N, q, p, B, K = o["N"], o["q"], o["p"], 192, 16
    pad = lambda a, dt: np.array(list(a) + [0] * (N - len(a)), dtype=dt)
    h, f, fp = pad(key["h"], np.uint16), pad(key["f"], np.int8), pad(key["fp"], np.uint8)
    g = np.random.default_rng(11)
    r, m = g.integers(0, 3, (B, N), dtype=np.uint8), g.integers(0, 2, (B, N), dtype=np.uint8)
    e, _ = eng.encrypt_batch(N, q, h, r, m)
    want_value = eng.decrypt_batch(N, q, p, f, fp, e)[0]
    want_sum = eng.sum_groups(N, q, e, K=K)
    os_ = eng.pack_params(q - 1, N)["outputSize"]
    d = Dev(eng)
    try:
        d_packed = d.put(np.zeros((B, os_, 4), np.uint64))
        d_value, d_sum = d.put(np.zeros((B, N), np.uint8)), d.put(np.zeros((B // K, N), np.uint16))
        eng.encrypt_pack_batch_dev(N, q, d.put(h), d.put(r), d.put(m), B, None, d_packed)
        pkg.decrypt_packed_batch_dev(eng, N, q, p, d.put(f), d.put(fp), d_packed, B, d_value)
        pkg.sum_groups_packed_dev(eng, N, q, d_packed, d_sum, B // K, K=K)
        assert eng.last_kernel() == "k_sum_groups_packed<12,1,0>"
        assert eng.dev_download(d_packed, (B, os_, 4), np.uint64).tobytes() == ref.pack_rows(q, e).tobytes()
        assert eng.dev_download(d_value, (B, N), np.uint8).tobytes() == want_value.tobytes()
        assert eng.dev_download(d_sum, (B // K, N), np.uint16).tobytes() == want_sum.tobytes()
    finally:
        d.free()


def test_dev_forms_only_enqueue(eng):
    """Behind a long-running kernel on the same stream the _dev forms return while it still runs: no synchronisation, no allocation
    that waits for the device (the scratch buffer has its size from the calls above)."""
    import torch
    N, q, p, B, K = 167, 2048, 3, 70, 7
    _, rows, packed = rows_of(N, q, 11, B, 1)
    f, fp = private_key(N, 2)
    d = Dev(eng)
    try:
        d_f, d_fp, d_packed = d.put(f), d.put(fp), d.put(packed)
        d_sum, d_value = d.put(np.zeros((B, N), np.uint16)), d.put(np.zeros((B, N), np.uint8))
        calls = [lambda: pkg.sum_groups_packed_dev(eng, N, q, d_packed, d_sum, B // K, K=K),
                 lambda: pkg.tally_decrypt_packed_batch_dev(eng, N, q, p, d_f, d_fp, d_packed, d_sum, d_value, B // K, K=K),
                 lambda: pkg.decrypt_packed_batch_dev(eng, N, q, p, d_f, d_fp, d_packed, B, d_value)]
        for call in calls:
            call()                                     # (first use grows the scratch buffer)
        eng.set_stream(torch.cuda.current_stream().cuda_stream)
        torch.cuda.synchronize()
        torch.cuda._sleep(200_000_000)
        for call in calls:
            call()
        still_running = not torch.cuda.current_stream().query()
        torch.cuda.synchronize()
        assert still_running
        assert eng.dev_download(d_value, (B, N), np.uint8).tobytes() == eng.decrypt_batch(N, q, p, f, fp, rows)[0].tobytes()
    finally:
        eng.set_stream(None)
        d.free()
