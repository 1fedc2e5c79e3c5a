"""Byte messages as packed bits on the GPU: k_bytes_to_rows / k_rows_to_bytes against the numpy restatement (tests/message_bytes_ref.py)
across row lengths, block sizes, batch sizes and byte alignments; the byte forms of encrypt, decrypt and the pipeline against the
existing calls on expanded rows; the reference-captured blocks; the refusals."""
import ctypes as C
import json
import os

import numpy as np
import pytest

import __graft_entry__ as ge
import message_bytes_ref as ref

pytestmark = pytest.mark.gpu
pkg = ge.load_package()

NS = [8, 17, 167, 509, 821, 1024, 1920]
BS = [1, 3, 257, 4099]
SHIFTS = [(0, 0, 0), (1, 7, 1), (7, 1, 7)]          # byte offsets of (input, output, flags) into their allocations
FILL = 0xAA


def block_sizes(N):
    W = N // 8
    return sorted({1, max(W - 1, 1), W})


@pytest.fixture(scope="module")
def eng():
    e = pkg.Engine(0)
    yield e
    e.set_kernel_path(0)


@pytest.fixture(scope="module")
def sets():
    return ref.load_sets()


@pytest.fixture(scope="module")
def keys(sets):
    """name -> (N, q, p, W, h, f, fp, dr): the fixture's four keys and the N = 821, q = 4096 key of the scheme fixture."""
    out = {s["set"]: ref.set_key(s) + (s["options"]["dr"],) for s in sets}
    with open(os.path.join(ge.ROOT, "tests", "golden", "scheme_n821_q4096.json")) as fh:
        gold = json.load(fh)
    o, k = gold["options"], gold["keys"][0]
    N = o["N"]
    out["n821_q4096"] = (N, o["q"], o["p"], N // 8, ref.pad(k["h"], N, np.uint16), ref.pad(k["f"], N, np.int8), ref.pad(k["fp"], N, np.uint8),
                         o["dr"])
    return out


class Dev:
    """Device buffers through the engine's own allocator, `shift` BYTES off the allocation's start, with `guard` bytes of FILL around."""

    def __init__(self, eng):
        self.eng, self.held = eng, []

    def put(self, a, shift=0):
        a = np.ascontiguousarray(a)
        p = self.eng.dev_alloc(a.nbytes + shift + 64)
        self.held.append(p)
        if a.nbytes:
            self.eng.dev_upload(p + shift, a)
        return p + shift

    def filled(self, nbytes, shift=0):
        """nbytes of FILL with 16 guard bytes of FILL on either side; returns the pointer to the payload."""
        return self.put(np.full(nbytes + 32, FILL, np.uint8), shift) + 16

    def get_guarded(self, p, nbytes):
        """(payload, guards untouched?)"""
        raw = self.eng.dev_download(p - 16, (nbytes + 32,), np.uint8)
        return raw[16:16 + nbytes], bool((raw[:16] == FILL).all() and (raw[16 + nbytes:] == FILL).all())

    def free(self):
        self.eng.synchronize()
        for p in self.held:
            self.eng.dev_free(p)
        self.held = []


def host_view(nbytes, shift):
    """A uint8 view of nbytes, `shift` bytes into a FILL-ed allocation with 16 guard bytes on either side: (raw, view)."""
    raw = np.full(nbytes + 32 + shift, FILL, np.uint8)
    return raw, raw[16 + shift:16 + shift + nbytes]


def guards_ok(raw, nbytes, shift):
    return bool((raw[:16 + shift] == FILL).all() and (raw[16 + shift + nbytes:] == FILL).all())


def vp(a):
    return a.ctypes.data_as(C.c_void_p)


def rand_r(g, B, N, dr):
    r = np.zeros((B, N), np.uint8)
    r[:, :dr] = 1
    r[:, dr:2 * dr] = 2
    return g.permuted(r, axis=1)


# ---- the two codec kernels ------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("N", NS)
def test_bytes_to_rows_equals_restatement(eng, N):
    g = np.random.default_rng(N)
    for nbytes in block_sizes(N):
        for B in BS:
            data = g.integers(0, 256, (B, nbytes), dtype=np.uint8)
            want = ref.np_bytes_to_rows(data, N)
            for si, so, _ in SHIFTS:
                tag = (N, nbytes, B, si, so)
                d = Dev(eng)
                try:
                    out = d.filled(B * N, so)                                # pre-filled: the pad must be WRITTEN
                    eng.bytes_to_rows_dev(N, nbytes, d.put(data, si), B, out)
                    got, intact = d.get_guarded(out, B * N)
                finally:
                    d.free()
                assert intact, tag + ("dev: bytes around the buffer changed",)
                assert np.array_equal(got.reshape(B, N), want), tag + ("dev",)
                raw_in, vin = host_view(B * nbytes, si)
                vin[:] = data.reshape(-1)
                raw_out, vout = host_view(B * N, so)
                eng._chk(eng._lib.ntru_bytes_to_rows(eng._h, N, nbytes, vp(vin), B, vp(vout)))
                assert guards_ok(raw_out, B * N, so), tag + ("host: bytes around the buffer changed",)
                assert np.array_equal(vout.reshape(B, N), want), tag + ("host",)
            if B == 257:
                assert np.array_equal(eng.bytes_to_rows(N, nbytes, data), want)


def planted_rows(g, N, nbytes, B):
    """Rows from {0, 1}; a listed subset gets a 2 inside the message bits or a 1 or 2 in the pad, at the first and last coefficient of
    each region.  Returns (rows, the planted row indices)."""
    rows = g.integers(0, 2, (B, N), dtype=np.uint8)
    msg = 8 * nbytes
    rows[:, msg:] = 0
    spots = [(0, 2), (msg - 1, 2)] + ([(msg, 1), (N - 1, 2), (msg, 2), (N - 1, 1)] if msg < N else [])
    planted = sorted(set(int(x) for x in g.integers(0, B, min(B, 12)))) if B > 1 else [0]
    for i, b in enumerate(planted):
        k, v = spots[i % len(spots)]
        rows[b, k] = v
    return rows, planted


@pytest.mark.parametrize("N", NS)
def test_rows_to_bytes_equals_restatement(eng, N):
    g = np.random.default_rng(1000 + N)
    for nbytes in block_sizes(N):
        for B in BS:
            rows, planted = planted_rows(g, N, nbytes, B)
            want, want_flags = ref.np_rows_to_bytes(rows, nbytes)
            assert all(want_flags[b] for b in planted) and not want_flags[[b for b in range(B) if b not in planted]].any()
            for si, so, sf in SHIFTS:
                tag = (N, nbytes, B, si, so, sf)
                d = Dev(eng)
                try:
                    out, fl = d.filled(B * nbytes, so), d.filled(B, sf)
                    src = d.put(rows, si)
                    eng.rows_to_bytes_dev(N, nbytes, src, B, out, fl)
                    got, intact = d.get_guarded(out, B * nbytes)
                    got_fl, intact_fl = d.get_guarded(fl, B)
                    out2 = d.filled(B * nbytes, so)
                    eng.rows_to_bytes_dev(N, nbytes, src, B, out2, None)     # flags = NULL
                    got2, intact2 = d.get_guarded(out2, B * nbytes)
                finally:
                    d.free()
                assert intact and intact_fl and intact2, tag + ("dev: bytes around a buffer changed",)
                assert np.array_equal(got.reshape(B, nbytes), want) and np.array_equal(got2.reshape(B, nbytes), want), tag + ("dev",)
                assert np.array_equal(got_fl, want_flags), tag + ("dev flags",)
                raw_in, vin = host_view(B * N, si)
                vin[:] = rows.reshape(-1)
                raw_out, vout = host_view(B * nbytes, so)
                raw_fl, vfl = host_view(B, sf)
                eng._chk(eng._lib.ntru_rows_to_bytes(eng._h, N, nbytes, vp(vin), B, vp(vout), vp(vfl)))
                assert guards_ok(raw_out, B * nbytes, so) and guards_ok(raw_fl, B, sf), tag + ("host: bytes around a buffer changed",)
                assert np.array_equal(vout.reshape(B, nbytes), want) and np.array_equal(vfl, want_flags), tag + ("host",)
            if B == 257:
                got, got_fl = eng.rows_to_bytes(N, nbytes, rows)
                assert np.array_equal(got, want) and np.array_equal(got_fl, want_flags)
                assert np.array_equal(eng.rows_to_bytes(N, nbytes, rows, want_flags=False)[0], want)


# ---- the scheme calls on bytes against the existing calls on rows ---------------------------------------------------------------------

KEY_NAMES = ["n17_q32", "n167_q128_low_noise", "n167_q128_default", "n509_q2048", "n821_q4096"]


@pytest.mark.parametrize("name", KEY_NAMES)
def test_encrypt_and_decrypt_bytes_equal_the_calls_on_rows(eng, keys, name):
    N, q, p, W, h, f, fp, dr = keys[name]
    g = np.random.default_rng(N + q)
    B = 301
    r = rand_r(g, B, N, dr)
    for nbytes in sorted({W, max(1, W - 1)}):
        data = g.integers(0, 256, (B, nbytes), dtype=np.uint8)
        rows = ref.np_bytes_to_rows(data, N)
        for path in (0, 1, 4):
            eng.set_kernel_path(path)
            tag = (name, nbytes, path)
            e_want, quot_want = eng.encrypt_batch(N, q, h, r, rows)
            e, quot = eng.encrypt_bytes_batch(N, q, nbytes, h, r, data)
            assert np.array_equal(e, e_want) and np.array_equal(quot, quot_want), tag + ("encrypt host",)
            assert eng.encrypt_bytes_batch(N, q, nbytes, h, r, data, want_quot=False)[1] is None
            # decrypt: the fresh ciphertexts and, for the flags, rows of noise
            e_mix = e_want.copy()
            e_mix[::7] = g.integers(0, q, e_mix[::7].shape, dtype=np.uint16)
            value = eng.decrypt_batch(N, q, p, f, fp, e_mix, want_witness=False)[0]
            bytes_want, flags_want = ref.np_rows_to_bytes(value, nbytes)
            got, flags = eng.decrypt_bytes_batch(N, q, p, nbytes, f, fp, e_mix)
            assert np.array_equal(got, bytes_want) and np.array_equal(flags, flags_want), tag + ("decrypt host",)
            assert flags_want[::7].any() or N < 64, tag
            d = Dev(eng)
            try:
                d_e, d_q = d.put(np.zeros((B, N), np.uint16)), d.put(np.zeros((B, N), np.uint16))
                eng.encrypt_bytes_batch_dev(N, q, nbytes, d.put(h), d.put(r), d.put(data, 1), B, d_e, d_q)
                e_dev, q_dev = eng.dev_download(d_e, (B, N), np.uint16), eng.dev_download(d_q, (B, N), np.uint16)
                d_out, d_fl = d.filled(B * nbytes, 7), d.filled(B, 1)
                eng.decrypt_bytes_batch_dev(N, q, p, nbytes, d.put(f), d.put(fp), d.put(e_mix), B, d_out, d_fl)
                got_dev, ok1 = d.get_guarded(d_out, B * nbytes)
                fl_dev, ok2 = d.get_guarded(d_fl, B)
                d_out2 = d.filled(B * nbytes, 0)
                eng.decrypt_bytes_batch_dev(N, q, p, nbytes, d.put(f), d.put(fp), d.put(e_mix), B, d_out2, None)
                got_dev2, ok3 = d.get_guarded(d_out2, B * nbytes)
            finally:
                d.free()
            assert np.array_equal(e_dev, e_want) and np.array_equal(q_dev, quot_want), tag + ("encrypt dev",)
            assert ok1 and ok2 and ok3, tag
            assert np.array_equal(got_dev.reshape(B, nbytes), bytes_want) and np.array_equal(fl_dev, flags_want), tag + ("decrypt dev",)
            assert np.array_equal(got_dev2.reshape(B, nbytes), bytes_want), tag + ("decrypt dev, no flags",)
    eng.set_kernel_path(0)


def test_scheme_calls_cross_the_pass_boundary(eng, keys):
    """65536 + 3 blocks at N = 167: the _dev forms run two passes over the engine-owned rows."""
    N, q, p, W, h, f, fp, dr = keys["n167_q128_low_noise"]
    B = 65536 + 3
    g = np.random.default_rng(99)
    r = rand_r(g, B, N, dr)
    data = g.integers(0, 256, (B, W), dtype=np.uint8)
    e_want = eng.encrypt_batch(N, q, h, r, ref.np_bytes_to_rows(data, N), want_quot=False)[0]
    value = eng.decrypt_batch(N, q, p, f, fp, e_want, want_witness=False)[0]
    bytes_want, flags_want = ref.np_rows_to_bytes(value, W)
    d = Dev(eng)
    try:
        d_e = d.put(np.zeros((B, N), np.uint16))
        eng.encrypt_bytes_batch_dev(N, q, W, d.put(h), d.put(r), d.put(data), B, d_e)
        d_out, d_fl = d.filled(B * W), d.filled(B)
        eng.decrypt_bytes_batch_dev(N, q, p, W, d.put(f), d.put(fp), d_e, B, d_out, d_fl)
        e_dev = eng.dev_download(d_e, (B, N), np.uint16)
        got, ok1 = d.get_guarded(d_out, B * W)
        fl, ok2 = d.get_guarded(d_fl, B)
    finally:
        d.free()
    assert np.array_equal(e_dev, e_want)
    assert ok1 and ok2 and np.array_equal(got.reshape(B, W), bytes_want) and np.array_equal(fl, flags_want)
    assert np.array_equal(bytes_want, data) and not flags_want.any()          # this parameter set decrypts every message


def test_pipeline_bytes_batch_equals_pipeline_batch_on_rows(eng, keys):
    N, q, p, W, h, f, fp, dr = keys["n821_q4096"]
    B = 4 * 2048 + 5                                                          # four chunks of the host pipeline
    g = np.random.default_rng(3)
    data = g.integers(0, 256, (B, W), dtype=np.uint8)
    key = g.integers(0, 2 ** 32, 8, dtype=np.uint32)
    want = eng.pipeline_batch(N, q, p, h, ref.np_bytes_to_rows(data, N), f=f, fp=fp, key=key, first_item=11, n1=dr, n2=dr,
                              want_r=True, want_e=True, want_value=True)
    msg_want, flags_want = ref.np_rows_to_bytes(want["value"], W)
    kw = dict(f=f, fp=fp, key=key, first_item=11, n1=dr, n2=dr)
    got = eng.pipeline_bytes_batch(N, q, p, W, h, data, want_r=True, want_e=True, want_msg=True, want_flags=True, **kw)
    for name, w in (("r", want["r"]), ("e", want["e"]), ("msg", msg_want), ("flags", flags_want)):
        assert np.array_equal(got[name], w), ("pageable", name)
    pin = {"r": eng.pinned_empty((B, N), np.uint8), "e": eng.pinned_empty((B, N), np.uint16), "msg": eng.pinned_empty((B, W), np.uint8),
           "flags": eng.pinned_empty((B,), np.uint8)}
    pin_in = eng.pinned_empty((B, W), np.uint8)
    pin_in[:] = data
    got = eng.pipeline_bytes_batch(N, q, p, W, h, pin_in, out=pin, **kw)
    for name, w in (("r", want["r"]), ("e", want["e"]), ("msg", msg_want), ("flags", flags_want)):
        assert got[name] is pin[name] and np.array_equal(got[name], w), ("pinned", name)
    # r given instead of a key; only the message comes back; a smaller block
    got = eng.pipeline_bytes_batch(N, q, p, W - 1, h, data[:, :W - 1], f=f, fp=fp, r=want["r"], want_msg=True)
    value = eng.decrypt_batch(N, q, p, f, fp, eng.encrypt_batch(N, q, h, want["r"], ref.np_bytes_to_rows(data[:, :W - 1], N),
                                                                want_quot=False)[0], want_witness=False)[0]
    assert sorted(got) == ["msg"] and np.array_equal(got["msg"], ref.np_rows_to_bytes(value, W - 1)[0])
    # encrypt only
    got = eng.pipeline_bytes_batch(N, q, p, W, h, data, key=key, first_item=11, n1=dr, n2=dr, want_e=True)
    assert np.array_equal(got["e"], want["e"])


# ---- the reference-captured blocks ------------------------------------------------------------------------------------------------------

def test_golden_blocks(eng, sets):
    for s in sets:
        N, q, p, W, h, f, fp = ref.set_key(s)
        chunks, r, value, decrypted = ref.block_arrays(s)
        assert chunks.shape[0] >= 15
        e, _ = eng.encrypt_bytes_batch(N, q, W, h, r, chunks)
        assert np.array_equal(e, value), s["set"]
        ntru = pkg.NTRU(dict(s["options"], f=s["key"]["f"], fp=s["key"]["fp"], h=s["key"]["h"]), engine=eng)
        assert ntru.bytesPerBlock == W
        at = 0
        for m in s["messages"]:
            n = len(m["blocks"])
            rows = value[at:at + n]
            for b, blk in enumerate(m["blocks"]):                              # block by block: the recorded chunk, flags 0
                got, flags = ntru.decryptBytes(rows[b:b + 1])
                assert got == bytes(blk["chunk"]) and flags.tolist() == [0], (s["set"], m["length"], b)
            # the whole message through the Python mirror, with the recorded r: the recorded ciphertexts, then the message
            e_msg = ntru.encryptBytes(m["data"], r=r[at:at + n])
            assert np.array_equal(e_msg, rows), (s["set"], m["length"])
            got, flags = ntru.decryptBytes(e_msg, length=m["length"])
            assert got == m["data"] and not flags.any(), (s["set"], m["length"])
            assert ntru.decryptBytes(e_msg)[0] == m["data"]                    # no message of the fixture ends in a zero byte
            assert np.array_equal(ntru.encryptBytes(m["data"].decode("latin-1"), r=r[at:at + n]), rows)
            at += n
    assert ntru.encryptBytes(b"").shape == (0, N) and ntru.decryptBytes(np.zeros((0, N), np.uint16)) [0] == b""


def test_python_round_trip_with_fresh_randomness(eng, sets):
    """N = 509, q = 2048, df = dg = 40, dr = 20: |p r g + f m| < 200 < q / 2, every message decrypts whatever r is drawn."""
    s = [x for x in sets if x["set"] == "n509_q2048"][0]
    ntru = pkg.NTRU(dict(s["options"], f=s["key"]["f"], fp=s["key"]["fp"], h=s["key"]["h"]), engine=eng)
    data = bytes(range(256)) + b"\x00\x00tail\x00"
    e = ntru.encryptBytes(data)
    assert e.shape == (-(-len(data) // 63), 509)
    got, flags = ntru.decryptBytes(e, length=len(data))
    assert got == data and not flags.any()
    assert ntru.decryptBytes(e)[0] == data.rstrip(b"\x00")
    with pytest.raises(ValueError, match="length"):
        ntru.decryptBytes(e, length=e.shape[0] * 63 + 1)


def test_wrong_key_is_flagged(eng, sets):
    a, b = [x for x in sets if x["options"]["N"] == 167]
    for own, other in ((a, b), (b, a)):
        _, _, value, _ = ref.block_arrays(own)
        ntru = pkg.NTRU(dict(other["options"], f=other["key"]["f"], fp=other["key"]["fp"], h=other["key"]["h"]), engine=eng)
        _, flags = ntru.decryptBytes(value)
        assert flags.any(), (own["set"], other["set"])
        assert not (flags & ~np.uint8(ref.FLAG_NOT_BITS | ref.FLAG_PAD_NONZERO)).any()


# ---- refusals -----------------------------------------------------------------------------------------------------------------------------

def test_refusals(eng, keys):
    N, q, p, W, h, f, fp, dr = keys["n167_q128_low_noise"]
    lib, H = eng._lib, eng._h
    data = np.zeros((2, W), np.uint8)
    rows = np.zeros((2, N), np.uint8)
    r = np.zeros((2, N), np.uint8)
    e = np.zeros((2, N), np.uint16)
    out = np.zeros((2, W), np.uint8)
    ARG = 2
    for nb, n in ((0, N), (N // 8 + 1, N), (1, 7)):
        assert lib.ntru_bytes_to_rows(H, n, nb, vp(data), 2, vp(rows)) == ARG
        assert lib.ntru_bytes_to_rows_dev(H, n, nb, None, 2, None) == ARG
        assert lib.ntru_rows_to_bytes(H, n, nb, vp(rows), 2, vp(out), None) == ARG
        assert lib.ntru_rows_to_bytes_dev(H, n, nb, None, 2, None, None) == ARG
        assert lib.ntru_encrypt_bytes_batch(H, n, q, nb, vp(h), vp(r), vp(data), 2, vp(e), None) == ARG
        assert lib.ntru_encrypt_bytes_batch_dev(H, n, q, nb, None, None, None, 2, None, None) == ARG
        assert lib.ntru_decrypt_bytes_batch(H, n, q, p, nb, vp(f), vp(fp), vp(e), 2, vp(out), None) == ARG
        assert lib.ntru_decrypt_bytes_batch_dev(H, n, q, p, nb, None, None, None, 2, None, None) == ARG
        assert lib.ntru_pipeline_bytes_batch(H, n, q, p, vp(h), vp(f), vp(fp), None, 0, 0, 0, vp(r), nb, vp(data), 2, None, vp(e), vp(out),
                                             None) == ARG
    # msg_out / flags without the decrypt stage; half a private key; neither key nor r; no output
    flags = np.zeros(2, np.uint8)
    pipe = lib.ntru_pipeline_bytes_batch
    assert pipe(H, N, q, p, vp(h), None, None, None, 0, 0, 0, vp(r), W, vp(data), 2, None, vp(e), vp(out), None) == ARG
    assert pipe(H, N, q, p, vp(h), None, None, None, 0, 0, 0, vp(r), W, vp(data), 2, None, vp(e), None, vp(flags)) == ARG
    assert pipe(H, N, q, p, vp(h), vp(f), None, None, 0, 0, 0, vp(r), W, vp(data), 2, None, vp(e), vp(out), None) == ARG
    assert pipe(H, N, q, p, vp(h), vp(f), vp(fp), None, 0, 0, 0, None, W, vp(data), 2, None, vp(e), vp(out), None) == ARG
    assert pipe(H, N, q, p, vp(h), vp(f), vp(fp), None, 0, 0, 0, vp(r), W, vp(data), 2, None, None, None, None) == ARG
    # a NULL buffer with B > 0
    assert pipe(H, N, q, p, vp(h), vp(f), vp(fp), None, 0, 0, 0, vp(r), W, None, 2, None, vp(e), vp(out), None) == ARG
    assert lib.ntru_bytes_to_rows(H, N, W, None, 2, vp(rows)) == ARG and lib.ntru_bytes_to_rows_dev(H, N, W, None, 2, None) == ARG
    assert lib.ntru_rows_to_bytes(H, N, W, vp(rows), 2, None, None) == ARG and lib.ntru_rows_to_bytes_dev(H, N, W, None, 2, None, None) == ARG
    assert lib.ntru_encrypt_bytes_batch(H, N, q, W, vp(h), vp(r), None, 2, vp(e), None) == ARG
    assert lib.ntru_encrypt_bytes_batch_dev(H, N, q, W, None, None, None, 2, None, None) == ARG
    assert lib.ntru_decrypt_bytes_batch(H, N, q, p, W, vp(f), vp(fp), vp(e), 2, None, None) == ARG
    assert lib.ntru_decrypt_bytes_batch_dev(H, N, q, p, W, None, None, None, 2, None, None) == ARG
    assert b"NULL" in lib.ntru_last_error()
    # B = 0 launches nothing and is fine, whatever the pointers
    assert lib.ntru_bytes_to_rows(H, N, W, None, 0, None) == 0 and lib.ntru_bytes_to_rows_dev(H, N, W, None, 0, None) == 0
    assert lib.ntru_rows_to_bytes(H, N, W, None, 0, None, None) == 0 and lib.ntru_rows_to_bytes_dev(H, N, W, None, 0, None, None) == 0
    assert lib.ntru_encrypt_bytes_batch(H, N, q, W, None, None, None, 0, None, None) == 0
    assert lib.ntru_encrypt_bytes_batch_dev(H, N, q, W, None, None, None, 0, None, None) == 0
    assert lib.ntru_decrypt_bytes_batch(H, N, q, p, W, None, None, None, 0, None, None) == 0
    assert lib.ntru_decrypt_bytes_batch_dev(H, N, q, p, W, None, None, None, 0, None, None) == 0
    assert pipe(H, N, q, p, vp(h), vp(f), vp(fp), None, 0, 0, 0, vp(r), W, None, 0, None, vp(e), vp(out), None) == 0
