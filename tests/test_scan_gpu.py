"""Scanning for decryptable rows on the GPU (ntru_scan_bytes_batch and its three siblings, csrc/scan_hits.hip), byte for byte.  Expected
values: tests/scan_ref.py for the fixture of the unmodified reference; for engine-made batches the unchanged decrypt_bytes_batch per key
plus the numpy filter of scan_ref.select.  Every _dev result is read back whole: what lies behind the stored prefixes must be untouched."""
import json
import os

import numpy as np
import pytest

import __graft_entry__ as ge
import lift_ref
import scan_ref as ref

pytestmark = pytest.mark.gpu
pkg = ge.load_package()
FILL = 0xEE
TAG4 = b"NTRU"


@pytest.fixture(scope="module")
def eng():
    e = pkg.Engine(0)
    yield e
    e.set_kernel_path(0)
    pkg.lift.set_lift(e, "reference")


@pytest.fixture(scope="module")
def cases():
    return ref.load_cases()


class Dev:
    """Device buffers through the engine's own allocator (256-byte aligned), `shift` BYTES off the allocation's start."""

    def __init__(self, eng):
        self.eng, self.held = eng, []

    def put(self, a, shift=0):
        a = np.ascontiguousarray(a)
        p = self.eng.dev_alloc(a.nbytes + shift + 64)
        self.held.append(p)
        if a.nbytes:
            self.eng.dev_upload(p + shift, a)
        return p + shift

    def free(self):
        self.eng.synchronize()
        for p in self.held:
            self.eng.dev_free(p)
        self.held = []


def rand_r(g, B, N, dr):
    r = np.zeros((B, N), np.uint8)
    r[:, :dr] = 1
    r[:, dr:2 * dr] = 2
    return g.permuted(r, axis=1)


def fixture_keys(c):
    """[(h, f, fp)] of a fixture case."""
    return [(c["h"][k], c["f"][k], c["fp"][k]) for k in range(3)]


def make_batch(eng, N, q, keys, dr, B, shares, tag, tag_off, seed):
    """B rows: a share shares[k] of them tagged messages encrypted under key k, the rest arbitrary values below q, in random order."""
    g = np.random.default_rng(seed)
    W = N // 8
    owner = g.choice(len(shares) + 1, size=B, p=list(shares) + [1.0 - sum(shares)])
    data = g.integers(0, 256, (B, W), dtype=np.uint8)
    data[:, tag_off:tag_off + len(tag)] = np.frombuffer(tag, np.uint8)
    e = g.integers(0, q, (B, N)).astype(np.uint16)
    for k in range(len(shares)):
        idx = np.flatnonzero(owner == k)
        if idx.size:
            e[idx] = eng.encrypt_bytes_batch(N, q, W, keys[k][0], rand_r(g, idx.size, N, dr), data[idx], want_quot=False)[0]
    return e


def composition(eng, N, q, p, f, fp, e, tag=b"", tag_off=0, max_hits=None):
    """The scan as the calls it replaces: decrypt_bytes_batch per key, then the filter on the host."""
    f, fp = np.asarray(f).reshape(-1, N), np.asarray(fp).reshape(-1, N)
    res = [ref.select(*eng.decrypt_bytes_batch(N, q, p, N // 8, f[k], fp[k], e), tag, tag_off, max_hits) for k in range(f.shape[0])]
    return np.array([r[0] for r in res], np.int64), [r[1] for r in res], [r[2] for r in res]


def run_dev(eng, N, q, p, f, fp, rows, tag=b"", tag_off=0, max_hits=None, packed=False, shifts=(0, 0, 0), sync=True):
    """One _dev call on fresh device copies; shifts: BYTE offsets of the rows, of d_hit_row and of d_hit_bytes into their allocations.
    Returns a function that reads everything back, checks that nothing behind the stored prefixes (nor around the arrays) changed and
    gives (count, rows, bytes)."""
    W = N // 8
    f, fp = np.ascontiguousarray(f, np.int8).reshape(-1, N), np.ascontiguousarray(fp, np.uint8).reshape(-1, N)
    K, B = f.shape[0], rows.shape[0]
    max_hits = B if max_hits is None else max_hits
    d = Dev(eng)
    d_f, d_fp, d_rows = d.put(f), d.put(fp), d.put(rows, shifts[0])
    d_count = d.put(np.full(K + 2, -7, np.int64)) + 8
    guard = 16
    d_hr = d.put(np.full(K * max_hits * 8 + 2 * guard, FILL, np.uint8), shifts[1]) + guard
    d_hb = d.put(np.full(K * max_hits * W + 2 * guard, FILL, np.uint8), shifts[2]) + guard
    fn = pkg.scan_bytes_packed_batch_dev if packed else pkg.scan_bytes_batch_dev
    fn(eng, N, q, p, W, K, d_f, d_fp, d_rows, B, d_count, tag=tag, tag_off=tag_off, max_hits=max_hits,
       d_hit_row=d_hr if max_hits else None, d_hit_bytes=d_hb if max_hits else None)

    def result():
        eng.synchronize()
        try:
            cnt = eng.dev_download(d_count - 8, (K + 2,), np.int64)
            assert cnt[0] == -7 and cnt[-1] == -7
            count = cnt[1:-1].copy()
            hr = eng.dev_download(d_hr - guard, (K * max_hits * 8 + 2 * guard,), np.uint8)
            hb = eng.dev_download(d_hb - guard, (K * max_hits * W + 2 * guard,), np.uint8)
            assert (hr[:guard] == FILL).all() and (hr[len(hr) - guard:] == FILL).all()
            assert (hb[:guard] == FILL).all() and (hb[len(hb) - guard:] == FILL).all()
            hr = hr[guard:len(hr) - guard].reshape(K, max_hits * 8)
            hb = hb[guard:len(hb) - guard].reshape(K, max_hits * W)
            out_rows, out_bytes = [], []
            for k in range(K):
                s = int(min(count[k], max_hits))
                assert (hr[k, s * 8:] == FILL).all() and (hb[k, s * W:] == FILL).all(), "written behind the stored prefix of key %d" % k
                out_rows.append(np.frombuffer(hr[k, :s * 8].tobytes(), np.int64))
                out_bytes.append(hb[k, :s * W].reshape(s, W).copy())
            return count, out_rows, out_bytes
        finally:
            d.free()
    return result() if sync else result


def all_forms(eng, N, q, p, f, fp, e, tag=b"", tag_off=0, max_hits=None):
    """The four forms on the same rows: dense and packed, host and _dev."""
    packed = pkg.pack_rows(eng, N, q, e)
    return {"host": pkg.scan_bytes_batch(eng, N, q, p, N // 8, f, fp, e, tag, tag_off, max_hits),
            "host packed": pkg.scan_bytes_packed_batch(eng, N, q, p, N // 8, f, fp, packed, tag, tag_off, max_hits),
            "dev": run_dev(eng, N, q, p, f, fp, e, tag, tag_off, max_hits),
            "dev packed": run_dev(eng, N, q, p, f, fp, packed, tag, tag_off, max_hits, packed=True)}


def check(got, want, note=""):
    assert np.array_equal(got[0], want[0]), (note, "count", np.asarray(got[0]).tolist(), np.asarray(want[0]).tolist())
    for k in range(len(want[1])):
        assert np.array_equal(got[1][k], want[1][k]), (note, "rows of key", k)
        assert np.array_equal(got[2][k], want[2][k]), (note, "bytes of key", k)
    assert ref.same(got, want), note


# ---- 1. the fixture -------------------------------------------------------------------------------------------------------------------
def test_fixture_through_every_form(eng, cases):
    for c in cases:
        o = c["options"]
        N, q, p = o["N"], o["q"], o["p"]
        want = (c["hit"].sum(axis=1), [h[0] for h in c["hits"]], [h[1] for h in c["hits"]])
        check(ref.scan(N, q, p, c["W"], c["f"], c["fp"], c["e"], c["tag"], c["tagOffset"]), want, c["set"])
        for name, got in all_forms(eng, N, q, p, c["f"], c["fp"], c["e"], c["tag"], c["tagOffset"]).items():
            check(got, want, (c["set"], name))
        # the NTRU class: the instance's own key, then all three
        ntru = pkg.NTRU({**o, "f": c["f"][1].tolist(), "fp": c["fp"][1].tolist()}, engine=eng)
        one = ntru.scanBytes(c["e"], tag=c["tag"], tagOffset=c["tagOffset"])
        check((one["count"], one["rows"], one["bytes"]), (want[0][1:2], want[1][1:2], want[2][1:2]), c["set"])
        three = ntru.scanPacked(pkg.pack_rows(eng, N, q, c["e"]), keys=[(c["f"][k].tolist(), c["fp"][k].tolist()) for k in range(3)],
                                tag=c["tag"], tagOffset=c["tagOffset"])
        check((three["count"], three["rows"], three["bytes"]), want, c["set"])
    # the third set under the true centred lift: the honest rows are hits (tests/scan_ref.py under that lift)
    c = cases[2]
    o = c["options"]
    want = ref.scan(o["N"], o["q"], o["p"], c["W"], c["f"], c["fp"], c["e"], c["tag"], c["tagOffset"], mode=lift_ref.CENTRED)
    assert want[0].min() >= 2
    ntru = pkg.NTRU({**o, "lift": "centred", "f": c["f"][0].tolist(), "fp": c["fp"][0].tolist()}, engine=eng)
    got = ntru.scanBytes(c["e"], keys=[(c["f"][k], c["fp"][k]) for k in range(3)], tag=c["tag"], tagOffset=c["tagOffset"])
    check((got["count"], got["rows"], got["bytes"]), want, "centred")
    assert pkg.lift.get_lift(eng) == 0


# ---- 2. + 9. block edges, under every kernel path ------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def edge_batch(eng, cases):
    """N = 167, q = 128, 3001 rows: about half tagged under key A, a quarter under key B, the rest arbitrary; expected per prefix length."""
    c = cases[1]
    eng.set_kernel_path(0)
    keys = fixture_keys(c)
    e = make_batch(eng, 167, 128, keys, c["options"]["dr"], 3001, (0.5, 0.25), TAG4, 5, seed=3001)
    f, fp = c["f"][:2], c["fp"][:2]
    want = {B: composition(eng, 167, 128, 3, f, fp, e[:B], TAG4, 5) for B in (1, 63, 64, 65, 257, 3001)}
    assert 1200 < want[3001][0][0] < 1800 and 500 < want[3001][0][1] < 1000
    return e, f, fp, want


@pytest.mark.parametrize("path", [0, 1, 2, 3, 4, 5])
def test_block_edges(eng, edge_batch, path):
    e, f, fp, want = edge_batch
    eng.set_kernel_path(path)
    try:
        for B in (3001, 257, 65, 64, 63, 1) if path == 0 else (3001, 65):
            for name, got in all_forms(eng, 167, 128, 3, f, fp, e[:B], TAG4, 5).items():
                check(got, want[B], (path, B, name))
    finally:
        eng.set_kernel_path(0)


# ---- 3. the pass edge -----------------------------------------------------------------------------------------------------------------
def test_pass_edge(eng, cases):
    c = cases[0]
    N, q, p, B = 17, 32, 3, 65536 + 300
    tag, off = b"\xc3", 1
    e = make_batch(eng, N, q, fixture_keys(c), c["options"]["dr"], B, (1.0,), tag, off, seed=65836)
    f, fp = c["f"][:1], c["fp"][:1]
    want = composition(eng, N, q, p, f, fp, e, tag, off)
    rows = want[1][0]
    assert ((rows >= 65280) & (rows < 65536)).any() and ((rows >= 65536) & (rows < 65836)).any()
    assert 0 < want[0][0] <= B
    for name, got in all_forms(eng, N, q, p, f, fp, e, tag, off).items():
        check(got, want, name)


# ---- 4. truncation ----------------------------------------------------------------------------------------------------------------------
def test_truncation_counts_and_untouched_buffers(eng, cases):
    c = cases[1]
    N, q, p = 167, 128, 3
    e = make_batch(eng, N, q, fixture_keys(c), c["options"]["dr"], 100, (0.4, 0.3), TAG4, 0, seed=40)
    f, fp = c["f"][:2], c["fp"][:2]
    full = composition(eng, N, q, p, f, fp, e, TAG4, 0)
    assert 25 <= full[0][0] <= 60 and full[0][1] > 5          # about 40
    for max_hits in (5, 0, 1, int(full[0][0]), 100, 1000):
        want = (full[0], [r[:max_hits] for r in full[1]], [b[:max_hits] for b in full[2]])
        for name, got in all_forms(eng, N, q, p, f, fp, e, TAG4, 0, max_hits).items():
            check(got, want, (max_hits, name))                       # run_dev checks the canaries behind every stored prefix
    # a tag nobody carries: count 0, buffers untouched
    for name, got in all_forms(eng, N, q, p, f, fp, e, b"nope", 0, 7).items():
        assert got[0].tolist() == [0, 0] and all(r.size == 0 for r in got[1]) and all(b.size == 0 for b in got[2]), name
    # every row a hit: the rows key A decrypts to well-formed bytes, scanned without a tag
    good = e[composition(eng, N, q, p, f[:1], fp[:1], e)[1][0]]
    assert good.shape[0] >= 30
    for name, got in all_forms(eng, N, q, p, f[:1], fp[:1], good).items():
        assert got[0].tolist() == [good.shape[0]] and got[1][0].tolist() == list(range(good.shape[0])), name
        assert np.array_equal(got[2][0], eng.decrypt_bytes_batch(N, q, p, N // 8, f[0], fp[0], good)[0]), name
    # B == 0 sets the counts to 0
    assert pkg.scan_bytes_batch(eng, N, q, p, N // 8, f, fp, e[:0], TAG4, 0)[0].tolist() == [0, 0]
    assert run_dev(eng, N, q, p, f, fp, e[:0], TAG4, 0, max_hits=3)[0].tolist() == [0, 0]


# ---- 5. the tag -------------------------------------------------------------------------------------------------------------------------
def test_tag_positions_lengths_and_single_bits(eng, cases):
    c = cases[1]
    N, q, p, W = 167, 128, 3, 20
    f, fp = c["f"][:1], c["fp"][:1]
    g = np.random.default_rng(5)
    long_tag = bytes(g.integers(0, 256, 20, dtype=np.uint8))
    for tag, off in ((b"", 0), (b"", 20), (TAG4, 0), (TAG4, 16), (long_tag, 0), (b"\x00", 19)):
        e = make_batch(eng, N, q, fixture_keys(c), c["options"]["dr"], 70, (0.5,), tag, off, seed=len(tag) + off)
        want = composition(eng, N, q, p, f, fp, e, tag, off)
        assert want[0][0] >= 20
        for name, got in all_forms(eng, N, q, p, f, fp, e, tag, off).items():
            check(got, want, (tag, off, name))
    # a 32-byte tag needs nbytes >= 32: N = 821
    with open(os.path.join(ge.ROOT, "tests", "golden", "scheme_n821_q4096.json")) as fh:
        gold = json.load(fh)
    o, k = gold["options"], gold["keys"][0]
    pad = lambda a, dt: np.array(list(a) + [0] * (821 - len(a)), dtype=dt)
    h8, f8, fp8 = pad(k["h"], np.uint16), pad(k["f"], np.int8), pad(k["fp"], np.uint8)
    tag32 = bytes(g.integers(0, 256, 32, dtype=np.uint8))
    with pkg.lift.using(eng, "centred"):
        for off in (0, 70):
            e = make_batch(eng, 821, 4096, [(h8, f8, fp8)], o["dr"], 40, (0.6,), tag32, off, seed=off)
            want = composition(eng, 821, 4096, 3, f8, fp8, e, tag32, off)
            assert want[0][0] >= 15
            for name, got in all_forms(eng, 821, 4096, 3, f8, fp8, e, tag32, off).items():
                check(got, want, (32, off, name))
            miss = bytes([tag32[0]]) + bytes([tag32[1] ^ 0x80]) + tag32[2:]
            assert pkg.scan_bytes_batch(eng, 821, 4096, 3, 102, f8, fp8, e, miss, off)[0].tolist() == [0]
    # one flipped bit in any byte of a 4-byte tag turns every hit into a miss; nothing else changes
    e = make_batch(eng, N, q, fixture_keys(c), c["options"]["dr"], 70, (0.5,), TAG4, 7, seed=77)
    want = composition(eng, N, q, p, f, fp, e, TAG4, 7)
    assert want[0][0] >= 20
    for j in range(4):
        for bit in (0, 3, 7):
            bad = bytearray(TAG4)
            bad[j] ^= 1 << bit
            for name, got in (("host", pkg.scan_bytes_batch(eng, N, q, p, W, f, fp, e, bytes(bad), 7)),
                              ("dev", run_dev(eng, N, q, p, f, fp, e, bytes(bad), 7))):
                assert got[0].tolist() == [0] and got[1][0].size == 0, (j, bit, name)
    check(run_dev(eng, N, q, p, f, fp, e, TAG4, 7), want, "after the flips")


# ---- 6. packed = dense --------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("N,q,d", [(167, 2048, 20), (821, 4096, 60), (821, 8192, 60)])
def test_packed_equals_dense_with_the_ignored_bits_set(eng, N, q, d):
    p, B, W = 3, 96, N // 8
    kg = eng.keygen_batch(N, q, p, d, d, np.arange(8, dtype=np.uint32) + N, 2, want=("f", "fp", "h"))
    assert not kg["flags"].any()
    keys = [(kg["h"][k], kg["f"][k], kg["fp"][k]) for k in range(2)]
    with pkg.lift.using(eng, "centred"):
        e = make_batch(eng, N, q, keys, d // 2, B, (0.4, 0.3), TAG4, 2, seed=q)
        want = composition(eng, N, q, p, kg["f"], kg["fp"], e, TAG4, 2)
        assert want[0].min() >= 10
        packed = pkg.pack_rows(eng, N, q, e).copy()
        pr = eng.pack_params(q - 1, N)
        bits, per, osz = pr["maxInputBits"], pr["numInputsPerOutput"], pr["outputSize"]
        # ones in every ignored place: the fields with index >= N and the bits of an element above per * bits
        as_int = [[int(sum(int(packed[b, s, l]) << (64 * l) for l in range(4))) for s in range(osz)] for b in range(B)]
        for b in range(B):
            for s in range(osz):
                used = max(0, min(per, N - s * per))
                v = as_int[b][s] | (((1 << 256) - 1) ^ ((1 << (used * bits)) - 1))
                for l in range(4):
                    packed[b, s, l] = (v >> (64 * l)) & 0xFFFFFFFFFFFFFFFF
        assert not np.array_equal(packed, pkg.pack_rows(eng, N, q, e))
        assert np.array_equal(pkg.unpack_rows(eng, N, q, packed), e)
        check(pkg.scan_bytes_packed_batch(eng, N, q, p, W, kg["f"], kg["fp"], packed, TAG4, 2), want, "host packed")
        check(run_dev(eng, N, q, p, kg["f"], kg["fp"], packed, TAG4, 2, packed=True), want, "dev packed")
        check(pkg.scan_bytes_batch(eng, N, q, p, W, kg["f"], kg["fp"], e, TAG4, 2), want, "host dense")


# ---- 7. the lift --------------------------------------------------------------------------------------------------------------------------
def test_lift_is_the_engines_mode_read_at_enqueue(eng):
    with open(os.path.join(ge.ROOT, "tests", "golden", "scheme_n821_q4096.json")) as fh:
        gold = json.load(fh)
    o, k = gold["options"], gold["keys"][0]
    N, q, p, B = 821, 4096, 3, 96
    pad = lambda a, dt: np.array(list(a) + [0] * (N - len(a)), dtype=dt)
    h, f, fp = pad(k["h"], np.uint16), pad(k["f"], np.int8), pad(k["fp"], np.uint8)
    e = make_batch(eng, N, q, [(h, f, fp)], o["dr"], B, (1.0,), TAG4, 50, seed=821)
    assert pkg.lift.get_lift(eng) == 0
    plain = composition(eng, N, q, p, f, fp, e, TAG4, 50)
    for name, got in all_forms(eng, N, q, p, f, fp, e, TAG4, 50).items():
        check(got, plain, ("reference", name))
    with pkg.lift.using(eng, "centred"):
        centred = composition(eng, N, q, p, f, fp, e, TAG4, 50)
        assert centred[0].tolist() == [B] and centred[1][0].tolist() == list(range(B))          # every row is a hit
        for name, got in all_forms(eng, N, q, p, f, fp, e, TAG4, 50).items():
            check(got, centred, ("centred", name))
        pending = run_dev(eng, N, q, p, f, fp, e, TAG4, 50, sync=False)          # enqueued in the centred mode ...
    assert pkg.lift.get_lift(eng) == 0                                           # ... the mode changes before anything is waited for
    check(pending(), centred, "enqueued before the mode change")
    assert plain[0][0] < B


# ---- 8. alignment -------------------------------------------------------------------------------------------------------------------------
def test_alignment_of_every_device_array(eng, cases):
    c = cases[1]
    N, q, p = 167, 128, 3                                 # 20 bytes per message; the odd length follows below
    e = make_batch(eng, N, q, fixture_keys(c), c["options"]["dr"], 300, (0.5, 0.2), TAG4, 1, seed=8)
    f, fp = c["f"][:2], c["fp"][:2]
    want = composition(eng, N, q, p, f, fp, e, TAG4, 1)
    for shifts in ((2, 8, 1), (2, 8, 3), (0, 8, 7), (6, 248, 15)):
        check(run_dev(eng, N, q, p, f, fp, e, TAG4, 1, shifts=shifts), want, shifts)
    packed = pkg.pack_rows(eng, N, q, e)
    check(run_dev(eng, N, q, p, f, fp, packed, TAG4, 1, packed=True, shifts=(8, 8, 1)), want, "packed")
    # odd nbytes: N = 200 -> 25 bytes per message, hit_bytes one byte off
    kg = eng.keygen_batch(200, 2048, 3, 20, 20, np.arange(8, dtype=np.uint32), 1, want=("f", "fp", "h"))
    assert not kg["flags"].any()
    e = make_batch(eng, 200, 2048, [(kg["h"][0], kg["f"][0], kg["fp"][0])], 10, 300, (0.6,), TAG4, 21, seed=25)
    want = composition(eng, 200, 2048, 3, kg["f"], kg["fp"], e, TAG4, 21)
    assert want[0][0] > 100 and want[2][0].shape[1] == 25
    for shifts in ((2, 8, 1), (0, 0, 0)):
        check(run_dev(eng, 200, 2048, 3, kg["f"], kg["fp"], e, TAG4, 21, shifts=shifts), want, (200, shifts))
    check(pkg.scan_bytes_batch(eng, 200, 2048, 3, 25, kg["f"], kg["fp"], e, TAG4, 21), want, "host")
