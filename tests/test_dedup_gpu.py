"""ntru_dedup_rows[_dev] and ntru_dedup_packed[_dev] on the GPU, byte for byte against numpy.unique (tests/dedup_ref.py): a thinned cross
product of N (every fill of the last 16-byte load, every rows-per-wave geometry), mod (powers of two and not, raw equality) and B
(the 256-row compaction unit, the sort tile, the 65536 pass and the 2^18 round of the sort's offsets), with the row families mixed in
every batch; prior sets with duplicates of their own; narrow fingerprints, the only way into collision resolution; salts; NULL
outputs; the empty batch; the host forms; NTRU.dedupBatch on the fixture; and a call on another stream right behind a dedup.
Outputs sit between guard elements, on and 8 bytes off a 16-byte boundary; unique is untouched behind its count[0] entries."""
import ctypes as C

import numpy as np
import pytest

import __graft_entry__ as ge
import dedup_ref as ref
import packed_ref

pytestmark = pytest.mark.gpu
pkg = ge.load_package()
GUARD = 16
FILL = -0x5A3C5A3C5A3C5A3D
NS = [2, 7, 8, 9, 63, 64, 65, 167, 509, 821, 1024, 1919, 1920]
MODS = [2, 3, 7, 128, 4096, 65536]
BS = [1, 2, 255, 256, 257, 1025, 70001, 2 ** 18 + 3]
# (N, mod, B): every value of every axis at least once; the two large B at N = 8 and N = 167 only
CASES = [(2, 2, 1), (7, 3, 2), (8, 7, 255), (9, 128, 256), (63, 4096, 257), (64, 65536, 1025), (65, 2, 255), (167, 3, 257),
         (509, 7, 256), (821, 4096, 1025), (1024, 128, 2), (1919, 65536, 257), (1920, 4096, 255), (8, 4096, 70001),
         (167, 128, 2 ** 18 + 3), (8, 3, 2 ** 18 + 3), (167, 65536, 70001)]


@pytest.fixture(scope="module")
def eng():
    e = pkg.Engine(0)
    yield e
    e.close()


def dedup_dev(eng, N, mod, rows, prior=None, packed=False, salt=0x0123456789ABCDEF, bits=64, outputs=(True, True), shifts=(0, 0, 0)):
    """The _dev form on device copies: rows / prior dense uint16 [.][N] (shifts[0] elements of 2 bytes off a 256-byte boundary) or,
    with packed, uint64 [.][os][4] (shifts[0] elements of 8 bytes off); first and unique between guard elements, shifts[1] and
    shifts[2] elements of 8 bytes off.  An output that is not asked for is NULL and must stay untouched; unique must be untouched
    behind count[0] entries.  Returns (first or None, unique or None, count)."""
    dt = np.uint64 if packed else np.uint16
    rows = np.ascontiguousarray(rows, dt)
    B = rows.shape[0]
    S = 0 if prior is None else len(prior)
    held = []

    def put(a, shift_bytes=0):
        a = np.ascontiguousarray(a)
        p = eng.dev_alloc(shift_bytes + max(a.nbytes, 8))
        held.append(p)
        if a.nbytes:
            eng.dev_upload(p + shift_bytes, a)
        return p + shift_bytes
    try:
        sb = shifts[0] * dt().itemsize
        d_rows = put(rows, sb)
        d_prior = put(np.ascontiguousarray(prior, dt), sb) if S else None
        work = eng.dev_alloc(max(pkg.dedup_workspace_bytes(eng, N, S + B), 8))
        held.append(work)
        frames = [np.full(GUARD + shifts[1] + B + GUARD, FILL, np.int64), np.full(GUARD + shifts[2] + B + GUARD, FILL, np.int64),
                  np.full(2 * GUARD + 1, FILL, np.int64)]
        d_frames = [put(fr) for fr in frames]
        at = [d_frames[0] + 8 * (GUARD + shifts[1]), d_frames[1] + 8 * (GUARD + shifts[2]), d_frames[2] + 8 * GUARD]
        call = pkg.dedup_packed_dev if packed else pkg.dedup_rows_dev
        call(eng, N, mod, d_prior, S, d_rows, B, salt, bits, work, at[0] if outputs[0] else None, at[1] if outputs[1] else None, at[2])
        got = [eng.dev_download(d, fr.shape, np.int64) for d, fr in zip(d_frames, frames)]
        count = int(got[2][GUARD])
        assert (got[2][:GUARD] == FILL).all() and (got[2][GUARD + 1:] == FILL).all(), "guard elements around count were written"
        assert 0 <= count <= B
        out = []
        for k, name in enumerate(("first", "unique")):
            lo = GUARD + shifts[1 + k]
            assert (got[k][:lo] == FILL).all() and (got[k][lo + B:] == FILL).all(), "guard elements around %s were written" % name
            body = got[k][lo:lo + B]
            if not outputs[k]:
                assert (body == FILL).all(), "%s was written though it was not asked for" % name
                body = None
            elif k == 1:
                assert (body[count:] == FILL).all(), "unique was written behind its count[0] entries"
                body = body[:count]
            out.append(body)
        return out[0], out[1], count
    finally:
        eng.synchronize()
        for p in held:
            eng.dev_free(p)


def same(got, wanted, tag):
    first, unique, count = got
    wf, wu = wanted
    assert count == len(wu), (tag, "count", count, len(wu))
    assert first is None or first.tobytes() == wf.tobytes(), (tag, "first", np.nonzero(first != wf)[0][:8])
    assert unique is None or unique.tobytes() == wu.tobytes(), (tag, "unique")


def packed_of(mod, N, rows, rng):
    """The rows in the wire format, the ignored fields and high bits of every other row set, the rest left zero: equal rows differ there."""
    p = packed_ref.pack_rows(mod, rows)
    p[::2] = packed_ref.set_ignored_bits(mod, N, p[::2])
    return p


# ---- the cross product ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("N,mod,B", CASES)
def test_families_dense_and_packed(eng, N, mod, B):
    """The mixed families as dense rows (raw values up to 65535: mod and 2 mod added), then the same rows reduced below 2^bits as packed
    rows -- at a modulus that is no power of two the raw fields reach mod and beyond -- with ignored bits that differ between copies."""
    rng = np.random.default_rng(N * 131 + B)
    rows = ref.family_rows(rng, N, mod, B)
    wanted = ref.want(mod, rows)
    same(dedup_dev(eng, N, mod, rows, shifts=(B & 1, 1, 0)), wanted, "dense")
    bits = packed_ref.params(mod - 1, N)[0]
    raw = rows & ((1 << bits) - 1)                                            # what a field can hold; >= mod for some unless mod = 2^bits
    if mod & (mod - 1):
        raw[0, 0] = (1 << bits) - 1
        assert raw.max() >= mod
        wanted = ref.want(mod, raw)                                           # (a power of two: the same reduced rows, the same answer)
    packed = packed_of(mod, N, raw, rng)
    if B <= 1025:
        assert ref.want_packed(mod, N, packed)[0].tobytes() == wanted[0].tobytes()
    same(dedup_dev(eng, N, mod, packed, packed=True, shifts=(1, 0, 1)), wanted, "packed")


def test_the_axes_are_all_met():
    assert {c[0] for c in CASES} == set(NS) and {c[1] for c in CASES} == set(MODS) and {c[2] for c in CASES} == set(BS)
    assert all(c[0] in (8, 167) for c in CASES if c[2] > 1025)
    assert sorted({(N - 1) % 8 + 1 for N in NS}) == [1, 2, 5, 7, 8]           # the fills of the last 16-byte load
    assert {min((N + 7) // 8, 33) for N in NS} >= {1, 2, 8, 9, 21, 33}        # 64, 32, 8, 7, 3 rows per wave; one row per wave


@pytest.mark.parametrize("N,mod,B", [(167, 4096, 1025), (9, 3, 600)])
def test_all_distinct_and_all_identical(eng, N, mod, B):
    rng = np.random.default_rng(N)
    rows = rng.integers(0, mod, (B, N)).astype(np.uint16)
    digits = np.arange(B)
    for k in range(N - 1, max(N - 9, -1), -1):                                # the row number in base mod in the last coefficients
        rows[:, k] = digits % mod
        digits = digits // mod
    first, unique, count = dedup_dev(eng, N, mod, rows)
    assert count == B and first.tolist() == list(range(B)) and unique.tolist() == list(range(B))
    same((first, unique, count), ref.want(mod, rows), "distinct")
    rows[:] = rows[B // 2]
    first, unique, count = dedup_dev(eng, N, mod, rows)
    assert count == 1 and not first.any() and unique.tolist() == [0]
    twice = np.repeat(rng.integers(0, mod, (B // 2, N)).astype(np.uint16), 2, axis=0)      # every row twice, the copies adjacent
    twice[::2, 0], twice[1::2, 0] = np.arange(B // 2) % mod, np.arange(B // 2) % mod
    same(dedup_dev(eng, N, mod, twice), ref.want(mod, twice), "twice")
    mirror = np.concatenate([twice[::2], twice[::2][::-1]])                                 # copies at b and B - 1 - b
    same(dedup_dev(eng, N, mod, mirror), ref.want(mod, mirror), "mirror")
    zero = np.zeros((5, N), np.uint16)
    zero[3, N - 1] = mod if mod < 65536 else 0                                              # still the all-zero row
    zero[4, 0] = 1
    first, unique, count = dedup_dev(eng, N, mod, zero)
    assert first.tolist() == [0, 0, 0, 0, 4] and unique.tolist() == [0, 4]


# ---- prior sets ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("S", [0, 1, 300, 70000])
def test_prior_sets(eng, S):
    """Prior rows repeat one another, so first must name the smallest index; new rows match the prior set, each other, or nothing."""
    N, mod, B = (8, 7, 257) if S == 70000 else (167, 128, 257)
    rng = np.random.default_rng(S + 1)
    prior = ref.family_rows(rng, N, mod, S) if S else None
    rows = ref.family_rows(rng, N, mod, B)
    if S:
        prior[S - 1] = prior[0]
        pick = rng.integers(0, S, B // 3)
        rows[5:5 + B // 3] = prior[pick]                                                    # match the prior set
        rows[-1] = prior[S - 1]                                                             # index 0, not S - 1
    wanted = ref.want(mod, rows, prior)
    if S:
        assert wanted[0][-1] == 0 and (wanted[0] < S).sum() >= B // 3
    assert (wanted[0] >= S).sum() > len(wanted[1]) > 3                                     # some match each other, some nothing
    same(dedup_dev(eng, N, mod, rows, prior=prior, shifts=(S & 1, 1, 1)), wanted, "dense")
    if S <= 300:
        bits = packed_ref.params(mod - 1, N)[0]
        pr = None if prior is None else packed_of(mod, N, prior & ((1 << bits) - 1), rng)
        same(dedup_dev(eng, N, mod, packed_of(mod, N, rows & ((1 << bits) - 1), rng), prior=pr, packed=True),
             ref.want(mod, rows & ((1 << bits) - 1), None if prior is None else prior & ((1 << bits) - 1)), "packed")


# ---- what must not matter ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("N,mod,S,B,packed", [(167, 128, 300, 300, False), (9, 3, 0, 600, False), (821, 4096, 7, 100, False),
                                              (167, 12289, 40, 257, True), (64, 128, 0, 255, True)])
def test_the_fingerprint_width_changes_no_byte(eng, N, mod, S, B, packed):
    """3 bits: every run of the sorted order holds many distinct rows; 0 bits: every row collides with every other (S + B <= 600, where
    the walk is small).  Both must give the bytes of the 64-bit run: the only test of collision resolution."""
    assert S + B <= 600
    rng = np.random.default_rng(N + B)
    both = ref.family_rows(rng, N, mod, S + B)
    if packed:
        both &= (1 << packed_ref.params(mod - 1, N)[0]) - 1
    wanted = ref.want(mod, both[S:], both[:S] if S else None)
    assert 3 < len(wanted[1]) < B
    if packed:
        both = packed_of(mod, N, both, rng)
    runs = [dedup_dev(eng, N, mod, both[S:], prior=both[:S] if S else None, packed=packed, bits=b) for b in (64, 3, 0)]
    for got in runs:
        same(got, wanted, "bits")
        assert got[0].tobytes() == runs[0][0].tobytes() and got[1].tobytes() == runs[0][1].tobytes() and got[2] == runs[0][2]


def test_narrow_fingerprints_at_a_larger_size(eng):
    N, mod, B = 64, 4096, 1025
    rows = ref.family_rows(np.random.default_rng(9), N, mod, B)
    wanted = ref.want(mod, rows)
    for bits in (64, 3, 1):
        same(dedup_dev(eng, N, mod, rows, bits=bits), wanted, bits)


def test_two_salts_give_the_same_bytes(eng):
    N, mod, B = 509, 2048, 1025
    rows = ref.family_rows(np.random.default_rng(4), N, mod, B)
    wanted = ref.want(mod, rows)
    for salt in (0, 1, 0xFFFFFFFFFFFFFFFF, 0x9E3779B97F4A7C15):
        same(dedup_dev(eng, N, mod, rows, salt=salt), wanted, salt)


def test_each_output_null_in_turn(eng):
    N, mod, B = 167, 128, 257
    rows = ref.family_rows(np.random.default_rng(5), N, mod, B)
    wanted = ref.want(mod, rows)
    for outputs in ((True, False), (False, True), (False, False)):
        got = dedup_dev(eng, N, mod, rows, outputs=outputs, shifts=(1, 1, 1))
        assert (got[0] is None) == (not outputs[0]) and (got[1] is None) == (not outputs[1])
        same(got, wanted, outputs)
        same(dedup_dev(eng, N, mod, packed_of(mod, N, rows & 127, None), packed=True, outputs=outputs), ref.want(mod, rows & 127), outputs)


def test_the_empty_batch(eng):
    for packed in (False, True):
        empty = np.zeros((0, 3, 4), np.uint64) if packed else np.zeros((0, 17), np.uint16)
        first, unique, count = dedup_dev(eng, 17, 32, empty, packed=packed)
        assert count == 0 and first.shape == (0,) and unique.shape == (0,)
    prior = np.ones((4, 17), np.uint16)
    assert dedup_dev(eng, 17, 32, np.zeros((0, 17), np.uint16), prior=prior)[2] == 0
    first, unique = pkg.dedup_rows(eng, 17, 32, np.zeros((0, 17), np.uint16))
    assert first.shape == (0,) and unique.shape == (0,)


# ---- the host forms ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("B", [5, 8197])                  # one chunk; several chunks, the last one ragged
def test_host_forms(eng, B):
    rng = np.random.default_rng(B)
    for N, mod, S in ((17, 32, 0), (97, 8192, 9)):
        both = ref.family_rows(rng, N, mod, S + B)
        prior, rows = (both[:S] if S else None), both[S:]
        wf, wu = ref.want(mod, rows, prior)
        first, unique = pkg.dedup_rows(eng, N, mod, rows, prior=prior, salt=B)
        assert first.tobytes() == wf.tobytes() and unique.tobytes() == wu.tobytes(), (N, "dense")
        first, unique = pkg.dedup_rows(eng, N, mod, rows, prior=prior, want_first=False)
        assert first is None and unique.tobytes() == wu.tobytes()
        first, unique = pkg.dedup_rows(eng, N, mod, rows, prior=prior, want_unique=False)
        assert unique is None and first.tobytes() == wf.tobytes()
        bits = packed_ref.params(mod - 1, N)[0]
        raw = both & ((1 << bits) - 1)
        pk = packed_of(mod, N, raw, rng)
        wf, wu = ref.want(mod, raw[S:], raw[:S] if S else None)
        first, unique = pkg.dedup_packed(eng, N, mod, pk[S:], prior=pk[:S] if S else None, salt=7)
        assert first.tobytes() == wf.tobytes() and unique.tobytes() == wu.tobytes(), (N, "packed")
    # unique is untouched behind count[0] entries in the caller's own array too
    lib = pkg.load_library()
    ptr = lambda a: a.ctypes.data_as(C.c_void_p)
    rows = np.ascontiguousarray(both[S:])
    first, unique, count = np.full(B, FILL, np.int64), np.full(B, FILL, np.int64), np.full(1, FILL, np.int64)
    eng._chk(lib.ntru_dedup_rows(eng._h, N, mod, None, 0, ptr(rows), B, 3, 64, ptr(first), ptr(unique), ptr(count)))
    wf, wu = ref.want(mod, rows)
    assert count[0] == len(wu) and first.tobytes() == wf.tobytes() and unique[:len(wu)].tobytes() == wu.tobytes()
    assert (unique[len(wu):] == FILL).all()


# ---- Python ----------------------------------------------------------------------------------------------------------------------------------
def test_fixture_through_the_reference_style_method(eng):
    for c in ref.load_cases():
        ntru = pkg.NTRU({"N": c["N"], "q": c["q"]}, engine=eng)
        prior = np.array(c["prior"], np.uint16) if c["prior"] else None
        rows = np.array(c["rows"], np.uint16)
        for salt in (None, 5):
            got = ntru.dedupBatch(rows, prior=prior, salt=salt)
            assert got["first"].tolist() == c["first"] and got["unique"].tolist() == c["unique"], c["name"]
        bits = packed_ref.params(c["q"] - 1, c["N"])[0]
        raw, praw = rows & ((1 << bits) - 1), (None if prior is None else prior & ((1 << bits) - 1))
        wf, wu = ref.want(c["q"], raw, praw)
        got = ntru.dedupBatch(packed_ref.pack_rows(c["q"], raw), packed=True, prior=None if praw is None else packed_ref.pack_rows(c["q"], praw))
        assert got["first"].tolist() == wf.tolist() and got["unique"].tolist() == wu.tolist(), c["name"]


# ---- the scratch hand-over through the sort ------------------------------------------------------------------------------------------------
def test_a_call_on_another_stream_right_behind_a_dedup(eng):
    """The sort inside the dedup takes and releases the engine's scratch buffer; a draw on another stream right behind it takes the same
    buffer and must wait for the sort.  Both results are checked, and a second dedup behind the draw."""
    import torch
    N, mod, B = 167, 128, 9001
    rows = ref.family_rows(np.random.default_rng(6), N, mod, B)
    wanted = ref.want(mod, rows)
    key = np.arange(8, dtype=np.uint32)
    eng.set_stream(0)
    alone = pkg.draw_permutation(eng, key, 3, 50000)                          # more temporaries than the dedup's sort: a regrow
    other = torch.cuda.Stream()
    held = []
    try:
        d_rows = eng.dev_alloc(rows.nbytes); held.append(d_rows)
        eng.dev_upload(d_rows, rows)
        work = eng.dev_alloc(pkg.dedup_workspace_bytes(eng, N, B)); held.append(work)
        outs = [eng.dev_alloc(8 * B) for _ in range(4)] + [eng.dev_alloc(16)]
        held += outs
        d_src = eng.dev_alloc(8 * 50000); held.append(d_src)
        pkg.dedup_rows_dev(eng, N, mod, None, 0, d_rows, B, 1, 64, work, outs[0], outs[1], outs[4])
        eng.set_stream(other.cuda_stream)
        pkg.draw_permutation_dev(eng, key, 3, 50000, d_src)
        eng.synchronize()
        eng.set_stream(0)
        eng.synchronize()
        pkg.dedup_rows_dev(eng, N, mod, None, 0, d_rows, B, 2, 64, work, outs[2], outs[3], outs[4] + 8)
        eng.synchronize()
        assert eng.dev_download(d_src, (50000,), np.int64).tobytes() == alone.tobytes()
        counts = eng.dev_download(outs[4], (2,), np.int64)
        assert counts.tolist() == [len(wanted[1])] * 2
        for k in (0, 2):
            assert eng.dev_download(outs[k], (B,), np.int64).tobytes() == wanted[0].tobytes()
            assert eng.dev_download(outs[k + 1], (B,), np.int64)[:counts[0]].tobytes() == wanted[1].tobytes()
    finally:
        eng.set_stream(0)
        eng.synchronize()
        for p in held:
            eng.dev_free(p)


def test_the_launch_log_names_the_kernel(eng, tmp_path, monkeypatch):
    import json
    log = tmp_path / "launches.jsonl"
    monkeypatch.setenv("NTRU_LAUNCH_LOG", str(log))
    rows = np.ones((5, 17), np.uint16)
    dedup_dev(eng, 17, 32, rows)
    assert eng.last_kernel() == "k_dedup_emit"
    dedup_dev(eng, 17, 32, packed_ref.pack_rows(32, rows), prior=packed_ref.pack_rows(32, rows[:2]), packed=True, outputs=(True, False))
    rec = [json.loads(line) for line in log.read_text().splitlines()]
    assert rec == [{"kernel": "k_dedup_emit", "N": 17, "items": 5, "bytes_per_item": 34},
                   {"kernel": "k_dedup_offsets", "N": 17, "items": 7, "bytes_per_item": 96}]
