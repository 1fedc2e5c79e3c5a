"""Counting decrypted messages on the GPU (ntru_count_bytes_batch and its three siblings, csrc/count_bytes.hip), byte for byte.  Expected
values: tests/count_ref.py on the oracle for the fixture of the unmodified reference; for engine-made batches the composition the call
replaces -- the unchanged decrypt_bytes_batch plus the numpy classification of count_ref -- never the call under test.  Every _dev
result is read back whole, with what lies around count and cls."""
import numpy as np
import pytest

import __graft_entry__ as ge
import count_ref as ref
import lift_ref

pytestmark = pytest.mark.gpu
pkg = ge.load_package()
FILL = 0xEE
TAG4 = b"NTRU"
SMALL = dict(first_choice=1, n_choices=4, field_off=0, field_len=1, tag=b"\xc3", tag_off=1)                 # the fixture's W = 2 layout
LARGE = dict(first_choice=0x0100, n_choices=5, field_off=8, field_len=2, tag=TAG4, tag_off=3)              # the fixture's W = 20 layout


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
    """[(h, f, fp)] of a fixture case: the counting key, then the foreign key."""
    return [(c["h"][k], c["f"][k], c["fp"][k]) for k in range(2)]


def make_ballots(eng, N, q, keys, dr, B, lay, seed, honest=0.6):
    """B rows in random order: a share `honest` of tagged ballots under keys[0] whose field holds first_choice - 1 .. first_choice +
    n_choices (both ends outside the range), a tenth of ballots under keys[0] with one tag bit flipped, the rest half ballots under the
    foreign keys[1] and half arbitrary values below q."""
    g = np.random.default_rng(seed)
    W, tag = N // 8, np.frombuffer(lay["tag"], np.uint8)
    rest = (0.9 - honest) / 2
    kind = g.choice(4, size=B, p=[honest, 0.1, rest, rest])
    data = g.integers(0, 256, (B, W), dtype=np.uint8)
    v = np.clip(lay["first_choice"] + g.integers(-1, lay["n_choices"] + 1, B), 0, 256 ** lay["field_len"] - 1)
    for j in range(lay["field_len"]):
        data[:, lay["field_off"] + j] = (v >> (8 * (lay["field_len"] - 1 - j))) & 255
    data[:, lay["tag_off"]:lay["tag_off"] + tag.size] = tag                      # after the field: where they overlap the tag wins
    if tag.size:
        flip = np.flatnonzero(kind == 1)
        data[flip, lay["tag_off"] + g.integers(0, tag.size, flip.size)] ^= (1 << g.integers(0, 8, flip.size)).astype(np.uint8)
    e = g.integers(0, q, (B, N)).astype(np.uint16)
    for key, own in ((keys[0], kind <= 1), (keys[1], kind == 2)):
        idx = np.flatnonzero(own)
        if idx.size:
            e[idx] = eng.encrypt_bytes_batch(N, q, W, key[0], rand_r(g, idx.size, N, dr), data[idx], want_quot=False)[0]
    return e


def composition(eng, N, q, p, f, fp, e, lay, groups=None, G=1):
    """The count as the calls it replaces: decrypt_bytes_batch, then the classification and the table on the host."""
    return ref.count_data(*eng.decrypt_bytes_batch(N, q, p, N // 8, f, fp, e), groups=groups, G=G, **lay)


def run_dev(eng, N, q, p, f, fp, rows, lay, groups=None, G=1, packed=False, want_cls=True, shifts=(0, 0, 0), sparse=False):
    """One _dev call on fresh device copies; shifts: BYTE offsets of the rows, of d_group and of d_cls into their allocations.  count
    is pre-filled (the call SETS it) and stands between two guard words, cls between guard bytes.  Returns (count, cls)."""
    W = N // 8
    B, n_bins = rows.shape[0], lay["n_choices"] + 3
    d = Dev(eng)
    try:
        d_f, d_fp = d.put(np.ascontiguousarray(f, np.int8)), d.put(np.ascontiguousarray(fp, np.uint8))
        d_rows = d.put(rows, shifts[0])
        d_group = d.put(np.ascontiguousarray(groups, np.int32), shifts[1]) if groups is not None else None
        d_count = d.put(np.full(G * n_bins + 2, -7, np.int64)) + 8
        guard = 16
        d_cls = d.put(np.full(B * 4 + 2 * guard, FILL, np.uint8), shifts[2]) + guard
        fn = pkg.count_bytes_packed_batch_dev if packed else pkg.count_bytes_batch_dev
        fn(eng, N, q, p, W, d_f, d_fp, d_rows, B, d_count, d_group=d_group, G=G, d_cls=d_cls if want_cls else None, **lay)
        eng.synchronize()
        assert eng.last_kernel() == "k_count_classify" or B == 0
        cnt = eng.dev_download(d_count - 8, (G * n_bins + 2,), np.int64)
        assert cnt[0] == -7 and cnt[-1] == -7
        raw = eng.dev_download(d_cls - guard, (B * 4 + 2 * guard,), np.uint8)
        assert (raw[:guard] == FILL).all() and (raw[len(raw) - guard:] == FILL).all()
        body = raw[guard:len(raw) - guard]
        if not want_cls:
            assert (body == FILL).all()
        count = cnt[1:-1] if sparse else cnt[1:-1].reshape(G, n_bins).copy()
        return count, np.frombuffer(body.tobytes(), np.int32) if want_cls else None
    finally:
        d.free()


def all_forms(eng, N, q, p, f, fp, e, lay, groups=None, G=1):
    """The four forms on the same rows: dense and packed, host and _dev."""
    packed = pkg.pack_rows(eng, N, q, e)
    W = N // 8
    return {"host": pkg.count_bytes_batch(eng, N, q, p, W, f, fp, e, groups=groups, G=G, classes=True, **lay),
            "host packed": pkg.count_bytes_packed_batch(eng, N, q, p, W, f, fp, packed, groups=groups, G=G, classes=True, **lay),
            "dev": run_dev(eng, N, q, p, f, fp, e, lay, groups, G),
            "dev packed": run_dev(eng, N, q, p, f, fp, packed, lay, groups, G, packed=True)}


def check(got, want, note=""):
    assert got[0].shape == want[0].shape and got[0].dtype == np.int64, (note, got[0].shape, want[0].shape)
    assert np.array_equal(got[0], want[0]), (note, "count", np.argwhere(got[0] != want[0])[:5].tolist())
    assert got[1].dtype == np.int32 and np.array_equal(got[1], want[1]), (note, "cls", np.flatnonzero(got[1] != want[1])[:5].tolist())


# ---- 1. the fixture -------------------------------------------------------------------------------------------------------------------
def test_fixture_through_every_form(eng, cases):
    for c in cases:
        o = c["options"]
        N, q, p, lay = o["N"], o["q"], o["p"], ref.layout(c)
        want = (c["count"], c["cls"])
        check(ref.count_bytes(N, q, p, c["W"], c["f"][0], c["fp"][0], c["e"], groups=c["group"], G=3, **lay), want, c["set"])
        for name, got in all_forms(eng, N, q, p, c["f"][0], c["fp"][0], c["e"], lay, c["group"], 3).items():
            check(got, want, (c["set"], name))
        ntru = pkg.NTRU({**o, "f": c["f"][0].tolist(), "fp": c["fp"][0].tolist()}, engine=eng)
        kw = dict(tag=c["tag"], tagOffset=c["tagOffset"], groups=c["group"], G=3)
        one = ntru.countBytes(c["e"], c["firstChoice"], c["nChoices"], c["fieldOffset"], c["fieldLength"], classes=True, **kw)
        check((one["count"], one["classes"]), want, (c["set"], "countBytes"))
        two = ntru.countPacked(pkg.pack_rows(eng, N, q, c["e"]), c["firstChoice"], c["nChoices"], c["fieldOffset"], c["fieldLength"], **kw)
        assert two["classes"] is None and np.array_equal(two["count"], want[0]), (c["set"], "countPacked")
    # the third set under the true centred lift: the honest ballots are in their bins (tests/count_ref.py under that lift)
    c = cases[2]
    o, lay = c["options"], ref.layout(c)
    want = ref.count_bytes(o["N"], o["q"], o["p"], c["W"], c["f"][0], c["fp"][0], c["e"], mode=lift_ref.CENTRED, groups=c["group"], G=3, **lay)
    assert want[0][:, :c["nChoices"]].sum() == 9
    ntru = pkg.NTRU({**o, "lift": "centred", "f": c["f"][0].tolist(), "fp": c["fp"][0].tolist()}, engine=eng)
    kw = dict(tag=c["tag"], tagOffset=c["tagOffset"], groups=c["group"], G=3, classes=True)
    got = ntru.countBytes(c["e"], c["firstChoice"], c["nChoices"], c["fieldOffset"], c["fieldLength"], **kw)
    check((got["count"], got["classes"]), want, "centred")
    got = ntru.countPacked(pkg.pack_rows(eng, o["N"], o["q"], c["e"]), c["firstChoice"], c["nChoices"], c["fieldOffset"], c["fieldLength"], **kw)
    check((got["count"], got["classes"]), want, "centred packed")
    assert pkg.lift.get_lift(eng) == 0
    with pkg.lift.using(eng, "centred"):
        for name, got in all_forms(eng, o["N"], o["q"], o["p"], c["f"][0], c["fp"][0], c["e"], lay, c["group"], 3).items():
            check(got, want, ("centred", name))
    assert pkg.lift.get_lift(eng) == 0


# ---- 2. block and tile edges, under every kernel path ---------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def edge_batch(eng, cases):
    """N = 167, q = 128, 3001 rows, about 60 % honest ballots (five in seven of them inside the range), G = 3 with random ids; the composition's classes of every row, computed once."""
    c = cases[1]
    eng.set_kernel_path(0)
    e = make_ballots(eng, 167, 128, fixture_keys(c), c["options"]["dr"], 3001, LARGE, seed=3001)
    f, fp = c["f"][0], c["fp"][0]
    data, flags = eng.decrypt_bytes_batch(167, 128, 3, 20, f, fp, e)
    cls = ref.classify(data, flags, **LARGE)
    groups = np.random.default_rng(3).integers(0, 3, 3001).astype(np.int32)
    assert 1100 < (cls < 5).sum() < 1500 and all((cls == k).sum() > 100 for k in range(8))
    return e, f, fp, groups, cls, (data, flags)


@pytest.mark.parametrize("path", [0, 1, 2, 3, 4, 5])
def test_block_and_tile_edges(eng, edge_batch, path):
    e, f, fp, groups, cls, _ = edge_batch
    eng.set_kernel_path(path)
    try:
        for B in (3001, 257, 256, 255, 65, 64, 63, 1) if path == 0 else (3001, 65):
            want = ref.tabulate(cls[:B], 5, groups[:B], 3)
            for name, got in all_forms(eng, 167, 128, 3, f, fp, e[:B], LARGE, groups[:B], 3).items():
                check(got, want, (path, B, name))
    finally:
        eng.set_kernel_path(0)


# ---- 3. the pass edge -----------------------------------------------------------------------------------------------------------------
def test_pass_edge(eng, cases):
    c = cases[0]
    N, q, p, B = 17, 32, 3, 65536 + 300
    e = make_ballots(eng, N, q, fixture_keys(c), c["options"]["dr"], B, SMALL, seed=65836)
    f, fp = c["f"][0], c["fp"][0]
    groups = np.random.default_rng(4).integers(0, 3, B).astype(np.int32)
    want = composition(eng, N, q, p, f, fp, e, SMALL, groups, 3)
    in_bins = (want[1] >= 0) & (want[1] < 4)
    assert in_bins[65280:65536].any() and in_bins[65536:].any()
    assert want[0].sum() == B and (want[0].sum(axis=0) > 0).all()
    for name, got in all_forms(eng, N, q, p, f, fp, e, SMALL, groups, 3).items():
        check(got, want, name)


# ---- 4. both accumulation routes and their border ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("n_choices,G", [(ref.CT_LDS_BINS - 3, 1), (ref.CT_LDS_BINS - 2, 1), (2, 3000), (2, 1638), (2, 1639)])
def test_both_routes_agree_with_the_composition(eng, edge_batch, n_choices, G):
    """bins = G (n_choices + 3): 8192 is the last table counted in LDS, 8193 the first counted with one global atomic per row; 8190 and
    8195 are the same border with groups."""
    e, f, fp, _, _, decrypted = edge_batch
    lay = dict(LARGE, first_choice=0x0100 if n_choices == 2 else 0, n_choices=n_choices)
    groups = None if G == 1 else np.random.default_rng(G).integers(0, G, 3001).astype(np.int32)
    want = ref.count_data(*decrypted, groups=groups, G=G, **lay)
    assert want[0].sum() == 3001 and (want[1] < n_choices).sum() > 300
    for name, got in all_forms(eng, 167, 128, 3, f, fp, e, lay, groups, G).items():
        check(got, want, (n_choices, G, name))


def test_the_largest_table(eng, edge_batch):
    """G * n_bins = 2^24 exactly: the bins the composition fills are compared, every other one is zero."""
    e, f, fp, _, cls, _ = edge_batch
    G, n_bins = 1 << 21, 8
    assert G * n_bins == ref.MAX_BINS
    groups = np.random.default_rng(21).integers(0, G, 3001).astype(np.int32)
    groups[:2] = [0, G - 1]
    bins, times = np.unique(groups.astype(np.int64) * n_bins + cls, return_counts=True)
    for name, (count, got_cls) in (("dev", run_dev(eng, 167, 128, 3, f, fp, e, LARGE, groups, G, sparse=True)),
                                   ("host", pkg.count_bytes_batch(eng, 167, 128, 3, 20, f, fp, e, groups=groups, G=G, classes=True, **LARGE))):
        count = count.reshape(-1)
        assert count.size == 1 << 24 and np.array_equal(got_cls, cls), name
        assert np.array_equal(count[bins], times) and np.count_nonzero(count) == bins.size and count.sum() == 3001, name


# ---- 5. the field -----------------------------------------------------------------------------------------------------------------------
FIELDS = [dict(LARGE, field_off=off, field_len=n, first_choice=3 if n == 1 else 0x0100, tag_off=8)
          for n in (1, 2, 3, 4) for off in (0, 20 - n)]
FIELDS += [dict(LARGE, field_len=4, first_choice=0, n_choices=2), dict(LARGE, field_len=4, first_choice=0xFFFFFFFF, n_choices=2),
           dict(LARGE, field_off=5, field_len=4, first_choice=0x52550100),          # the field's first two bytes are the tag's last two
           dict(LARGE, tag=b"")]


@pytest.mark.parametrize("k", range(len(FIELDS)))
def test_field_lengths_positions_and_the_64_bit_compare(eng, cases, k):
    c, lay = cases[1], FIELDS[k]
    N, q, p, B = 167, 128, 3, 200
    e = make_ballots(eng, N, q, fixture_keys(c), c["options"]["dr"], B, lay, seed=500 + k)
    f, fp = c["f"][0], c["fp"][0]
    groups = np.random.default_rng(k).integers(0, 2, B).astype(np.int32)
    want = composition(eng, N, q, p, f, fp, e, lay, groups, 2)
    n = lay["n_choices"]
    assert (want[1] < n).sum() >= 40 and (want[1] == n).sum() >= 5 and (want[1] == n + 2).sum() >= 20, (lay, want[0].tolist())
    assert lay["first_choice"] != 0xFFFFFFFF or want[0][:, 0].sum() >= 10          # v = 2^32 - 1 is choice 0 of that range
    for name, got in all_forms(eng, N, q, p, f, fp, e, lay, groups, 2).items():
        check(got, want, (k, name))


# ---- 6. groups ----------------------------------------------------------------------------------------------------------------------------
def test_groups(eng, cases):
    c = cases[1]
    N, q, p, W, B = 167, 128, 3, 20, 300
    e = make_ballots(eng, N, q, fixture_keys(c), c["options"]["dr"], B, LARGE, seed=6)
    f, fp = c["f"][0], c["fp"][0]
    # no group array: one group
    want = composition(eng, N, q, p, f, fp, e, LARGE)
    assert want[0].shape == (1, 8) and want[0].sum() == B
    for name, got in all_forms(eng, N, q, p, f, fp, e, LARGE).items():
        check(got, want, ("one group", name))
    # an empty group
    groups = np.random.default_rng(6).choice([0, 1, 3], B).astype(np.int32)
    want = composition(eng, N, q, p, f, fp, e, LARGE, groups, 4)
    assert want[0][2].sum() == 0 and (want[0].sum(axis=1)[[0, 1, 3]] > 50).all()
    for name, got in all_forms(eng, N, q, p, f, fp, e, LARGE, groups, 4).items():
        check(got, want, ("empty group", name))
    # ids outside [0, G): counted nowhere, class -1 (the _dev forms; the host forms refuse them and name the index)
    bad = groups.copy()
    bad[[17, 256]] = [-1, 4]
    want = composition(eng, N, q, p, f, fp, e, LARGE, bad, 4)
    assert want[1][17] == want[1][256] == -1 and (want[1] == -1).sum() == 2 and want[0].sum() == B - 2
    check(run_dev(eng, N, q, p, f, fp, e, LARGE, bad, 4), want, "ids outside")
    check(run_dev(eng, N, q, p, f, fp, pkg.pack_rows(eng, N, q, e), LARGE, bad, 4, packed=True), want, "ids outside, packed")
    with pytest.raises(pkg.EngineError, match=r"group\[17\] = -1 is outside \[0, G\)"):
        pkg.count_bytes_batch(eng, N, q, p, W, f, fp, e, groups=bad, G=4, **LARGE)
    # no cls: the same table, nothing written where cls would be
    want = composition(eng, N, q, p, f, fp, e, LARGE, groups, 4)
    got = run_dev(eng, N, q, p, f, fp, e, LARGE, groups, 4, want_cls=False)
    assert got[1] is None and np.array_equal(got[0], want[0])
    got = pkg.count_bytes_batch(eng, N, q, p, W, f, fp, e, groups=groups, G=4, **LARGE)
    assert got[1] is None and np.array_equal(got[0], want[0])
    # B == 0 sets a pre-filled count to 0
    got = run_dev(eng, N, q, p, f, fp, e[:0], LARGE, groups[:0], 4)
    assert got[0].shape == (4, 8) and not got[0].any() and got[1].size == 0
    got = pkg.count_bytes_batch(eng, N, q, p, W, f, fp, e[:0], groups=groups[:0], G=4, classes=True, **LARGE)
    assert got[0].shape == (4, 8) and not got[0].any() and got[1].size == 0


# ---- 7. packed = dense --------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("N,q,d", [(167, 2048, 20), (821, 4096, 60), (821, 8192, 60)])
def test_packed_equals_dense_with_the_ignored_bits_set(eng, N, q, d):
    p, B, W = 3, 96, N // 8
    kg = eng.keygen_batch(N, q, p, d, d, np.arange(8, dtype=np.uint32) + N, 2, want=("f", "fp", "h"))
    assert not kg["flags"].any()
    keys = [(kg["h"][k], kg["f"][k], kg["fp"][k]) for k in range(2)]
    f, fp = kg["f"][0], kg["fp"][0]
    groups = np.random.default_rng(q).integers(0, 3, B).astype(np.int32)
    with pkg.lift.using(eng, "centred"):
        e = make_ballots(eng, N, q, keys, d // 2, B, LARGE, seed=q)
        want = composition(eng, N, q, p, f, fp, e, LARGE, groups, 3)
        assert (want[1] < 5).sum() >= 30 and (want[1] == 7).sum() >= 10
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
        check(pkg.count_bytes_packed_batch(eng, N, q, p, W, f, fp, packed, groups=groups, G=3, classes=True, **LARGE), want, "host packed")
        check(run_dev(eng, N, q, p, f, fp, packed, LARGE, groups, 3, packed=True), want, "dev packed")
        check(pkg.count_bytes_batch(eng, N, q, p, W, f, fp, e, groups=groups, G=3, classes=True, **LARGE), want, "host dense")
        check(run_dev(eng, N, q, p, f, fp, e, LARGE, groups, 3), want, "dev dense")


# ---- 8. alignment -------------------------------------------------------------------------------------------------------------------------
def test_alignment_of_every_device_array(eng, cases):
    c = cases[1]
    N, q, p, B = 167, 128, 3, 300
    e = make_ballots(eng, N, q, fixture_keys(c), c["options"]["dr"], B, LARGE, seed=8)
    f, fp = c["f"][0], c["fp"][0]
    groups = np.random.default_rng(8).integers(0, 3, B).astype(np.int32)
    want = composition(eng, N, q, p, f, fp, e, LARGE, groups, 3)
    for shifts in ((2, 4, 4), (2, 12, 20), (0, 4, 12), (6, 252, 4)):          # rows at any even byte, group and cls at any multiple of 4
        check(run_dev(eng, N, q, p, f, fp, e, LARGE, groups, 3, shifts=shifts), want, shifts)
    packed = pkg.pack_rows(eng, N, q, e)
    check(run_dev(eng, N, q, p, f, fp, packed, LARGE, groups, 3, packed=True, shifts=(8, 4, 12)), want, "packed")
    # odd nbytes: N = 200 -> 25 bytes per message, the field in the last two of them
    kg = eng.keygen_batch(200, 2048, 3, 20, 20, np.arange(8, dtype=np.uint32), 2, want=("f", "fp", "h"))
    assert not kg["flags"].any()
    lay = dict(LARGE, field_off=23, tag_off=19)
    e = make_ballots(eng, 200, 2048, [(kg["h"][k], kg["f"][k], kg["fp"][k]) for k in range(2)], 10, B, lay, seed=25)
    want = composition(eng, 200, 2048, 3, kg["f"][0], kg["fp"][0], e, lay, groups, 3)
    assert (want[1] < 5).sum() > 100
    for shifts in ((2, 4, 4), (0, 0, 0)):
        check(run_dev(eng, 200, 2048, 3, kg["f"][0], kg["fp"][0], e, lay, groups, 3, shifts=shifts), want, (200, shifts))
    check(pkg.count_bytes_batch(eng, 200, 2048, 3, 25, kg["f"][0], kg["fp"][0], e, groups=groups, G=3, classes=True, **lay), want, "host")
