"""ntru_combine_batch[_dev] on the GPU, bytes against bytes: the reference-captured combinations (tests/golden/combine_cases.json) and
the tally fixture as the G = 1 column, the exact integer product (tests/combine_ref.py) across the geometries at which the kernels take
another path, both on-device implementations (k_combine_m on the matrix cores, k_combine_v on the vector ALU) against each other,
extreme operands, many row blocks, every alignment with guard bytes, and one device-resident encrypt / combine / decrypt chain."""
import json
import os

import numpy as np
import pytest

import __graft_entry__ as ge
import ciphertext_sum_ref as sum_ref
import combine_ref as ref

pytestmark = pytest.mark.gpu
pkg = ge.load_package()
GUARD = 64            # guard elements on either side of out
FILL = 0xA5C3


@pytest.fixture(scope="module")
def eng():
    e = pkg.Engine(0)
    yield e
    e.set_kernel_path(0)


@pytest.fixture(scope="module")
def sets():
    return ref.load_sets()


def combine_dev(eng, N, mod, rows, weights, shifts=(0, 0, 0)):
    """ntru_combine_batch_dev on device copies; rows, weights and out `shifts` elements off a 256-byte boundary.  rows and weights end
    with their allocation; out lies between guard elements, which must survive."""
    B, G = rows.shape[0], weights.shape[1]
    held = []

    def put(a, shift):
        a = np.ascontiguousarray(a)
        p = eng.dev_alloc(2 * shift + max(a.nbytes, 2))
        held.append(p)
        if a.nbytes:
            eng.dev_upload(p + 2 * shift, a)
        return p + 2 * shift
    try:
        d_rows, d_w = put(rows, shifts[0]), put(weights, shifts[1])
        frame = np.full(GUARD + shifts[2] + G * N + GUARD, FILL, np.uint16)
        d_frame = put(frame, 0)
        pkg.combine_batch_dev(eng, N, mod, d_rows if B else None, d_w if B else None, B, G, d_frame + 2 * (GUARD + shifts[2]))
        got = eng.dev_download(d_frame, frame.shape, np.uint16)
        lo = GUARD + shifts[2]
        assert (got[:lo] == FILL).all() and (got[lo + G * N:] == FILL).all(), "guard elements around out were written"
        return got[lo:lo + G * N].reshape(G, N)
    finally:
        eng.synchronize()
        for p in held:
            eng.dev_free(p)


def rand(N, mod, B, G, seed):
    g = np.random.default_rng(seed)
    return g.integers(0, mod, (B, N), dtype=np.uint16), g.integers(0, mod, (B, G), dtype=np.uint16)


def check_both_paths(eng, N, mod, rows, weights, want=None, host=True):
    """Host and _dev form on kernel paths 0 and 1 against the exact product; the kernels are the ones the launcher's rule names."""
    want = ref.np_combine(rows, weights, mod) if want is None else want
    tag = (N, mod, rows.shape[0], weights.shape[1])
    try:
        for path in (0, 1):
            eng.set_kernel_path(path)
            got = combine_dev(eng, N, mod, rows, weights)
            if rows.shape[0]:
                assert eng.last_kernel() == ref.kernel_of(mod, path, weights.shape[1]), (tag, path)
            assert got.tobytes() == want.tobytes(), (tag, path, "dev")
            if host:
                assert pkg.combine_batch(eng, N, mod, rows, weights).tobytes() == want.tobytes(), (tag, path, "host")
    finally:
        eng.set_kernel_path(0)


# ---- the reference's own combinations -------------------------------------------------------------------------------------------------
def test_fixture_cases_bit_for_bit(eng, sets):
    for s in sets:
        N, q, p, f, fp, rows = ref.set_arrays(s)
        ntru = pkg.NTRU(dict(s["options"], f=s["key"]["f"], fp=s["key"]["fp"], h=s["key"]["h"]), engine=eng)
        for c in s["cases"]:
            w, sums = ref.case_arrays(s, c)
            tag = (s["set"], c["kind"])
            assert pkg.combine_batch(eng, N, q, rows, w).tobytes() == sums.tobytes(), tag
            assert combine_dev(eng, N, q, rows, w).tobytes() == sums.tobytes(), tag
            t = ntru.combineBatch(s["e"], c["weights"])
            for g, o in enumerate(c["outputs"]):
                inp = o["decrypt"]["inputs"]
                for name, key in (("sum", "e"), ("quotient1", "quotient1"), ("remainder1", "remainder1"), ("quotient2", "quotient2"),
                                  ("value", "remainder2")):
                    assert t[name][g].tolist() + [0] * (len(inp[key]) - N) == inp[key], (tag, g, name)
                if o["recovered"]:
                    assert t["value"][g].tolist() == sum_ref.pad(o["expected"], N, np.int64).tolist(), (tag, g)
            bare = ntru.combineBatch(s["e"], c["weights"], want_witness=False)
            assert bare["quotient1"] is None and bare["value"].tobytes() == t["value"].tobytes()
            assert pkg.combineCiphertexts(s["e"], q, c["weights"], engine=eng) == [pkg.trimPolynomial(o["sum"]) for o in c["outputs"]]


def test_tally_fixture_is_the_first_column(eng):
    cases = sum_ref.load_cases()
    assert len(cases) >= 12
    for c in cases:
        N, q, p, f, fp, rows, w, total = sum_ref.case_arrays(c)
        w = np.ones(rows.shape[0], np.uint16) if w is None else w
        assert np.array_equal(pkg.combine_batch(eng, N, q, rows, w[:, None])[0], total), (c["set"], c["K"], c["weights"])
        assert np.array_equal(combine_dev(eng, N, q, rows, w[:, None])[0], total), (c["set"], c["K"], c["weights"])


def test_rows_equal_sum_groups(eng):
    """Row g is byte for byte ntru_sum_groups with column g as the weights."""
    for N, mod, B, G in ((167, 128, 100, 3), (821, 4096, 777, 5), (33, 65521, 300, 2)):
        rows, w = rand(N, mod, B, G, 11)
        got = pkg.combine_batch(eng, N, mod, rows, w)
        for g in range(G):
            assert got[g].tobytes() == eng.sum_groups(N, mod, rows, weights=np.ascontiguousarray(w[:, g]))[0].tobytes(), (N, mod, g)


# ---- geometries ---------------------------------------------------------------------------------------------------------------------------
NS = [2, 31, 32, 33, 63, 65, 167, 821, 1920]
GS = [1, 2, 31, 32, 33, 65]
BS = [1, 15, 16, 17, 31, 32, 33, 63, 64, 65, 1000]
MODS = [2, 128, 4096, 8192, 65536]


def grid():
    """Every value of each axis with the others cycling, and the full G x B product at N = 33, mod = 4096."""
    pts = []
    for axis, values in enumerate((NS, GS, BS, MODS)):
        for i, v in enumerate(values):
            pt = [NS[(i + 1) % len(NS)], GS[(i + 2) % len(GS)], BS[(i + 3) % len(BS)], MODS[i % len(MODS)]]
            pt[axis] = v
            pts.append(tuple(pt))
    pts += [(33, G, B, 4096) for G in GS for B in BS]
    return sorted(set(pts))


def test_the_grid_covers_every_axis_value():
    pts = grid()
    assert 90 <= len(pts) <= 120
    for axis, values in enumerate((NS, GS, BS, MODS)):
        assert {p[axis] for p in pts} >= set(values)


@pytest.mark.parametrize("chunk", range(4))
def test_geometry_grid_equals_the_exact_product(eng, chunk):
    for k, (N, G, B, mod) in enumerate(grid()):
        if k % 4 == chunk:
            rows, w = rand(N, mod, B, G, 1000 + k)
            check_both_paths(eng, N, mod, rows, w)


@pytest.mark.parametrize("mod", [3, 5, 7, 65521, 65535])
def test_moduli_that_are_no_powers_of_two(eng, mod):
    for N, G, B in ((17, 3, 100), (167, 33, 1000), (821, 2, 4097)):
        rows, w = rand(N, mod, B, G, mod + N)
        want = ref.np_combine(rows, w, mod)
        try:
            for path in (0, 1, 4):
                eng.set_kernel_path(path)
                assert combine_dev(eng, N, mod, rows, w).tobytes() == want.tobytes(), (N, G, B, path)
                assert eng.last_kernel() == "k_combine_v<0>"
        finally:
            eng.set_kernel_path(0)
        assert pkg.combine_batch(eng, N, mod, rows, w).tobytes() == want.tobytes(), (N, G, B, "host")


# ---- extreme operands ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mod", [65536, 4096, 65521])
def test_every_operand_at_its_maximum(eng, mod):
    """70 000 rows of mod - 1 under weights of mod - 1: more rows than one row block, and sums far beyond 32 bits."""
    N, G, B = 33, 33, 70000
    rows, w = np.full((B, N), mod - 1, np.uint16), np.full((B, G), mod - 1, np.uint16)
    want = np.full((G, N), (mod - 1) * (mod - 1) * B % mod, np.uint16)
    check_both_paths(eng, N, mod, rows, w, want)


@pytest.mark.parametrize("mod", [65536, 4096, 65521])
def test_digit_boundaries_on_a_long_contraction(eng, mod):
    """Operands of 128 and 0x8080 (both digits at -128, the largest digit products) over 70 000 rows."""
    N, G, B = 33, 33, 70000
    v = 0x8080 if mod > 0x8080 else 128
    rows, w = np.full((B, N), v, np.uint16), np.full((B, G), v, np.uint16)
    rows[::7, ::3], w[::5, ::2] = 127, 255
    check_both_paths(eng, N, mod, rows, w, host=False)


@pytest.mark.parametrize("mod", [4096, 65521])
def test_zero_one_hot_and_identity_weights(eng, mod):
    N, G, B = 33, 33, 33
    rows, _ = rand(N, mod, B, G, 3)
    check_both_paths(eng, N, mod, rows, np.zeros((B, G), np.uint16), np.zeros((G, N), np.uint16))
    check_both_paths(eng, N, mod, rows, np.eye(B, dtype=np.uint16), rows)                       # identity-like: out == rows
    pick = np.random.default_rng(4).integers(0, B, G)
    hot = np.zeros((B, G), np.uint16)
    hot[pick, np.arange(G)] = 1                                                                  # one row per output
    check_both_paths(eng, N, mod, rows, hot, rows[pick])


# ---- row blocks -----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("N,mod,G", [(821, 4096, 3), (2, 2, 1)])
def test_many_row_blocks(eng, N, mod, G):
    for B in (20000, 20001):
        rows, w = rand(N, mod, B, G, B)
        check_both_paths(eng, N, mod, rows, w)


@pytest.mark.parametrize("N", [2, 33])
def test_one_row_block_stores_directly(eng, N):
    """33 rows are fewer than a row block holds at the least: one block, and the row kernel stores the final rows itself; G = 4096 is
    the widest weight matrix."""
    rows, w = rand(N, 4096, 33, 4096, N)
    check_both_paths(eng, N, 4096, rows, w)


# ---- alignment, guards, empty batches, chunking ------------------------------------------------------------------------------------------------
def test_every_alignment_with_guards(eng):
    N, mod, G, B = 821, 4096, 33, 65
    rows, w = rand(N, mod, B, G, 8)
    want = ref.np_combine(rows, w, mod)
    try:
        for path in (0, 1):
            eng.set_kernel_path(path)
            for k in range(8):
                shifts = (k & 1, (k >> 1) & 1, (k >> 2) & 1)
                assert combine_dev(eng, N, mod, rows, w, shifts).tobytes() == want.tobytes(), (path, shifts)
    finally:
        eng.set_kernel_path(0)
    # host arrays one element off as well
    hr, hw = np.zeros(B * N + 1, np.uint16), np.zeros(B * G + 1, np.uint16)
    hr[1:], hw[1:] = rows.ravel(), w.ravel()
    assert pkg.combine_batch(eng, N, mod, hr[1:].reshape(B, N), hw[1:].reshape(B, G)).tobytes() == want.tobytes()


def test_no_rows_give_zero_rows(eng):
    for mod in (4096, 65521):
        rows, w = np.zeros((0, 17), np.uint16), np.zeros((0, 5), np.uint16)
        assert not combine_dev(eng, 17, mod, rows, w).any()
        out = pkg.combine_batch(eng, 17, mod, rows, w)
        assert out.shape == (5, 17) and not out.any()


def test_host_form_over_several_chunks(eng):
    N, G, B = 2, 2, 100003                 # above ntru_chunk_items: four chunks, the last three add to the first
    for mod in (4096, 65521):
        rows, w = rand(N, mod, B, G, mod)
        assert pkg.combine_batch(eng, N, mod, rows, w).tobytes() == ref.np_combine(rows, w, mod).tobytes(), mod


def test_host_form_refuses_a_weight_that_is_not_below_mod(eng):
    rows, w = rand(17, 32, 9, 4, 1)
    w[6, 2] = 32
    with pytest.raises(pkg.EngineError) as ei:
        pkg.combine_batch(eng, 17, 32, rows, w)
    assert ei.value.code == 2 and "row 6" in str(ei.value) and "column 2" in str(ei.value)


# ---- device-resident chains ------------------------------------------------------------------------------------------------------------------
def test_device_resident_encrypt_combine_decrypt(eng, sets):
    """Sample r, encrypt 64 bit messages, combine them by the overlapping 0/1 matrix (grand total + two halves), decrypt: all on the
    device, on one stream.  The VerifyDecrypt kernel accepts every witness."""
    import torch
    s = next(s for s in sets if s["set"] == "n509_q2048")
    o = s["options"]
    N, q, p, dr = o["N"], o["q"], o["p"], o["dr"]
    B, G = 64, 3
    dev = torch.device("cuda:0")
    eng.set_stream(torch.cuda.current_stream().cuda_stream)
    try:
        up = lambda a: torch.from_numpy(a.view(np.int16) if a.dtype == np.uint16 else a).to(dev)
        h, f, fp = (up(sum_ref.pad(s["key"][k], N, dt)) for k, dt in (("h", np.uint16), ("f", np.int8), ("fp", np.uint8)))
        d = lambda dt, shape: torch.empty(shape, dtype=dt, device=dev)
        r = d(torch.uint8, (B, N))
        eng.sample_ternary_dev(N, dr, dr, p - 1, np.arange(8, dtype=np.uint32), 0, B, r.data_ptr())
        m = torch.randint(0, 2, (B, N), generator=torch.Generator(device=dev).manual_seed(3), device=dev, dtype=torch.int32).to(torch.uint8)
        e = d(torch.int16, (B, N))
        eng.encrypt_batch_dev(N, q, h.data_ptr(), r.data_ptr(), m.data_ptr(), B, e.data_ptr())
        w_host = np.array([[1, b < B // 2, b >= B // 2] for b in range(B)], np.uint16)
        w = up(w_host)
        c, q1, r1 = d(torch.int16, (G, N)), d(torch.int16, (G, N)), d(torch.int16, (G, N))
        v, q2 = d(torch.uint8, (G, N)), d(torch.uint8, (G, N))
        pkg.combine_batch_dev(eng, N, q, e.data_ptr(), w.data_ptr(), B, G, c.data_ptr())
        eng.decrypt_batch_dev(N, q, p, f.data_ptr(), fp.data_ptr(), c.data_ptr(), G, v.data_ptr(), q1.data_ptr(), r1.data_ptr(), q2.data_ptr())
        torch.cuda.synchronize()
        e_host = e.cpu().numpy().view(np.uint16)
        assert c.cpu().numpy().view(np.uint16).tobytes() == ref.np_combine(e_host, w_host, q).tobytes()
        ntru = pkg.NTRU(o)
        nq, np_ = ntru.calculateNq(), ntru.calculateNp()
        pad1 = lambda t: torch.nn.functional.pad(t.to(torch.int32), (0, 1)).to(torch.int16).contiguous()
        f16 = torch.where(f < 0, f.to(torch.int32) + q, f.to(torch.int32)).to(torch.int16).repeat(G, 1).contiguous()
        fp16 = fp.to(torch.int16).repeat(G, 1).contiguous()
        flags = d(torch.uint8, (G,))
        wit = [f16, fp16, c, pad1(q1), pad1(r1), pad1(q2), pad1(v)]
        eng.check_decrypt_batch_dev(N, q, nq, p, np_, *[t.data_ptr() for t in wit], G, flags.data_ptr())
        torch.cuda.synchronize()
        assert not flags.any().item()
    finally:
        eng.set_stream(None)


def test_centred_lift_recovers_sums_of_two(eng):
    """N = 821, q = 4096: the reference's lift is off there (q = 1 mod 3); in the centred mode every output of two summands decrypts to
    the sum of its plaintexts modulo p."""
    with open(os.path.join(ge.ROOT, "tests", "golden", "scheme_n821_q4096.json")) as fh:
        gold = json.load(fh)
    o, key = gold["options"], gold["keys"][0]
    N, q, p, dr = o["N"], o["q"], o["p"], o["dr"]
    B, G = 8, 4
    g = np.random.default_rng(821)
    m = g.integers(0, 2, (B, N), dtype=np.uint8)
    r = eng.sample_ternary(N, dr, dr, p - 1, np.arange(8, dtype=np.uint32), 0, B)
    e, _ = eng.encrypt_batch(N, q, sum_ref.pad(key["h"], N, np.uint16), r, m)
    w = np.zeros((B, G), np.uint16)
    w[np.arange(B), np.arange(B) // 2] = 1
    ntru = pkg.NTRU(dict(o, f=key["f"], fp=key["fp"], h=key["h"], lift="centred"), engine=eng)
    t = ntru.combineBatch(e, w)
    assert t["sum"].tobytes() == ref.np_combine(e, w, q).tobytes()
    want = (w.astype(np.int64).T @ m) % p
    assert t["value"].tolist() == want.tolist()
    assert pkg.lift.get_lift(eng) == pkg.lift.REFERENCE
