"""ntru_noise_batch[_dev] and its packed forms on the GPU, exact integers against exact integers: every expected value is the oracle's
decrypt_batch rem1 reduced in numpy.  Every strip geometry of k_noise_m on kernel paths 0, 4 and 5, every operand kind, every batch
size, a second row block per workgroup, every alignment between guard bytes with each output NULL in turn, the slow route, the packed
forms, the host forms, the lift mode, the launch log, and the fixture of the unmodified reference through NTRU.noiseBatch and Node."""
import ctypes as C
import json
import os
import shutil
import subprocess

import numpy as np
import pytest

import __graft_entry__ as ge
import noise_ref as ref
import packed_ref

pytestmark = pytest.mark.gpu
pkg = ge.load_package()
GUARD = 16            # guard elements on either side of peak and energy
FILL16, FILL64 = 0xA5C3, 0xA5C3A5C3A5C3A5C3
NS = [2, 17, 33, 64, 96, 97, 128, 167, 509, 512, 513, 821, 1023, 1024]
QS = [2, 4, 128, 2048, 4096, 8192]
BS = [1, 31, 32, 33, 65]


@pytest.fixture(scope="module")
def eng():
    e = pkg.Engine(0)
    yield e
    e.set_kernel_path(0)


def noise_dev(eng, N, q, f, e, outputs=(True, True), shifts=(0, 0, 0), packed=None):
    """ntru_noise_batch_dev on device copies (ntru_noise_packed_batch_dev on `packed`, uint64 [B][os][4], when given): e and peak
    shifts[0], shifts[1] elements of 2 bytes off a 256-byte boundary, energy shifts[2] elements of 8 bytes.  peak and energy lie
    between guard elements, which must survive; an output that is not asked for is passed as NULL and must stay untouched.  Returns
    (peak or None, energy or None)."""
    rows = np.ascontiguousarray(e, np.uint16).reshape(-1, N) if packed is None else np.ascontiguousarray(packed, np.uint64)
    B = rows.shape[0]
    held = []

    def put(a, shift_bytes):
        a = np.ascontiguousarray(a)
        p = eng.dev_alloc(shift_bytes + max(a.nbytes, 8))
        held.append(p)
        if a.nbytes:
            eng.dev_upload(p + shift_bytes, a)
        return p + shift_bytes
    try:
        d_f, d_rows = put(np.asarray(f, np.int8), 0), put(rows, 2 * shifts[0] if packed is None else 8 * shifts[0])
        frames = [np.full(GUARD + shifts[1] + B + GUARD, FILL16, np.uint16), np.full(GUARD + shifts[2] + B + GUARD, FILL64, np.uint64)]
        d_frames = [put(fr, 0) for fr in frames]
        at = [d_frames[0] + 2 * (GUARD + shifts[1]), d_frames[1] + 8 * (GUARD + shifts[2])]
        args = (eng, N, q, d_f, d_rows, B, at[0] if outputs[0] else None, at[1] if outputs[1] else None)
        (pkg.noise_batch_dev if packed is None else pkg.noise_packed_batch_dev)(*args)
        out = []
        for k, (d, fr, sh, fill, dt) in enumerate(zip(d_frames, frames, shifts[1:], (FILL16, FILL64), (np.uint16, np.uint64))):
            got = eng.dev_download(d, fr.shape, dt)
            lo = GUARD + sh
            assert (got[:lo] == fill).all() and (got[lo + B:] == fill).all(), "guard elements around %s were written" % ("peak", "energy")[k]
            body = got[lo:lo + B]
            if not outputs[k]:
                assert (body == fill).all(), "%s was written though it was not asked for" % ("peak", "energy")[k]
                body = None
            out.append(body)
        return out
    finally:
        eng.synchronize()
        for p in held:
            eng.dev_free(p)


def check(eng, N, q, f, e, paths=(0, 4, 5), tag=None, wanted=None, **kw):
    wp, we = wanted if wanted is not None else ref.want(N, q, f, e)
    try:
        for path in paths:
            eng.set_kernel_path(path)
            peak, energy = noise_dev(eng, N, q, f, e, **kw)
            assert eng.last_kernel().startswith(ref.kernel_of(N, q, path)), (tag, N, q, path, eng.last_kernel())
            assert peak is None or peak.tolist() == wp.tolist(), (tag, N, q, path, "peak", np.nonzero(peak != wp)[0][:8])
            assert energy is None or energy.tolist() == we.tolist(), (tag, N, q, path, "energy", np.nonzero(energy != we)[0][:8])
    finally:
        eng.set_kernel_path(0)
    return wp, we


def planted_rows(N, q, j, sign):
    """Under f = sign x^j: a with one non-zero coefficient (every column at N = 97, the tile borders elsewhere; the values around q/2),
    a zero row, and a row that makes every a_k = q/2.  (rows, peak, energy) with the expected values from the construction itself."""
    cols = list(range(N)) if N == 97 else ref.border_columns(N)
    rows, a = ref.spike_rows(N, q, j, sign, cols, ref.edge_values(q))
    rows = np.concatenate([rows, np.zeros((1, N), np.uint16), np.full((1, N), q // 2, np.uint16)])
    a = np.concatenate([a, np.zeros((1, N), np.uint16), np.full((1, N), q // 2, np.uint16)])
    return rows, ref.reduce_rows(a, q)


# ---- geometries and operands -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("N", NS)
def test_every_strip_geometry_with_every_operand_kind(eng, N):
    """Waves without a strip (NT 1 to 3), the first NT at which every wave has one, one and two rounds of strips, strips of unequal
    width, last tiles with 1, 2, 7, 17, 21, 29, 31 and 32 valid columns; q and B cycle with N so that every value of both is met.  Path
    0 below N = 64 takes the slow route and must give the same numbers."""
    i = NS.index(N)
    rng = np.random.default_rng(200 + N)
    for k in range(2):
        q, B = QS[(i + k) % len(QS)], BS[(i + 2 * k) % len(BS)]
        check(eng, N, q, ref.ternary(rng, N), rng.integers(0, q, (B, N)), tag="random")
        f, e = ref.honest(N, q, B, seed=k)
        wp, _ = check(eng, N, q, f, e, tag="honest")
        if q >= 2048:
            assert int(wp.max()) < q // 4, "honest ciphertexts are expected to be quiet here: an unmasked junk column would show"
        j, sign = (5 * i + 1) % N, (1, -1)[k]
        rows, wanted = planted_rows(N, q, j, sign)
        got = check(eng, N, q, ref.monomial(N, j, sign), rows, tag="planted")
        assert got[0].tolist() == wanted[0].tolist() and got[1].tolist() == wanted[1].tolist(), "the oracle agrees with the construction"
        assert wanted[0][-1] == q // 2 and wanted[1][-1] == N * (q // 2) ** 2 and wanted[0][-2] == 0 and wanted[1][-2] == 0


def test_the_axes_cycle_through_every_value():
    met = [(QS[(i + k) % len(QS)], BS[(i + 2 * k) % len(BS)]) for i in range(len(NS)) for k in range(2)]
    assert {q for q, _ in met} == set(QS) and {b for _, b in met} == set(BS)
    assert sorted({(N + 31) // 32 for N in NS}) == [1, 2, 3, 4, 6, 16, 17, 26, 32]
    assert sorted({(N - 1) % 32 + 1 for N in NS}) == [1, 2, 7, 17, 21, 29, 31, 32]


def test_the_energy_needs_the_64_bit_fold(eng):
    """Every a_k = q/2 at N = 1024, q = 8192: energy = 1024 . 4096^2 = 2^34."""
    N, q = 1024, 8192
    rows = np.full((3, N), q // 2, np.uint16)
    rows[1] = 0
    wp, we = check(eng, N, q, ref.monomial(N, 7, -1), rows)
    assert wp.tolist() == [q // 2, 0, q // 2] and we.tolist() == [1 << 34, 0, 1 << 34]


@pytest.mark.parametrize("B", BS)
def test_every_batch_size(eng, B):
    rng = np.random.default_rng(B)
    for N, q in ((167, 128), (97, 4096), (33, 2)):
        check(eng, N, q, ref.ternary(rng, N), rng.integers(0, q, (B, N)), paths=(4, 0))


def test_a_workgroup_takes_a_second_row_block(eng):
    """N = 64: the persistent grid is at most two workgroups per CU, so 32 (2 CUs + 1) + 5 rows give the first workgroup a second row
    block and end in a partial one.  The first row block holds the largest values: a running maximum or sum that is not started again
    shows in the second."""
    import torch
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    N, q = 64, 4096
    B = 32 * (2 * cus + 1) + 5
    rng = np.random.default_rng(64)
    rows = rng.integers(0, 3, (B, N)).astype(np.uint16)
    rows[:32] = rng.integers(q // 2 - 8, q // 2 + 8, (32, N))
    wp, _ = check(eng, N, q, ref.monomial(N, 3, 1), rows, paths=(0, 5, 4))
    assert wp[:32].min() >= q // 2 - 8 and wp[32:].max() <= 2


def test_every_alignment_with_guards_and_each_output_null(eng):
    """e and peak each on and 2 bytes off a 16-byte boundary, energy on and 8 bytes off; then each output NULL in turn."""
    N, q, B = 821, 4096, 33
    rng = np.random.default_rng(8)
    f, e = ref.ternary(rng, N), rng.integers(0, q, (B, N))
    wanted = ref.want(N, q, f, e)
    for k in range(8):
        check(eng, N, q, f, e, paths=(0,), shifts=(k & 1, (k >> 1) & 1, (k >> 2) & 1), tag=k, wanted=wanted)
    for outputs in ((True, False), (False, True)):
        check(eng, N, q, f, e, paths=(0, 5), outputs=outputs, wanted=wanted, shifts=(1, 1, 1))
        check(eng, 167, 128, ref.ternary(rng, 167), rng.integers(0, 128, (65, 167)), paths=(4, 1), outputs=outputs, shifts=(1, 1, 1))


# ---- the slow route ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("N,q,paths", [(167, 128, (1, 2, 3)), (167, 65536, (0,)), (1025, 4096, (0,)), (1920, 16384, (0,))])
def test_the_slow_route(eng, N, q, paths):
    rng = np.random.default_rng(N + q)
    assert not ref.matrix_range(N, q, paths[0])
    check(eng, N, q, ref.ternary(rng, N), rng.integers(0, q, (33, N)), paths=paths, tag="random")
    rows, wanted = planted_rows(N, q, 11, -1)
    got = check(eng, N, q, ref.monomial(N, 11, -1), rows, paths=paths, tag="planted")
    assert got[0].tolist() == wanted[0].tolist() and got[1].tolist() == wanted[1].tolist()
    try:
        eng.set_kernel_path(paths[0])
        noise_dev(eng, N, q, ref.monomial(N, 0, 1), rows[:2])
        name = eng.last_kernel()
        assert name.startswith("noise_rows(k_decrypt") and name.endswith(")"), name
    finally:
        eng.set_kernel_path(0)


def test_the_slow_route_in_several_passes(eng):
    """65536 + 3 rows at N = 2: two passes through scratch, the last one ragged."""
    N, q, B = 2, 4096, ref.PASS + 3
    rng = np.random.default_rng(2)
    check(eng, N, q, np.array([1, -1], np.int8), rng.integers(0, q, (B, N)), paths=(0,))


# ---- packed rows ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("N,q,path", [(167, 128, 0), (821, 4096, 4), (33, 2048, 0), (167, 65536, 0), (167, 128, 2)])
def test_packed_forms_equal_the_dense_forms(eng, N, q, path):
    """ntru_pack_batch of the same rows with ones in every ignored field and bit, on both routes."""
    rng = np.random.default_rng(N + q + path)
    B = 65
    f, e = ref.ternary(rng, N), rng.integers(0, q, (B, N)).astype(np.uint16)
    packed = packed_ref.set_ignored_bits(q, N, pkg.pack_rows(eng, N, q, e))
    wanted = ref.want(N, q, f, e)
    check(eng, N, q, f, None, paths=(path,), packed=packed, wanted=wanted, shifts=(1, 1, 1))
    check(eng, N, q, f, None, paths=(path,), packed=packed, wanted=wanted, outputs=(False, True))
    try:
        eng.set_kernel_path(path)
        hp, he = pkg.noise_packed_batch(eng, N, q, f, packed)
        assert hp.tolist() == wanted[0].tolist() and he.tolist() == wanted[1].tolist()
    finally:
        eng.set_kernel_path(0)


def test_packed_rows_in_several_passes(eng):
    """More packed rows than a pass unpacks, on the matrix route: the second pass reuses the scratch rows and ends ragged."""
    N, q, B = 64, 4, ref.PASS + 33
    rng = np.random.default_rng(3)
    f, e = ref.ternary(rng, N), rng.integers(0, q, (B, N)).astype(np.uint16)
    check(eng, N, q, f, None, paths=(0,), packed=pkg.pack_rows(eng, N, q, e), wanted=ref.want(N, q, f, e))


# ---- the host forms ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("B", [3, 8197])                  # one chunk; several chunks, the last one ragged
def test_host_forms_equal_the_dev_forms(eng, B):
    rng = np.random.default_rng(B)
    lib = pkg.load_library()
    for N, q in ((17, 32), (97, 8192)):
        f, e = ref.ternary(rng, N), rng.integers(0, q, (B, N)).astype(np.uint16)
        dpk, den = noise_dev(eng, N, q, f, e)
        hp, he = pkg.noise_batch(eng, N, q, f, e)                                          # pageable arrays
        assert hp.tolist() == dpk.tolist() and he.tolist() == den.tolist(), (N, q, "pageable")
        hp, he = pkg.noise_batch(eng, N, q, f, e, want_energy=False)
        assert he is None and hp.tolist() == dpk.tolist()
        hp, he = pkg.noise_batch(eng, N, q, f, e, want_peak=False)
        assert hp is None and he.tolist() == den.tolist()
        pin_e, pin_p, pin_n = eng.pinned_empty((B, N), np.uint16), eng.pinned_empty((B,), np.uint16), eng.pinned_empty((B,), np.uint64)
        pin_e[:] = e
        pin_p[:], pin_n[:] = FILL16, FILL64
        ptr = lambda a: a.ctypes.data_as(C.c_void_p)
        eng._chk(lib.ntru_noise_batch(eng._h, N, q, ptr(f), ptr(pin_e), B, ptr(pin_p), ptr(pin_n)))
        assert pin_p.tolist() == dpk.tolist() and pin_n.tolist() == den.tolist(), (N, q, "pinned")
    assert pkg.noise_batch(eng, 17, 32, np.zeros(17, np.int8), np.zeros((0, 17), np.uint16))[0].shape == (0,)


# ---- what does not matter, and what is reported ----------------------------------------------------------------------------------------------
def test_the_lift_mode_changes_nothing(eng):
    rng = np.random.default_rng(5)
    for N, q, path in ((167, 128, 0), (33, 4096, 0)):
        f, e = ref.ternary(rng, N), rng.integers(0, q, (33, N))
        wanted = ref.want(N, q, f, e)
        for mode in ("reference", "centred"):
            with pkg.lift.using(eng, mode):
                check(eng, N, q, f, e, paths=(path,), wanted=wanted, tag=mode)


def test_the_launch_log_names_the_kernel(eng, tmp_path, monkeypatch):
    log = tmp_path / "launches.jsonl"
    monkeypatch.setenv("NTRU_LAUNCH_LOG", str(log))
    N, q, B = 167, 128, 5
    f, e = np.ones(N, np.int8), np.ones((B, N), np.uint16)
    noise_dev(eng, N, q, f, e)
    assert eng.last_kernel() == "k_noise_m"
    noise_dev(eng, N, q, f, e, outputs=(True, False))
    rec = [json.loads(line) for line in log.read_text().splitlines()]
    assert rec == [{"kernel": "k_noise_m", "N": N, "items": B, "bytes_per_item": 2 * N + 10},
                   {"kernel": "k_noise_m", "N": N, "items": B, "bytes_per_item": 2 * N + 2}]


# ---- the fixture of the unmodified reference -------------------------------------------------------------------------------------------------
def test_fixture_through_the_reference_style_method(eng):
    inside = outside = 0
    for st in ref.load_sets():
        o = st["options"]
        N, q = o["N"], o["q"]
        ntru = pkg.NTRU({k: o[k] for k in ("N", "q", "p", "df", "dg", "dr")}, engine=eng)
        ntru.f = list(st["f"])
        rows = np.array([c["e"] for c in st["cases"]], np.uint16)
        wp, we = ref.reduce_rows(np.array([c["remainder1"] for c in st["cases"]]), q)
        for path in (0, 4, 1):
            try:
                eng.set_kernel_path(path)
                got = ntru.noiseBatch(rows)
                via_packed = ntru.noiseBatch(pkg.pack_rows(eng, N, q, rows), packed=True)
            finally:
                eng.set_kernel_path(0)
            for g in (got, via_packed):
                assert g["peak"].tolist() == wp.tolist() and g["energy"].tolist() == we.tolist(), (st["set"], path)
                assert g["margin"].tolist() == [q // 2 - int(x) for x in wp]
        for c, pk, en in zip(st["cases"], wp, we):
            A = np.array(c["A"], np.int64)
            if c["inside"]:
                inside += 1
                assert int(pk) == int(np.abs(A).max()) and int(en) == int((A * A).sum()), (st["set"], c["K"])
            else:
                outside += 1
    assert inside >= 8 and outside >= 2


# ---- Node ---------------------------------------------------------------------------------------------------------------------------------
NODE = shutil.which("node")


@pytest.mark.skipif(NODE is None, reason="node is not installed")
def test_shim_noise():
    ge.build()
    r = subprocess.run([NODE, os.path.join(ge.ROOT, "tests", "js", "shim_noise.mjs")], cwd=ge.ROOT, capture_output=True, text=True,
                       timeout=600)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    assert "shim_noise: 4 sets, 16 rows" in r.stdout
