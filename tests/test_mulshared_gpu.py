"""ntru_mul_shared_batch[_dev] on the GPU, bytes against bytes: the oracle's polymul_split_batch on s repeated per row, across every
strip geometry of k_mul_shared_m, every operand kind that sits on an edge of its digit planes, kernel paths 0, 4 and 5, the replicated
route for everything outside the matrix range, two exact cross-checks against the shared-key decrypt and encrypt kernels, every
alignment between guard bytes, the host form against the _dev form, and the fixture of the unmodified reference."""
import ctypes as C
import os
import shutil
import subprocess

import numpy as np
import pytest

import __graft_entry__ as ge
import mulshared_ref as ref

pytestmark = pytest.mark.gpu
pkg = ge.load_package()
GUARD = 64            # guard elements on either side of quot and rem
FILL = 0xA5C3
NS = [2, 31, 32, 33, 63, 64, 65, 127, 128, 129, 167, 509, 821, 1023, 1024]
MODS = [2, 128, 4096, 8192]
BS = [1, 31, 32, 33, 65]


@pytest.fixture(scope="module")
def eng():
    e = pkg.Engine(0)
    yield e
    e.set_kernel_path(0)


def mul_dev(eng, N, mod, s, rows, want_quot=True, shifts=(0, 0, 0, 0)):
    """ntru_mul_shared_batch_dev on device copies; s, rows, quot and rem `shifts` elements (2 bytes each) off a 256-byte boundary.  The
    inputs end with their allocation; quot and rem lie between guard elements, which must survive.  Returns (quot or None, rem)."""
    rows = np.ascontiguousarray(rows, np.uint16).reshape(-1, N)
    B = rows.shape[0]
    held = []

    def put(a, shift):
        a = np.ascontiguousarray(a)
        p = eng.dev_alloc(2 * shift + max(a.nbytes, 2))
        held.append(p)
        if a.nbytes:
            eng.dev_upload(p + 2 * shift, a)
        return p + 2 * shift
    try:
        d_s, d_rows = put(np.asarray(s, np.uint16), shifts[0]), put(rows, shifts[1])
        frames = [np.full(GUARD + sh + B * N + GUARD, FILL, np.uint16) for sh in shifts[2:]]
        d_frames = [put(f, 0) for f in frames]
        at = [d + 2 * (GUARD + sh) for d, sh in zip(d_frames, shifts[2:])]
        pkg.mul_shared_batch_dev(eng, N, mod, d_s, d_rows, B, at[0] if want_quot else None, at[1])
        out = []
        for k, (d, f, sh) in enumerate(zip(d_frames, frames, shifts[2:])):
            got = eng.dev_download(d, f.shape, np.uint16)
            lo = GUARD + sh
            assert (got[:lo] == FILL).all() and (got[lo + B * N:] == FILL).all(), "guard elements around %s were written" % ("quot", "rem")[k]
            body = got[lo:lo + B * N].reshape(B, N)
            if k == 0 and not want_quot:
                assert (body == FILL).all(), "quot was written though it was not asked for"
                body = None
            out.append(body)
        return out
    finally:
        eng.synchronize()
        for p in held:
            eng.dev_free(p)


def check(eng, N, mod, s, rows, paths=(0, 4, 5), tag=None, **kw):
    wq, wr = ref.want(N, mod, s, rows)
    try:
        for path in paths:
            eng.set_kernel_path(path)
            quot, rem = mul_dev(eng, N, mod, s, rows, **kw)
            assert eng.last_kernel().startswith(ref.kernel_of(N, mod, path)), (tag, N, mod, path, eng.last_kernel())
            assert rem.tobytes() == wr.tobytes(), (tag, N, mod, path, "rem")
            assert quot is None or quot.tobytes() == wq.tobytes(), (tag, N, mod, path, "quot")
    finally:
        eng.set_kernel_path(0)


# ---- geometries and operands -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("N", NS)
def test_every_strip_geometry_with_every_operand_kind(eng, N):
    """One tile, a partial tile, every strip count, two rounds of strips (821); the modulus and the batch size cycle with N, so that every
    value of both is met, and every operand kind runs on kernel paths 0, 4 and 5 (path 0 below N = 64: the replicated route)."""
    i = NS.index(N)
    rng = np.random.default_rng(100 + N)
    for k in range(2):
        mod, B = MODS[(i + k) % len(MODS)], BS[(i + 2 * k) % len(BS)]
        for label, s, rows in ref.operand_sets(N, mod, B, rng):
            check(eng, N, mod, s, rows, tag=label)


def test_the_axes_cycle_through_every_value():
    met = [(MODS[(i + k) % len(MODS)], BS[(i + 2 * k) % len(BS)]) for i in range(len(NS)) for k in range(2)]
    assert {m for m, _ in met} == set(MODS) and {b for _, b in met} == set(BS)


@pytest.mark.parametrize("mod", MODS)
def test_every_modulus_with_every_batch_size(eng, mod):
    rng = np.random.default_rng(mod)
    for N in (167, 33):
        for B in BS:
            check(eng, N, mod, ref.edge_s(N, mod, rng), rng.integers(0, mod, (B, N)), paths=(4, 0))


def test_a_workgroup_takes_a_second_row_block(eng):
    """N = 64: the persistent grid is at most two workgroups per CU, so 32 (2 CUs + 1) + 5 rows give the first workgroup a second row
    block and end in a partial one."""
    import torch
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    N, mod = 64, 4096
    B = 32 * (2 * cus + 1) + 5
    rng = np.random.default_rng(64)
    check(eng, N, mod, ref.edge_s(N, mod, rng), rng.integers(0, mod, (B, N)), paths=(0, 5))


def test_without_the_quotient(eng):
    rng = np.random.default_rng(9)
    for N, mod, B in ((821, 4096, 33), (65, 8192, 65), (167, 65536, 5), (17, 3, 4)):
        check(eng, N, mod, rng.integers(0, mod, N), rng.integers(0, mod, (B, N)), paths=(0, 4, 1), want_quot=False)


def test_every_alignment_with_guards(eng):
    """s, rows, quot and rem each on and 2 bytes off a 16-byte boundary."""
    N, mod, B = 821, 4096, 33
    rng = np.random.default_rng(8)
    s, rows = ref.edge_s(N, mod, rng), rng.integers(0, mod, (B, N))
    for k in range(16):
        check(eng, N, mod, s, rows, paths=(0,), shifts=(k & 1, (k >> 1) & 1, (k >> 2) & 1, (k >> 3) & 1), tag=k)
    check(eng, 167, 128, ref.edge_s(167, 128, rng), rng.integers(0, 128, (65, 167)), paths=(4, 1), shifts=(1, 1, 1, 1))


# ---- outside the matrix range ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("N,mod,paths", [(167, 128, (1, 2, 3)), (167, 65536, (0, 4)), (167, 3, (0, 4, 1)), (1025, 4096, (0, 5)),
                                         (1920, 16384, (0,))])
def test_the_replicated_route(eng, N, mod, paths):
    rng = np.random.default_rng(N + mod)
    for label, s, rows in ref.operand_sets(N, mod, 33, rng):
        check(eng, N, mod, s, rows, paths=paths, tag=label)
        assert not ref.matrix_range(N, mod, paths[0])


def test_the_replicated_route_in_several_passes(eng):
    """More rows than a pass replicates s for: the second pass reuses the replicated rows and ends ragged."""
    N, mod, B = 2, 3, ref.FALLBACK_PASS + 3
    rng = np.random.default_rng(2)
    check(eng, N, mod, rng.integers(0, mod, N), rng.integers(0, mod, (B, N)), paths=(0,))
    check(eng, N, 4096, rng.integers(0, 4096, N), rng.integers(0, 4096, (B, N)), paths=(1,), want_quot=False)


# ---- cross-checks against the shared-key kernels: exact identities, whatever the noise -----------------------------------------------------
@pytest.mark.parametrize("N,q", [(167, 128), (821, 4096)])
def test_equals_product_1_of_decrypt_and_the_product_of_encrypt(eng, N, q):
    rng = np.random.default_rng(N)
    B, p = 65, 3
    f = rng.integers(-1, 2, N).astype(np.int8)
    fp = rng.integers(0, p, N).astype(np.uint8)
    e = rng.integers(0, q, (B, N)).astype(np.uint16)
    _, quot1, rem1, _ = eng.decrypt_batch(N, q, p, f, fp, e)
    quot, rem = pkg.mul_shared_batch(eng, N, q, f.astype(np.int64) % q, e)
    assert quot.tobytes() == quot1.tobytes() and rem.tobytes() == rem1.tobytes()
    h = rng.integers(0, q, N).astype(np.uint16)
    r = rng.integers(0, p, (B, N)).astype(np.uint8)
    ct, quotE = eng.encrypt_batch(N, q, h, r, np.zeros((B, N), np.uint8))
    quot, rem = pkg.mul_shared_batch(eng, N, q, h, r.astype(np.uint16))
    assert quot.tobytes() == quotE.tobytes() and rem.tobytes() == ct.tobytes()


# ---- the host form ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("B", [3, 8197])                  # one chunk; four chunks of 2050, the last one ragged
def test_host_form_equals_the_dev_form(eng, B):
    rng = np.random.default_rng(B)
    lib = pkg.load_library()
    for N, mod in ((17, 32), (65, 8192)):
        s, rows = ref.edge_s(N, mod, rng), rng.integers(0, mod, (B, N)).astype(np.uint16)
        dq, dr = mul_dev(eng, N, mod, s, rows)
        hq, hr = pkg.mul_shared_batch(eng, N, mod, s, rows)                               # pageable arrays
        assert hq.tobytes() == dq.tobytes() and hr.tobytes() == dr.tobytes(), (N, mod, "pageable")
        _, hr2 = pkg.mul_shared_batch(eng, N, mod, s, rows, want_quot=False)
        assert hr2.tobytes() == dr.tobytes(), (N, mod, "pageable, no quot")
        pin = [eng.pinned_empty((B, N), np.uint16) for _ in range(3)]                     # ntru_host_alloc memory: DMA in place
        pin[0][:] = rows
        pin[1][:], pin[2][:] = FILL, FILL
        ptr = lambda a: a.ctypes.data_as(C.c_void_p)
        eng._chk(lib.ntru_mul_shared_batch(eng._h, N, mod, ptr(s), ptr(pin[0]), B, ptr(pin[1]), ptr(pin[2])))
        assert pin[1].tobytes() == dq.tobytes() and pin[2].tobytes() == dr.tobytes(), (N, mod, "pinned")
    assert pkg.mul_shared_batch(eng, 17, 32, np.zeros(17, np.uint16), np.zeros((0, 17), np.uint16))[1].shape == (0, 17)


def test_fixture_and_the_reference_style_method(eng):
    for st in ref.load_sets():
        N, q = st["N"], st["q"]
        rows = np.array(st["rows"], np.uint16)
        want_q = np.array([ref.pad(c["quotient"], N) for c in st["cases"]], np.uint16)
        want_r = np.array([ref.pad(c["remainder"], N) for c in st["cases"]], np.uint16)
        try:
            for path in (0, 4, 1):
                eng.set_kernel_path(path)
                quot, rem = pkg.mul_shared_batch(eng, N, q, st["s"], rows)
                assert quot.tobytes() == want_q.tobytes() and rem.tobytes() == want_r.tobytes(), (N, q, path)
        finally:
            eng.set_kernel_path(0)
        ntru = pkg.NTRU({"N": N, "q": q, "p": 3, "df": 1, "dg": 1, "dr": 1}, engine=eng)
        signed = [v - q if v > q // 2 else v for v in st["s"]]
        assert ntru.multiplyByPolynomialBatch(rows, signed).tobytes() == want_r.tobytes()
        got_q, got_r = ntru.multiplyByPolynomialBatch(rows, pkg.trimPolynomial(st["s"]), want_quot=True)
        assert got_q.tobytes() == want_q.tobytes() and got_r.tobytes() == want_r.tobytes()


def test_rotation_by_a_monomial(eng):
    """c = x^k rotates the coefficients: the plainest use of the product."""
    N, q, k = 167, 128, 5
    rows = np.random.default_rng(1).integers(0, q, (4, N)).astype(np.uint16)
    c = np.zeros(N, np.uint16)
    c[k] = 1
    _, rem = pkg.mul_shared_batch(eng, N, q, c, rows)
    assert np.array_equal(rem, np.roll(rows, k, axis=1))


def test_the_launch_log_names_the_kernel(eng, tmp_path, monkeypatch):
    import json
    log = tmp_path / "launches.jsonl"
    monkeypatch.setenv("NTRU_LAUNCH_LOG", str(log))
    N, mod, B = 167, 128, 5
    mul_dev(eng, N, mod, np.ones(N, np.uint16), np.ones((B, N), np.uint16))
    mul_dev(eng, N, mod, np.ones(N, np.uint16), np.ones((B, N), np.uint16), want_quot=False)
    rec = [json.loads(line) for line in log.read_text().splitlines()]
    assert rec == [{"kernel": "k_mul_shared_m", "N": N, "items": B, "bytes_per_item": 6 * N},
                   {"kernel": "k_mul_shared_m", "N": N, "items": B, "bytes_per_item": 4 * N}]


# ---- Node ---------------------------------------------------------------------------------------------------------------------------------
NODE = shutil.which("node")


@pytest.mark.skipif(NODE is None, reason="node is not installed")
def test_shim_mulshared():
    ge.build()
    r = subprocess.run([NODE, os.path.join(ge.ROOT, "tests", "js", "shim_mulshared.mjs")], cwd=ge.ROOT, capture_output=True, text=True,
                       timeout=600)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    assert "shim_mulshared: 4 sets, 10 rows" in r.stdout
