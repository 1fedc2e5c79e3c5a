"""Every compiled kernel instantiation (tests/kernel_variants.py) launched through its entry point and compared bit for bit with the
CPU oracle, on the operand values and batch sizes where kernels go wrong; p != 3 on every kernel that takes p; and a dispatch sweep
over every N of kernel paths 0-3, so that a launcher cannot ask for an instantiation that does not exist and, wherever
tests/valu_geometry.py predicts the kernel (every call at paths 1-3), launches that one.  The rows of the per-item scheme, the
segmented sums, the byte codec, the witness checks and key generation run against the references their own test modules use
(tests/peritem_ref.py, ciphertext_sum_ref.py, message_bytes_ref.py, witness_circuit.py, keygen_ref.py, packed_ref.py).  Every row of
the decrypt family runs each call in both lift modes: the default against the oracle, the centred one against tests/lift_ref.py.
The runners (one call of an entry point and its reference) live in tests/variant_runners.py, shared with
tests/test_valu_geometry_gpu.py, which checks the vector-ALU families' outputs at the N where their lane geometry changes."""
import numpy as np
import pytest

import kernel_variants as kv
import peritem_ref
import valu_geometry as vg
from variant_runners import (LIFT_DIFFERED, P3_ONLY, Dev, assert_equal, batch_sizes, decrypt_peritem_call, pkg, run_decrypt,
                             run_decrypt_pack, run_decrypt_peritem, run_public_key, run_shape, run_verify_keys)

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def eng():
    e = pkg.Engine(0)
    yield e
    e.close()


REACHABLE = [r for r in kv.ROWS if r["shapes"]]


@pytest.mark.parametrize("row", REACHABLE, ids=[r["kernel"] for r in REACHABLE])
def test_variant_row_equals_oracle(eng, row):
    rng = np.random.default_rng(sum(map(ord, row["kernel"])))
    try:
        for s in row["shapes"]:
            eng.set_kernel_path(s["path"])
            del LIFT_DIFFERED[:]
            for B in batch_sizes(row["kernel"], s):
                for variant in range(3):
                    got, want = run_shape(eng, row["entry"], s, B, rng, variant)
                    ctx = (row["kernel"], s, B, variant)
                    if row["last"]:
                        # the lock-step decrypt runs only with every witness array; value-only calls take k_decrypt_m
                        expect = "k_decrypt_m" if row["kernel"] == "k_decrypt_m8" and variant == 1 else row["last"]
                        assert eng.last_kernel() == expect, (ctx, eng.last_kernel())
                    if row["entry"] == "encrypt_pack":
                        assert eng.last_kernel() == "k_encrypt_wp", ctx
                    assert_equal(got, want, ctx)
            if row["entry"] in kv.LIFT_ENTRIES:
                # every call ran in both lift modes; at an addend other than 1 the shape's calls told them apart
                assert LIFT_DIFFERED and any(LIFT_DIFFERED) == (kv.lift_addend(s["q"], s["p"]) != 1), (row["kernel"], s, LIFT_DIFFERED)
    finally:
        eng.set_kernel_path(0)
        eng.set_sampler_rounds(20)


# ---- p != 3 ------------------------------------------------------------------------------------------------------------------------
P_MAX_N = {5: 1920, 7: 1820, 11: 655, 13: 455}          # the largest N with N (p - 1)^2 < 65536 (and N <= 1920)


def _not_p3_only(eng, ctx):
    assert not eng.last_kernel().startswith(P3_ONLY), (ctx, eng.last_kernel())
    assert eng.last_kernel() in kv.LAST_KERNELS, (ctx, eng.last_kernel())


@pytest.mark.parametrize("p", sorted(P_MAX_N))
def test_decrypt_and_verify_keys_p_sweep(eng, p):
    rng = np.random.default_rng(p)
    for N in (17, P_MAX_N[p]):
        for q in (2048, 8192, 65536):
            for variant in range(3):
                got, want = run_decrypt(eng, N, q, p, 3, rng, variant, witness=variant != 1)
                _not_p3_only(eng, ("decrypt", N, q, p))
                assert_equal(got, want, ("decrypt", N, q, p, variant))
        for q in sorted({2048, max(2 ** k for k in range(1, 17) if p * (2 ** k - 1) <= 65535)}):
            got, want = run_verify_keys(eng, N, q, p, 7, rng, 0)
            _not_p3_only(eng, ("verify_keys", N, q, p))
            assert_equal(got, want, ("verify_keys", N, q, p))


@pytest.mark.parametrize("p", sorted(P_MAX_N))
def test_decrypt_peritem_p_sweep(eng, p):
    """p != 3 with one key pair per item: the composed path, whatever N and q, on the edge operands of the per-row cases."""
    rng = np.random.default_rng(200 + p)
    for N in (17, P_MAX_N[p]):
        for q in (2048, 8192, 65536):
            for variant in range(3):
                got, want = run_decrypt_peritem(eng, N, q, p, 3, rng, variant)
                lk, ctx = eng.last_kernel(), ("decrypt_peritem", N, q, p, variant)
                assert lk.startswith("peritem_composed(") and lk.endswith(")"), (ctx, lk)
                inner = lk[len("peritem_composed("):-1]
                assert not inner.startswith(P3_ONLY) and inner in kv.LAST_KERNELS, (ctx, lk)
                assert_equal(got, want, ctx)


@pytest.mark.parametrize("N", [128, 1024])
def test_decrypt_peritem_unreduced_fp(eng, N):
    """fp bytes of 3, 128 and 255 in one item, inside one lane's 16-byte chunk: the ABI asks for fp in [0, p), and k_decrypt_pi_m
    carries a wave-wide branch that reduces such bytes.  Pinned: the result is that of fp % 3, and that of the composed path (kernel
    path 1) on the same bytes."""
    q, B = 2048, 5
    rng = np.random.default_rng(N)
    f, fp, e = peritem_ref.decrypt_operands(rng, N, q, 3, B, 2)
    fp[2] = rng.integers(0, 3, N)
    chunk = 16 * (N // 16 - 3)
    fp[2, chunk + 1], fp[2, chunk + 7], fp[2, chunk + 15] = 3, 128, 255
    assert (fp >= 3).sum() == 3
    want = list(peritem_ref.oracle_decrypt(N, q, 3, f, fp % 3, e))
    try:
        got = decrypt_peritem_call(eng, N, q, 3, f, fp, e)
        assert eng.last_kernel() == "k_decrypt_pi_m"
        reduced = decrypt_peritem_call(eng, N, q, 3, f, fp % 3, e)
        eng.set_kernel_path(1)
        composed = decrypt_peritem_call(eng, N, q, 3, f, fp, e)
        assert eng.last_kernel().startswith("peritem_composed("), eng.last_kernel()
    finally:
        eng.set_kernel_path(0)
    assert_equal(reduced, want, ("fp % 3", N))
    assert_equal(got, want, ("fp >= 3 on the matrix kernel", N))
    assert_equal(composed, want, ("fp >= 3 on the composed path", N))


@pytest.mark.parametrize("p", [1, 2, 4, 5, 7, 8])
def test_public_key_p_sweep(eng, p):
    rng = np.random.default_rng(100 + p)
    q = 8192
    try:
        for path, N, kernel in ((0, 509, "k_public_key_m"), (4, 64, "k_public_key_m"), (1, 509, "k_public_key<5>"),
                                (0, 101, "k_public_key<1>"), (0, 1920, "k_public_key<15>")):
            eng.set_kernel_path(path)
            for variant in range(3):
                got, want = run_public_key(eng, N, q, p, 3, rng, variant)
                assert eng.last_kernel() == kernel, (N, p, path, eng.last_kernel())
                assert_equal(got, want, ("public_key", N, q, p, path, variant))
    finally:
        eng.set_kernel_path(0)


def test_decrypt_pack_p5(eng):
    """packOutput with max 4 (3 bits per value) behind the vector-ALU decrypt: not the fused p == 3 kernel."""
    rng = np.random.default_rng(5)
    for N, q in ((17, 2048), (821, 4096), (1920, 8192)):
        for variant in range(3):
            got, want = run_decrypt_pack(eng, N, q, 5, 3, rng, variant, fused=False)
            _not_p3_only(eng, ("decrypt_pack", N, q))
            assert_equal(got, want, ("decrypt_pack", N, q, 5, variant))


# ---- dispatch sweep -------------------------------------------------------------------------------------------------------------
SWEEP_Q = (2048, 4096, 8192, 16384, 32768)
MAXN = 1920


def documented_refusal(entry, N, q, p):
    """Calls the ABI refuses by its documented rules: verify_keys needs p (q - 1) <= 65535."""
    return entry == "verify_keys" and p * (q - 1) > 65535


@pytest.mark.parametrize("entry", ["encrypt", "decrypt", "verify_keys", "polymul_split"])
def test_dispatch_sweep_every_n(eng, entry):
    """Every N from 2 to 1920 at kernel paths 0-3 and q 2048..32768, B = 1 or 2, device buffers sized for N = 1920: each call the ABI
    accepts returns NTRU_OK and launches a kernel of the variant table: the one tests/valu_geometry.py predicts from the launchers'
    rules wherever it predicts one, which is every call at paths 1-3 and, at path 0, every call outside the matrix-core kernels' range.
    Outputs are checked by the per-row cases and, across the lane geometries, by tests/test_valu_geometry_gpu.py."""
    B = 2
    z16, z8 = np.zeros(B * MAXN, np.uint16), np.zeros(B * MAXN, np.uint8)
    failed, unknown, wrong = [], set(), []
    p = 3 if entry in ("decrypt", "verify_keys") else 0
    with Dev(eng) as d:
        u16 = [d.up(z16) for _ in range(6)]
        u8 = [d.up(z8) for _ in range(6)]
        try:
            for N in range(2, MAXN + 1):
                b = 1 + N % 2
                for path in range(4):
                    eng.set_kernel_path(path)
                    for q in SWEEP_Q:
                        try:
                            if entry == "encrypt":
                                eng.encrypt_batch_dev(N, q, u16[0], u8[0], u8[1], b, u16[1], u16[2])
                            elif entry == "decrypt":
                                eng.decrypt_batch_dev(N, q, 3, u8[0], u8[1], u16[0], b, u8[2], u16[1], u16[2], u8[3])
                            elif entry == "verify_keys":
                                if documented_refusal(entry, N, q, 3):
                                    with pytest.raises(pkg.EngineError):
                                        eng.verify_keys_batch_dev(N, q, 3, u8[0], u8[1], u16[0], u8[2], u16[1], b, u16[2], u16[3],
                                                                  u8[3], u8[4], u16[4], u16[5], u8[5])
                                    continue
                                eng.verify_keys_batch_dev(N, q, 3, u8[0], u8[1], u16[0], u8[2], u16[1], b, u16[2], u16[3], u8[3],
                                                          u8[4], u16[4], u16[5], u8[5])
                            else:
                                eng.polymul_split_dev(N, q, u16[0], u16[1], b, u16[2], u16[3])
                        except pkg.EngineError as exc:
                            failed.append((N, q, path, str(exc)))
                            continue
                        if eng.last_kernel() not in kv.LAST_KERNELS:
                            unknown.add((eng.last_kernel(), N, q, path))
                        want = vg.expected_last(entry, N, q, p, path)
                        assert want is not None or path == 0, (N, q, path)
                        if want is not None and eng.last_kernel() != want:
                            wrong.append((N, q, path, eng.last_kernel(), want))
                eng.synchronize()
        finally:
            eng.set_kernel_path(0)
    assert not failed, (len(failed), failed[:12])
    assert not unknown, sorted(unknown)[:12]
    assert not wrong, (len(wrong), wrong[:12])
