"""The contraction steps of a strip that do not fill a block of NT_S steps (toeplitz_strip, csrc/matrix_common.h).  Above the
diagonal they are the LAST sub-steps of a block whose fragment window is loaded already rotated; below it they are the first
sub-steps of a block that is never finished.  What can go wrong is a combination of (strip width NT_S, kb0 mod NT_S, steps left
below the diagonal mod NT_S), so the sizes here are chosen by tile count: every combination that for_each_strip can hand out is
reached (asserted below), at every q with its own digit planes, at batch sizes of one row, a ragged second row block and a third.
Every output array of every shared-key matrix kernel is compared bit for bit with the CPU oracle, and k_decrypt_m8 with
k_decrypt_m."""
import numpy as np
import pytest

import __graft_entry__ as ge
import mix_ref
import variant_runners as vr
from oracle import ntru_oracle as orc

pkg = ge.load_package()
gpu = pytest.mark.gpu

# the sizes the schedule was written against, and four more for the combinations they leave out (7, 13, 17 and 29 column tiles;
# 13 has what 29 has, at a size the lock-step kernel still takes)
SIZES = [33, 65, 97, 129, 161, 225, 289, 353, 417, 481, 545, 609, 673, 701, 737, 821, 864, 896, 1024] + [193, 385, 513, 897]
MODULI = [2048, 4096, 8192]              # 8192: the signed digit planes of encrypt
BATCHES = [1, 33, 70]
WAVES = 4


def strips(NT, maxt=4):
    """for_each_strip: (kb0, nt) of every non-empty strip of a row of NT column tiles."""
    rounds = ((NT + maxt - 1) // maxt + WAVES - 1) // WAVES
    n = rounds * WAVES
    base, rem = NT // n, NT % n
    return [(j * base + min(j, rem), base + (j < rem)) for j in range(n) if base + (j < rem) > 0]


def triples(NT):
    """(NT_S, steps above the diagonal mod NT_S -- None where there are none and the diagonal block comes first --, steps below mod NT_S)"""
    return {(nt, kb0 % nt if kb0 else None, (NT - kb0 - nt) % nt) for kb0, nt in strips(NT)}


def test_sizes_reach_every_strip_combination():
    reachable = set().union(*(triples(NT) for NT in range(1, 33)))            # N <= 1024
    covered = set().union(*(triples((N + 31) // 32) for N in SIZES))
    assert all(1 <= nt <= 4 for nt, _, _ in reachable)
    assert covered == reachable, sorted(reachable - covered, key=repr)
    # the lock-step kernel stops fitting at 27 / 28 column tiles: what it can reach is covered by sizes it takes
    m8 = set().union(*(triples(NT) for NT in range(1, 28)))
    assert set().union(*(triples((N + 31) // 32) for N in SIZES if N <= 864)) == m8


@pytest.fixture(scope="module")
def eng():
    e = pkg.Engine(0)
    yield e
    e.set_kernel_path(0)


def m8_fits(N, q):
    return N <= (896 if q <= 2048 else 864)      # tests/test_decrypt_lockstep_fit_gpu.py


@gpu
@pytest.mark.parametrize("q", MODULI)
@pytest.mark.parametrize("N", SIZES)
def test_encrypt_and_decrypt_equal_oracle_on_both_paths(eng, N, q):
    memo, p = {}, 3
    try:
        for B in BATCHES:
            # the runners' key variants: h all q - 1 (the largest accumulators) with f all ones, then random h with random f and fp
            for h_variant, variant in ((0, 1), (1, 2)):
                dec = {}
                for path in (4, 5):
                    eng.set_kernel_path(path)
                    ctx = (N, q, B, variant, path)
                    got, want = vr.run_encrypt(eng, N, q, B, np.random.default_rng(N + q + B + variant), h_variant, witness=True, memo=memo)
                    # (N = 1024: rows of r that start at a dword boundary, as these do, still fit one direct-to-LDS instruction)
                    assert eng.last_kernel() == ("k_encrypt_m" if path == 4 else "k_encrypt_md"), (ctx, eng.last_kernel())
                    vr.assert_equal(got, want, ("encrypt",) + ctx)
                    got, want = vr.run_decrypt(eng, N, q, p, B, np.random.default_rng(N + q + B + variant), variant, witness=True, memo=memo)
                    assert eng.last_kernel() == ("k_decrypt_m8" if path == 5 and m8_fits(N, q) else "k_decrypt_m"), (ctx, eng.last_kernel())
                    vr.assert_equal(got, want, ("decrypt",) + ctx)
                    dec[path] = got
                for a, b in zip(dec[4], dec[5]):
                    assert a.tobytes() == b.tobytes(), (N, q, B, variant, "k_decrypt_m8 against k_decrypt_m")
    finally:
        eng.set_kernel_path(0)


@gpu
@pytest.mark.parametrize("path", [4, 5])
def test_pitched_rows(eng, path):
    """ld = N rounded up to 64: pads of the inputs hold garbage, pads of the outputs and the row behind the batch stay as they were."""
    N, q, p, B = 609, 8192, 3, 70
    ld = (N + 63) // 64 * 64
    rng = np.random.default_rng(ld + path)
    h = rng.integers(0, q, N).astype(np.uint16)
    r, m = rng.integers(0, 3, (B, N)).astype(np.uint8), rng.integers(0, 3, (B, N)).astype(np.uint8)
    f, fp = vr.decrypt_key(rng, N, p, 2)
    e_o, quot_o = orc.encrypt_batch(N, q, h, r, m)
    want = orc.decrypt_batch(N, q, p, f, fp, e_o)

    def pitched(a, dtype):
        buf = rng.integers(0, 1 << (8 * np.dtype(dtype).itemsize), (B + 1, ld)).astype(dtype)
        buf[:B, :N] = a
        return buf

    def check(d, ptr, dtype, rows, what):
        a = d.get(ptr, (B + 1, ld), dtype)
        fill = np.uint8(vr.FILL) if dtype == np.uint8 else np.uint16(vr.FILL * 0x0101)
        assert np.array_equal(a[:B, :N], rows), (what, path)
        assert (a[:B, N:] == fill).all() and (a[B:] == fill).all(), (what, path, "wrote outside the rows")

    eng.set_kernel_path(path)
    try:
        with vr.Dev(eng) as d:
            de, dq = d.out((B + 1, ld), np.uint16), d.out((B + 1, ld), np.uint16)
            eng.encrypt_batch_dev(N, q, d.up(h), d.up(pitched(r, np.uint8)), d.up(pitched(m, np.uint8)), B, de, dq, ld=ld)
            assert eng.last_kernel() == ("k_encrypt_m" if path == 4 else "k_encrypt_md")
            check(d, de, np.uint16, e_o, "e"); check(d, dq, np.uint16, quot_o, "quotE")
            outs = [d.out((B + 1, ld), dt) for dt in (np.uint8, np.uint16, np.uint16, np.uint8)]
            eng.decrypt_batch_dev(N, q, p, d.up(f), d.up(fp), d.up(pitched(e_o, np.uint16)), B, *outs, ld=ld)
            assert eng.last_kernel() == ("k_decrypt_m" if path == 4 else "k_decrypt_m8")
            for o, dt, w, name in zip(outs, (np.uint8, np.uint16, np.uint16, np.uint8), want, ("value", "quotient1", "remainder1", "quotient2")):
                check(d, o, dt, w, name)
    finally:
        eng.set_kernel_path(0)


def mp_fits(N, q):
    """ntru_launch_decrypt_pack_matrix's conditions (csrc/matrix_decrypt.hip)."""
    NT = (N + 31) // 32
    pitchA, tpitch = 32 * NT + 16, (16 * NT + 31) // 32 * 32 + 8
    out_size = orc.pack_params(2, N)["outputSize"]
    lds = 32 * tpitch + 64 * pitchA + 256 * NT + ((q + 15) & ~15)
    m3_end = ((((4 * N + 4) & ~3) + 4 * N + 1 + 15) & ~15)
    img = (8 * (126 * out_size + 16) + 15) & ~15
    return lds <= 160 * 1024 and m3_end + img <= 32 * pitchA and 126 * out_size + 16 >= 32 * NT


@gpu
@pytest.mark.parametrize("N", SIZES)
def test_fused_decrypt_and_pack(eng, N):
    q = MODULI[N % 3]
    fused = mp_fits(N, q)                      # beyond its LDS: decrypt, then pack (the value array is the intermediate)
    eng.set_kernel_path(5)
    try:
        for B in (1, 70):
            got, want = vr.run_decrypt_pack(eng, N, q, 3, B, np.random.default_rng(N + B), 2, fused=fused)
            if fused:
                assert eng.last_kernel() == "k_decrypt_mp", (N, q, B, eng.last_kernel())
            vr.assert_equal(got, want, ("decrypt_pack", N, q, B))
    finally:
        eng.set_kernel_path(0)


def test_fused_decrypt_covers_the_combinations_it_can_reach():
    """k_decrypt_mp is taken wherever its LDS fits: the sizes it takes reach every combination that range holds."""
    taken = [N for N in SIZES if mp_fits(N, MODULI[N % 3])]
    top = max((N + 31) // 32 for N in taken)
    assert top >= 26                                                          # N = 821 and beyond
    assert set().union(*(triples((N + 31) // 32) for N in taken)) >= set().union(*(triples(NT) for NT in range(1, top + 1)))


@gpu
@pytest.mark.parametrize("N", SIZES)
def test_reencrypt_identity_and_shuffled(eng, N):
    q, B = MODULI[(N + 1) % 3], 70
    rng = np.random.default_rng(N)
    h = rng.integers(0, q, N)
    r = rng.integers(0, 3, (B, N))
    e_in = rng.integers(0, q, (B + 5, N))
    shuffled = rng.integers(0, B + 5, B)                                       # repeats, and rows of e_in that no output takes
    try:
        for src in (None, np.arange(B), shuffled):
            want_e, want_q = mix_ref.reencrypt(N, q, h, r, e_in, src)
            for path, kernel in ((5, "k_reencrypt_md"), (4, "k_reencrypt_m")):      # (N = 1024: rows of r at a dword boundary still fit the DMA)
                eng.set_kernel_path(path)
                e, quot = pkg.mix.reencrypt_batch(eng, N, q, h, r, e_in, src=src)
                assert eng.last_kernel() == kernel, (N, q, path, eng.last_kernel())
                ctx = (N, q, path, None if src is None else "identity" if src is not shuffled else "shuffled")
                vr.assert_equal([np.asarray(e), np.asarray(quot)], [np.asarray(want_e), np.asarray(want_q)], ("reencrypt",) + ctx)
    finally:
        eng.set_kernel_path(0)
