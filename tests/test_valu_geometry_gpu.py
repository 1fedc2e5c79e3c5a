"""The vector-ALU families (csrc/valu_families.hip) across their lane geometries: every output against the oracle, bit for bit, at the N
where the geometry derived from N changes (tests/valu_geometry.py: every number of lanes per item at which several items share a
wave, idle lanes, the four fills of an item's last lane at the narrowest, a middle and the two widest items of every K, the ends of
every K range, the shared stepping's 32-lane stretches), at kernel paths 1-3 and at path 0 wherever no matrix-core kernel applies.

Each call must launch the kernel valu_geometry.expected_last names, leave the GUARD bytes around every output untouched (a last lane
that stores one element past N writes there, or into the next row, which then differs from the oracle; an element left unwritten
keeps its FILL bytes and differs too), and equal the references tests/test_kernel_variants_gpu.py uses: oracle.ntru_oracle's *_batch,
and tests/lift_ref.py for decrypt's centred mode (every decrypt call runs in both lift modes).  No call may be refused: the sweep
builds none that the ABI's documented rules refuse (valu_geometry.accepted; verify_keys with p (q - 1) > 65535 among them), and an
EngineError fails the test."""
import numpy as np
import pytest

import kernel_variants as kv
import valu_geometry as vg
from variant_runners import (assert_equal, pkg, run_decrypt, run_encrypt, run_polymul_split, run_public_key, run_verify_keys)

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def eng():
    e = pkg.Engine(0)
    yield e
    e.close()


def run_call(eng, entry, c, memo):
    """One call of the sweep.  The operands depend on the call's parameters but not on its kernel path, so that `memo` computes the
    reference of operands sent down several paths once."""
    N, q, p, B, variant = c["N"], c["q"], c["p"], c["B"], c["variant"]
    rng = np.random.default_rng([vg.ENTRIES.index(entry), N, q, p, B, variant])
    opts = dict(guard=True, memo=memo)
    if entry == "encrypt":
        return run_encrypt(eng, N, q, B, rng, variant, **opts)
    if entry == "decrypt":
        return run_decrypt(eng, N, q, p, B, rng, variant, witness=c["witness"], **opts)
    if entry == "verify_keys":
        return run_verify_keys(eng, N, q, p, B, rng, variant, **opts)
    if entry == "polymul_split":
        return run_polymul_split(eng, N, q, B, rng, variant, **opts)
    return run_public_key(eng, N, q, p, B, rng, variant, **opts)


def sweep(eng, entry, K):
    """Every call of valu_geometry.calls(entry, K).  A call that differs from its reference, launches another kernel or touches a guard
    is noted and the sweep goes on, so that a failure lists every case it concerns; an EngineError ends it."""
    calls = vg.calls(entry, K)
    assert calls, (entry, K)
    memo, failures = {}, []
    try:
        for c in calls:
            eng.set_kernel_path(c["path"])
            try:
                got, want = run_call(eng, entry, c, memo)
                assert eng.last_kernel() == c["last"], ("launched", eng.last_kernel())
                assert_equal(got, want, "outputs")
            except AssertionError as exc:
                failures.append((entry, c, str(exc)[:300]))
    finally:
        eng.set_kernel_path(0)
    assert not failures, (len(failures), "of", len(calls), "calls; the first:", failures[:6])


KS = sorted(kv.K_RANGES)


@pytest.mark.parametrize("K", KS)
def test_encrypt_across_geometries(eng, K):
    sweep(eng, "encrypt", K)


@pytest.mark.parametrize("K", KS)
def test_decrypt_across_geometries(eng, K):
    """p = 3 with every witness array and, at one batch size, the value alone; p = 5 on the multiply-accumulate path."""
    sweep(eng, "decrypt", K)


@pytest.mark.parametrize("K", KS)
def test_verify_keys_across_geometries(eng, K):
    """p = 3 and p = 5; where a wave holds several items at least seven, so that the flag kinds meet in one wave."""
    sweep(eng, "verify_keys", K)


@pytest.mark.parametrize("K", KS)
def test_polymul_split_across_geometries(eng, K):
    """Powers of two and modulus 3, the finish that is no power of two."""
    sweep(eng, "polymul_split", K)


@pytest.mark.parametrize("K", KS)
def test_public_key_across_geometries(eng, K):
    """p = 3 and p = 8."""
    sweep(eng, "public_key", K)
