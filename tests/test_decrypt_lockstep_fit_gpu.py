"""The lock-step decrypt kernel (k_decrypt_m8) where its LDS stops fitting: two groups' stages, the shared mod-p tables of
product 2, three key arrays (f, fp, 64 f) and the lift table.  At q = 4096 and 8192 the last N that fits is 864 (27 column
tiles), at q <= 2048 it is 896; beyond, the launcher falls back to k_decrypt_m.  Every case is checked against the CPU oracle."""
import numpy as np
import pytest

import __graft_entry__ as ge
from oracle import ntru_oracle as orc

pytestmark = pytest.mark.gpu
pkg = ge.load_package()


@pytest.fixture(scope="module")
def eng():
    return pkg.Engine(0)


def ternary(rng, N, n1, n2, two):
    out = np.zeros(N, np.int64)
    perm = rng.permutation(N)
    out[perm[:n1]] = 1
    out[perm[n1:n1 + n2]] = two
    return out


@pytest.mark.parametrize("path", [0, 5])
@pytest.mark.parametrize("N,q,m8", [(833, 8192, True), (863, 4096, True), (864, 8192, True), (864, 4096, True),
                                    (865, 4096, False), (866, 8192, False), (896, 2048, True),
                                    (896, 4096, False), (897, 2048, False)])
def test_lockstep_decrypt_either_side_of_lds_fit(eng, N, q, m8, path):
    rng = np.random.default_rng(N * 7 + q + path)
    p, d = 3, N // 3
    f = ternary(rng, N, d + 1, d, -1)
    fp = rng.integers(0, p, N)
    eng.set_kernel_path(path)
    try:
        for B in (70, 32 * 3):                           # a ragged last row block; an odd row-block count (one group idles)
            e = rng.integers(0, q, (B, N))
            e[0, :4] = (q - 1, 0, q // 2, q // 2 + 1)
            got = eng.decrypt_batch(N, q, p, f, fp, e)
            assert eng.last_kernel() == ("k_decrypt_m8" if m8 else "k_decrypt_m"), (N, q, path)
            want = orc.decrypt_batch(N, q, p, f, fp, e)
            for g_, w_, name in zip(got, want, ("value", "quotient1", "remainder1", "quotient2")):
                assert np.array_equal(g_, w_), (N, q, B, path, name)
    finally:
        eng.set_kernel_path(0)
