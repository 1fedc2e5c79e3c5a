"""CPU replay of ntru_keygen_batch's documented stream positions (include/ntru_engine.h) on oracle.ntru_oracle's sampler and
oracle.ntru_keygen's inverses.  Not a test module: imported by tests/test_keygen_gpu.py and tests/variant_runners.py."""
import numpy as np

from oracle import ntru_keygen as kg
from oracle import ntru_oracle as orc


def replay(N, df, dg, key, first, B, max_tries):
    """The contract, item by item, on the CPU: (f, g, tries, flags)."""
    g = orc.sample_ternary_batch(N, dg, dg, 255, key, (1 << 40) + first, B).view(np.int8)
    f = orc.sample_ternary_batch(N, df, df - 1, 255, key, first, B).view(np.int8).copy()
    tries = np.zeros(B, np.uint8)
    flags = np.zeros(B, np.uint8)
    for b in range(B):
        for t in range(max_tries):
            row = f[b] if t == 0 else orc.sample_ternary_batch(N, df, df - 1, 255, key, (t << 44) + first + b, 1).view(np.int8)[0]
            fl = (0 if kg.is_unit(row, N, 2) else 8) | (0 if kg.is_unit(row, N, 3) else 16)
            f[b], tries[b], flags[b] = row, t + 1, fl
            if not fl:
                break
    return f, g, tries, flags


def key_pairs(N, q, df, dg, key, first, B, max_tries):
    """replay() plus the inverses and the public key of every item that drew a unit (zero rows elsewhere), p = 3:
    {f, g, fq, fp, h, tries, flags}."""
    f, g, tries, flags = replay(N, df, dg, key, first, B, max_tries)
    fq, fp = np.zeros((B, N), np.int64), np.zeros((B, N), np.int64)
    for b in np.nonzero(flags == 0)[0]:
        a, c = kg.load_private_key(f[b], N, q, 3)
        fq[b], fp[b] = np.mod(a, q), np.mod(c, 3)
    h = orc.public_key_batch(N, q, 3, fq.astype(np.uint16), g)
    h[flags != 0] = 0
    return {"f": f, "g": g, "fq": fq.astype(np.uint16), "fp": fp.astype(np.uint8), "h": h, "tries": tries, "flags": flags}
