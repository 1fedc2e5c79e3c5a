"""Restatement of the mix order drawn on the device (include/ntru_engine.h "drawing the mix order") and of a whole mix step from a key:
the checker the GPU tests of permutation.hip use, built from the oracle's ChaCha20 block function and sampler and from
tests/mix_ref.py, tied to both by tests/test_shuffle_cpu.py.  Not a test module."""
import numpy as np

import mix_ref
from oracle import ntru_oracle as orc

PERM_NONCE2 = 0x5045524D          # "PERM"


def perm_keys(key, perm_id, B):
    """k_i = w[2 j] | w[2 j + 1] << 32, j = i mod 8, w = the ChaCha20 block under `key`, counter i // 8, nonce (lo, hi, "PERM")."""
    nonce = [perm_id & 0xFFFFFFFF, (perm_id >> 32) & 0xFFFFFFFF, PERM_NONCE2]
    blocks = [orc.chacha20_block(key, c, nonce) for c in range((B + 7) // 8)]
    w = np.concatenate(blocks).astype(np.uint64) if blocks else np.zeros(0, np.uint64)
    return (w[0::2] | (w[1::2] << np.uint64(32)))[:B]


def argsort_inverse(keys):
    """(src, dst): the stable ascending argsort of the keys and its inverse, int64."""
    src = np.argsort(np.asarray(keys, np.uint64), kind="stable").astype(np.int64)
    dst = np.empty_like(src)
    dst[src] = np.arange(src.size, dtype=np.int64)
    return src, dst


def permutation(key, perm_id, B):
    return argsort_inverse(perm_keys(key, perm_id, B))


def mix(N, q, p, h, key, first_item, n1, n2, perm_id, e_in):
    """(e_out, quotE, r, src) of one mix step from a key."""
    e_in = np.asarray(e_in).reshape(-1, N)
    B = e_in.shape[0]
    r = orc.sample_ternary_batch(N, n1, n2, p - 1, key, first_item, B)
    src = permutation(key, perm_id, B)[0]
    e_out, quot = mix_ref.reencrypt(N, q, h, r, e_in, src)
    return e_out, quot, r, src
