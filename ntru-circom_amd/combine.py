"""Combining ciphertexts by a weight matrix (include/ntru_engine.h "combining ciphertexts"): G linear combinations of the same B rows
in one device pass, out = weights^T . rows modulo mod -- the weights of sum_groups widened to G columns.  Functions on an Engine: its
class keeps the methods it had."""
import numpy as np

from .engine import _np, _ptr

MAX_G = 4096          # NTRU_COMBINE_MAX_G


def combine_batch(eng, N, mod, rows, weights):
    """rows [B][N] uint16 below mod, weights [B][G] uint16 below mod (row b: the G weights of row b; a flat sequence of B weights is
    one column).  Returns out [G][N] uint16, out[g] = (sum over b of weights[b][g] * rows[b]) % mod: row g is what
    Engine.sum_groups(N, mod, rows, weights=weights[:, g]) returns."""
    rows = _np(rows, np.uint16).reshape(-1, N)
    B = rows.shape[0]
    weights = _np(weights, np.uint16)
    if weights.ndim == 1:
        weights = weights.reshape(-1, 1)
    if weights.ndim != 2:
        raise ValueError("combine_batch: weights must be [B][G]")
    if weights.shape[0] != B:
        raise ValueError("combine_batch: %d rows of weights for %d rows" % (weights.shape[0], B))
    G = weights.shape[1]
    out = np.empty((G, N), np.uint16)
    eng._chk(eng._lib.ntru_combine_batch(eng._h, N, mod, _ptr(rows) if B else None, _ptr(weights) if B else None, B, G, _ptr(out)))
    return out


def combine_batch_dev(eng, N, mod, d_rows, d_weights, B, G, d_out):
    """The same on DEVICE pointers, enqueued on the engine's stream without synchronising: d_rows [B][N], d_weights [B][G], d_out [G][N],
    all uint16.  Weights that are not below mod are the caller's error."""
    dp = eng._dp
    eng._chk(eng._lib.ntru_combine_batch_dev(eng._h, N, mod, dp(d_rows), dp(d_weights), int(B), int(G), dp(d_out)))
