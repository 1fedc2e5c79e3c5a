"""Multiplying a batch by one shared polynomial (include/ntru_engine.h "product of a batch with ONE shared polynomial"): rows [B][N]
times s [N] modulo mod, split by 1 - x^N -- polymul_split with its second operand fixed over the batch, on the shared-key matrix kernels
where they apply.  Functions on an Engine: its class keeps the methods it had."""
import numpy as np

from .engine import _np, _ptr


def mul_shared_batch(eng, N, mod, s, rows, want_quot=True):
    """s [N] uint16, rows [B][N] uint16 (any uint16 when mod is a power of two, below mod otherwise).  Returns (quot, rem), both
    [B][N] uint16 (quot is None without want_quot): row b is what Engine.polymul_split(N, mod, rows[b], s) returns."""
    s = _np(s, np.uint16, (N,))
    rows = _np(rows, np.uint16).reshape(-1, N)
    B = rows.shape[0]
    quot = np.empty((B, N), np.uint16) if want_quot else None
    rem = np.empty((B, N), np.uint16)
    eng._chk(eng._lib.ntru_mul_shared_batch(eng._h, N, mod, _ptr(s), _ptr(rows), B, _ptr(quot), _ptr(rem)))
    return quot, rem


def mul_shared_batch_dev(eng, N, mod, d_s, d_rows, B, d_quot, d_rem):
    """The same on DEVICE pointers, enqueued on the engine's stream without synchronising: d_s [N], d_rows, d_quot, d_rem [B][N], all
    uint16; d_quot may be None."""
    dp = eng._dp
    eng._chk(eng._lib.ntru_mul_shared_batch_dev(eng._h, N, mod, dp(d_s), dp(d_rows), int(B), dp(d_quot), dp(d_rem)))
    eng._note(N, B, (6 if d_quot else 4) * N)        # rows in; rem (+ quot) out
