"""Removing duplicates: which ciphertext rows of a batch repeat an earlier row, of the batch or of a prior set (include/ntru_engine.h
"removing duplicates").  Two rows are equal when every coefficient agrees modulo `mod`; packed rows compare by their N fields.  The
S prior rows take the indices 0 .. S - 1, the B new rows S .. S + B - 1; first[b] is the smallest index of a row equal to new row b,
unique lists the new rows that are their own first occurrence.  Functions on an Engine: its class keeps the methods it had."""
import ctypes as C

import numpy as np

from .engine import _np, _ptr
from .packed import _packed

DEDUP_MAX_ROWS = 1 << 24          # NTRU_DEDUP_MAX_ROWS


def dedup_workspace_bytes(eng, N, total_rows):
    """Bytes of the caller-owned device workspace of the _dev forms for S + B = total_rows rows."""
    n = C.c_size_t()
    eng._chk(eng._lib.ntru_dedup_workspace_bytes(int(N), int(total_rows), C.byref(n)))
    return n.value


def _host(eng, call, N, mod, prior, rows, salt, fingerprint_bits, want_first, want_unique):
    B, S = rows.shape[0], 0 if prior is None else prior.shape[0]
    first = np.empty(B, np.int64) if want_first else None
    unique = np.empty(B, np.int64) if want_unique else None
    count = np.zeros(1, np.int64)
    eng._chk(call(eng._h, N, mod, _ptr(prior) if S else None, S, _ptr(rows), B, int(salt), int(fingerprint_bits), _ptr(first), _ptr(unique),
                  _ptr(count)))
    return first, (unique[:int(count[0])] if want_unique else None)


def dedup_rows(eng, N, mod, rows, prior=None, salt=0, fingerprint_bits=64, want_first=True, want_unique=True):
    """rows [B][N] uint16, prior [S][N] uint16 or None.  Returns (first [B] int64, unique [count] int64); what was not wanted is
    None."""
    rows = _np(rows, np.uint16).reshape(-1, N)
    prior = None if prior is None else _np(prior, np.uint16).reshape(-1, N)
    return _host(eng, eng._lib.ntru_dedup_rows, N, mod, prior, rows, salt, fingerprint_bits, want_first, want_unique)


def dedup_packed(eng, N, mod, packed, prior=None, salt=0, fingerprint_bits=64, want_first=True, want_unique=True):
    """dedup_rows on rows in the wire format: packed (and prior) uint64 [.][outputSize][4], packOutput(mod - 1, N, e) of every row."""
    packed = _packed(eng, N, mod, packed)
    prior = None if prior is None else _packed(eng, N, mod, prior)
    return _host(eng, eng._lib.ntru_dedup_packed, N, mod, prior, packed, salt, fingerprint_bits, want_first, want_unique)


def _dev(eng, call, row_bytes, N, mod, d_prior, S, d_rows, B, salt, fingerprint_bits, d_work, d_first, d_unique, d_count):
    dp = eng._dp
    eng._chk(call(eng._h, N, mod, dp(d_prior), int(S), dp(d_rows), int(B), int(salt), int(fingerprint_bits), dp(d_work), dp(d_first),
                  dp(d_unique), dp(d_count)))
    if B > 0:
        eng._note(N, int(S) + int(B), row_bytes)


def dedup_rows_dev(eng, N, mod, d_prior, S, d_rows, B, salt, fingerprint_bits, d_work, d_first, d_unique, d_count):
    """The same on DEVICE pointers, enqueued on the engine's stream without synchronising: d_prior [S][N] and d_rows [B][N] uint16,
    d_work dedup_workspace_bytes(N, S + B) bytes, d_first [B], d_unique [B] and d_count [1] int64; d_prior (S == 0), d_first and
    d_unique may be None."""
    _dev(eng, eng._lib.ntru_dedup_rows_dev, 2 * N, N, mod, d_prior, S, d_rows, B, salt, fingerprint_bits, d_work, d_first, d_unique, d_count)


def dedup_packed_dev(eng, N, mod, d_prior, S, d_packed, B, salt, fingerprint_bits, d_work, d_first, d_unique, d_count):
    """dedup_rows_dev with DEVICE uint64 [.][outputSize][4] rows in place of d_prior and d_rows."""
    row_bytes = 32 * eng.pack_params(mod - 1, N)["outputSize"] if 2 <= mod <= 65536 and N >= 0 else 0
    _dev(eng, eng._lib.ntru_dedup_packed_dev, row_bytes, N, mod, d_prior, S, d_packed, B, salt, fingerprint_bits, d_work, d_first, d_unique,
         d_count)
