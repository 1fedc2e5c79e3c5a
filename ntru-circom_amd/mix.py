"""Re-randomising and shuffling ciphertexts under the shared public key h (include/ntru_engine.h "re-randomising and shuffling"):
encryptBits (index.js:87-110) with an existing ciphertext row in the place of m, one mix step.  Output row i is
(Enc(0; r[i]) + e[src[i]]) mod q with the quotient of Enc(0; r[i]); VerifyEncrypt (circuits/ntru.circom:188-208) accepts
{r, m: e[src[i]], h, quotientE, remainderE}.  Functions on an Engine: its class keeps the methods it had."""
import numpy as np

from .engine import _np, _ptr


def reencrypt_batch(eng, N, q, h, r, e, src=None, want_quot=True):
    """h (N,) uint16, r [B][N] in {0, 1, p - 1}, e [B_in][N] uint16 (any value, reduced mod q), src [B] row indices into e (None:
    row i, needs B <= B_in; repeats allowed; an index outside [0, B_in) is an EngineError).  Returns (e_out, quotE), [B][N] uint16;
    quotE is None without want_quot."""
    h = _np(h, np.uint16, (N,))
    r = _np(r, np.uint8).reshape(-1, N)
    e = _np(e, np.uint16).reshape(-1, N)
    B, B_in = r.shape[0], e.shape[0]
    if src is not None:
        src = _np(src, np.int64).reshape(-1)
        if src.shape[0] != B:
            raise ValueError("reencrypt_batch: r has %d rows, src %d entries" % (B, src.shape[0]))
    e_out = np.empty((B, N), np.uint16)
    quot = np.empty((B, N), np.uint16) if want_quot else None
    eng._chk(eng._lib.ntru_reencrypt_batch(eng._h, N, q, _ptr(h), _ptr(r), _ptr(e), B_in, _ptr(src), B, _ptr(e_out), _ptr(quot)))
    return e_out, quot


def reencrypt_batch_dev(eng, N, q, d_h, d_r, d_e_in, B_in, d_e_out, B, d_src=None, d_quotE=None):
    """The same on DEVICE pointers, enqueued on the engine's stream; d_src: int64 [B] in device memory.  d_e_out may be d_e_in when
    d_src is None.  A d_src entry outside [0, B_in) reads nothing: that row becomes Enc(0; r[i])."""
    dp = eng._dp
    eng._chk(eng._lib.ntru_reencrypt_batch_dev(eng._h, N, q, dp(d_h), dp(d_r), dp(d_e_in), int(B_in), dp(d_src), int(B), dp(d_e_out),
                                               dp(d_quotE)))
