"""Re-randomising and shuffling ciphertexts under the shared public key h (include/ntru_engine.h "re-randomising and shuffling"):
encryptBits (index.js:87-110) with an existing ciphertext row in the place of m, one mix step.  Output row i is
(Enc(0; r[i]) + e[src[i]]) mod q with the quotient of Enc(0; r[i]); VerifyEncrypt (circuits/ntru.circom:188-208) accepts
{r, m: e[src[i]], h, quotientE, remainderE}.  The order itself can be drawn on the device from a ChaCha20 key (draw_permutation, made
by argsort_keys_dev's stable sort), and mix_batch is the whole step from a key: draw r, draw the order, re-encrypt.  Functions on an
Engine: its class keeps the methods it had."""
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


# ---- the order of a mix step drawn on the device (include/ntru_engine.h "drawing the mix order") --------------------------------------
PERM_NONCE2 = 0x5045524D          # NTRU_PERM_NONCE2, "PERM"
PERM_MAX_B = 1 << 24              # NTRU_PERM_MAX_B


def _key(key):
    return _np(key, np.uint32, (8,))


def argsort_keys_dev(eng, d_keys, B, d_order):
    """d_order [B] int64 = the stable ascending argsort of the DEVICE keys d_keys [B] uint64 (not modified), enqueued on the engine's
    stream."""
    dp = eng._dp
    eng._chk(eng._lib.ntru_argsort_keys_dev(eng._h, dp(d_keys), int(B), dp(d_order)))


def draw_permutation(eng, key, perm_id, B, want_inverse=False):
    """The permutation of B items under key (8 words) and perm_id: src [B] int64, the stable argsort of the ChaCha20 sort keys; with
    want_inverse (src, dst), dst[src[j]] = j."""
    key = _key(key)
    src = np.empty(int(B), np.int64)
    dst = np.empty(int(B), np.int64) if want_inverse else None
    eng._chk(eng._lib.ntru_draw_permutation(eng._h, _ptr(key), int(perm_id), int(B), _ptr(src), _ptr(dst)))
    return (src, dst) if want_inverse else src


def draw_permutation_dev(eng, key, perm_id, B, d_src, d_dst=None):
    """The same into DEVICE arrays, enqueued on the engine's stream; key is host data, read now.  d_dst may be None; d_src may be None
    only if d_dst is not."""
    dp = eng._dp
    key = _key(key)
    eng._chk(eng._lib.ntru_draw_permutation_dev(eng._h, _ptr(key), int(perm_id), int(B), dp(d_src), dp(d_dst)))


def mix_batch(eng, N, q, p, h, key, first_item, n1, n2, perm_id, e, want_r=True, want_src=True, want_quot=True):
    """One mix step from a key: r[i] = row first_item + i of sample_ternary(N, n1, n2, p - 1, key), src = draw_permutation(key, perm_id,
    B), e_out[i] = (Enc(0; r[i]) + e[src[i]]) mod q.  e [B][N] uint16.  Returns (e_out, quotE, r, src); what was not wanted is None."""
    h = _np(h, np.uint16, (N,))
    key = _key(key)
    e = _np(e, np.uint16).reshape(-1, N)
    B = e.shape[0]
    e_out = np.empty((B, N), np.uint16)
    quot = np.empty((B, N), np.uint16) if want_quot else None
    r = np.empty((B, N), np.uint8) if want_r else None
    src = np.empty(B, np.int64) if want_src else None
    eng._chk(eng._lib.ntru_mix_batch(eng._h, N, q, p, _ptr(h), _ptr(key), int(first_item), int(n1), int(n2), int(perm_id), _ptr(e), B,
                                     _ptr(r), _ptr(src), _ptr(e_out), _ptr(quot)))
    return e_out, quot, r, src


def mix_batch_dev(eng, N, q, p, d_h, key, first_item, n1, n2, perm_id, d_e_in, B, d_r, d_src, d_e_out, d_quotE=None):
    """The same on DEVICE pointers, enqueued on the engine's stream: d_r [B][N] uint8 and d_src [B] int64 are outputs the caller
    supplies; d_e_out must not overlap d_e_in; key is host data, read now."""
    dp = eng._dp
    key = _key(key)
    eng._chk(eng._lib.ntru_mix_batch_dev(eng._h, N, q, p, dp(d_h), _ptr(key), int(first_item), int(n1), int(n2), int(perm_id), dp(d_e_in),
                                         int(B), dp(d_r), dp(d_src), dp(d_e_out), dp(d_quotE)))
