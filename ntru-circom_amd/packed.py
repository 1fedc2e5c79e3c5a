"""Ciphertexts in the circuits' wire format -- rows of packOutput(q - 1, N, e) field elements, uint64 [B][outputSize][4] -- summed,
tallied and decrypted without unpacking them first (include/ntru_engine.h "packed ciphertexts").  Functions on an Engine: its class
keeps the methods it had.  pack_rows / unpack_rows are the engine's own pack_batch / unpack_batch shaped for whole batches of rows."""
import numpy as np

from .engine import _np, _ptr


def _shape(eng, N, mod):
    pr = eng.pack_params(mod - 1, N)
    return pr["maxInputBits"], pr["numInputsPerOutput"], pr["outputSize"]


def _packed(eng, N, mod, packed):
    """packed as contiguous uint64 [B][outputSize][4]."""
    os_ = _shape(eng, N, mod)[2]
    return _np(packed, np.uint64).reshape(-1, os_, 4)


def pack_rows(eng, N, mod, rows):
    """[B][N] coefficients -> [B][outputSize][4] uint64 limbs: packOutput(mod - 1, N, row) of every row (index.js:572-596)."""
    return eng.pack_batch(mod - 1, N, _np(rows, np.uint16).reshape(-1, N))


def unpack_rows(eng, N, mod, packed):
    """[B][outputSize][4] limbs -> [B][N] uint16: unpackInput (index.js:598-620) of every row, the pad dropped."""
    bits, per, _ = _shape(eng, N, mod)
    packed = _packed(eng, N, mod, packed)
    return np.ascontiguousarray(eng.unpack_batch(mod - 1, per * bits, packed)[:, :N])


def sum_groups_packed(eng, N, mod, packed, offsets=None, K=None, weights=None):
    """Engine.sum_groups on the rows that `packed` holds: [G][N] uint16."""
    packed = _packed(eng, N, mod, packed)
    offsets, K, G, weights = eng._groups(packed, offsets, K, weights)
    out = np.empty((G, N), np.uint16)
    eng._chk(eng._lib.ntru_sum_groups_packed(eng._h, N, mod, _ptr(packed), _ptr(weights), _ptr(offsets), K, G, _ptr(out)))
    return out


def sum_groups_packed_dev(eng, N, mod, d_packed, d_out, G, d_offsets=None, K=None, d_weights=None):
    """Engine.sum_groups_dev with d_packed, DEVICE uint64 [B][outputSize][4], in place of d_rows; d_out is dense [G][N]."""
    dp = eng._dp
    eng._chk(eng._lib.ntru_sum_groups_packed_dev(eng._h, N, mod, dp(d_packed), dp(d_weights), dp(d_offsets), int(K or 0), int(G),
                                                 dp(d_out)))


def tally_decrypt_packed_batch(eng, N, q, p, f, fp, packed, offsets=None, K=None, weights=None, want_witness=True):
    """Engine.tally_decrypt_batch on packed rows.  Returns (sum, value, quot1, rem1, quot2), dense [G][N]."""
    f, fp = _np(f, np.int8, (N,)), _np(fp, np.uint8, (N,))
    packed = _packed(eng, N, q, packed)
    offsets, K, G, weights = eng._groups(packed, offsets, K, weights)
    total, value = np.empty((G, N), np.uint16), np.empty((G, N), np.uint8)
    q1 = np.empty((G, N), np.uint16) if want_witness else None
    r1 = np.empty((G, N), np.uint16) if want_witness else None
    q2 = np.empty((G, N), np.uint8) if want_witness else None
    eng._chk(eng._lib.ntru_tally_decrypt_packed_batch(eng._h, N, q, p, _ptr(f), _ptr(fp), _ptr(packed), _ptr(weights), _ptr(offsets), K, G,
                                                      _ptr(total), _ptr(value), _ptr(q1), _ptr(r1), _ptr(q2)))
    return total, value, q1, r1, q2


def tally_decrypt_packed_batch_dev(eng, N, q, p, d_f, d_fp, d_packed, d_sum, d_value, G, d_offsets=None, K=None, d_weights=None,
                                   d_quot1=None, d_rem1=None, d_quot2=None):
    dp = eng._dp
    eng._chk(eng._lib.ntru_tally_decrypt_packed_batch_dev(eng._h, N, q, p, dp(d_f), dp(d_fp), dp(d_packed), dp(d_weights), dp(d_offsets),
                                                          int(K or 0), int(G), dp(d_sum), dp(d_value), dp(d_quot1), dp(d_rem1),
                                                          dp(d_quot2)))


def decrypt_packed_batch(eng, N, q, p, f, fp, packed, want_witness=True):
    """Engine.decrypt_batch on packed rows.  Returns (value, quot1, rem1, quot2), [B][N]."""
    f, fp = _np(f, np.int8, (N,)), _np(fp, np.uint8, (N,))
    packed = _packed(eng, N, q, packed)
    B = packed.shape[0]
    value = np.empty((B, N), np.uint8)
    q1 = np.empty((B, N), np.uint16) if want_witness else None
    r1 = np.empty((B, N), np.uint16) if want_witness else None
    q2 = np.empty((B, N), np.uint8) if want_witness else None
    eng._chk(eng._lib.ntru_decrypt_packed_batch(eng._h, N, q, p, _ptr(f), _ptr(fp), _ptr(packed), B, _ptr(value), _ptr(q1), _ptr(r1),
                                                _ptr(q2)))
    return value, q1, r1, q2


def decrypt_packed_batch_dev(eng, N, q, p, d_f, d_fp, d_packed, B, d_value, d_quot1=None, d_rem1=None, d_quot2=None):
    dp = eng._dp
    eng._chk(eng._lib.ntru_decrypt_packed_batch_dev(eng._h, N, q, p, dp(d_f), dp(d_fp), dp(d_packed), int(B), dp(d_value), dp(d_quot1),
                                                    dp(d_rem1), dp(d_quot2)))
