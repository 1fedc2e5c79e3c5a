"""Measuring the decryption noise of ciphertext rows under a private key (include/ntru_engine.h "measuring noise"): a = f * e mod
(x^N - 1, q) -- the rem1 of decrypt_batch -- centred at q/2 and reduced to peak = max |c_k| and energy = sum c_k^2 per row, on the
shared-key matrix kernels where they apply.  Functions on an Engine: its class keeps the methods it had."""
import numpy as np

from .engine import _np, _ptr
from .packed import _packed


def _outputs(B, want_peak, want_energy):
    return (np.empty(B, np.uint16) if want_peak else None), (np.empty(B, np.uint64) if want_energy else None)


def noise_batch(eng, N, q, f, e, want_peak=True, want_energy=True):
    """f [N] int8 in {-1, 0, 1}, e [B][N] uint16.  Returns (peak [B] uint16, energy [B] uint64); one of them may be switched off
    (it comes back as None), not both."""
    f = _np(f, np.int8, (N,))
    e = _np(e, np.uint16).reshape(-1, N)
    B = e.shape[0]
    peak, energy = _outputs(B, want_peak, want_energy)
    eng._chk(eng._lib.ntru_noise_batch(eng._h, N, q, _ptr(f), _ptr(e), B, _ptr(peak), _ptr(energy)))
    return peak, energy


def noise_batch_dev(eng, N, q, d_f, d_e, B, d_peak, d_energy):
    """The same on DEVICE pointers, enqueued on the engine's stream without synchronising: d_f [N] int8, d_e [B][N] uint16, d_peak [B]
    uint16, d_energy [B] uint64 (8-byte aligned); d_peak or d_energy may be None."""
    dp = eng._dp
    eng._chk(eng._lib.ntru_noise_batch_dev(eng._h, N, q, dp(d_f), dp(d_e), int(B), dp(d_peak), dp(d_energy)))
    eng._note(N, B, 2 * N + (2 if d_peak else 0) + (8 if d_energy else 0))        # the row in; 2 + 8 bytes out


def noise_packed_batch(eng, N, q, f, packed, want_peak=True, want_energy=True):
    """noise_batch on rows in the wire format: packed uint64 [B][outputSize][4], packOutput(q - 1, N, e) of every row."""
    f = _np(f, np.int8, (N,))
    packed = _packed(eng, N, q, packed)
    B = packed.shape[0]
    peak, energy = _outputs(B, want_peak, want_energy)
    eng._chk(eng._lib.ntru_noise_packed_batch(eng._h, N, q, _ptr(f), _ptr(packed), B, _ptr(peak), _ptr(energy)))
    return peak, energy


def noise_packed_batch_dev(eng, N, q, d_f, d_packed, B, d_peak, d_energy):
    """noise_batch_dev with d_packed, DEVICE uint64 [B][outputSize][4], in place of d_e."""
    dp = eng._dp
    eng._chk(eng._lib.ntru_noise_packed_batch_dev(eng._h, N, q, dp(d_f), dp(d_packed), int(B), dp(d_peak), dp(d_energy)))
