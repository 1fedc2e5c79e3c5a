"""Restatement of the packed-ciphertext format and of the sums over it, without the engine: packOutput / unpackInput (index.js:572-620)
on Python ints, the same on whole batches of uint64 limbs in numpy, the rules for what a reader ignores, and np_sum of
tests/ciphertext_sum_ref.py on the unpacked rows.  tests/test_packed_ciphertexts_cpu.py ties it to the captured packOutput vectors."""
import numpy as np

import ciphertext_sum_ref as sum_ref

# N, mod, bits, per, output_size: one shape for every way the sum kernel lays a row out -- several rows side by side in a wave
# (os <= 32), one row per step (32 < os <= 64), tiles of 64 elements (os > 64), a modulus that is no power of two, and the two
# smallest, whose elements hold more than 36 fields (per > 36)
SHAPES = [(64, 128, 7, 36, 3), (167, 2048, 11, 22, 8), (821, 4096, 12, 21, 40), (701, 8192, 13, 19, 37), (509, 65536, 16, 15, 34),
          (1920, 4096, 12, 21, 92), (167, 12289, 14, 18, 10), (17, 32, 5, 50, 3), (167, 3, 2, 126, 3)]


def params(max_val, data_len):
    """(bits, per, arr_len, output_size) as packOutput computes them (index.js:573-580)."""
    bits = int(max_val).bit_length()
    per = 252 // bits
    arr_len = max(-(-data_len // per) * per, 3 * per)
    return bits, per, arr_len, max(-(-arr_len // per), 3)


def pack_ints(max_val, data_len, data):
    """packOutput(max_val, data_len, data).expected as Python ints: field j of element i is data[i * per + j], zero behind the data."""
    bits, per, arr_len, os_ = params(max_val, data_len)
    padded = [int(x) for x in data] + [0] * (arr_len - len(data))
    return [sum(padded[i * per + j] << (j * bits) for j in range(per)) for i in range(os_)]


def unpack_ints(max_val, N, elements):
    """The N coefficients a reader takes from the elements (Python ints below 2^256): field j of element i, masked to `bits`; whatever
    lies above per * bits in an element, and every field with index >= N, is ignored."""
    bits, per, _, _ = params(max_val, N)
    mask = (1 << bits) - 1
    return [(int(elements[i // per]) >> ((i % per) * bits)) & mask for i in range(N)]


def limbs_of(elements):
    """Python ints below 2^256 -> uint64 [n][4], little-endian limbs."""
    return np.array([[(int(v) >> (64 * k)) & 0xFFFFFFFFFFFFFFFF for k in range(4)] for v in elements], dtype=np.uint64).reshape(-1, 4)


def ints_of(limbs):
    return [sum(int(w) << (64 * k) for k, w in enumerate(row)) for row in np.asarray(limbs).reshape(-1, 4)]


def pack_rows(mod, rows):
    """[B][N] values below 2^bits -> uint64 [B][os][4]: packOutput(mod - 1, N, row) of every row (field by field on the limbs)."""
    rows = np.asarray(rows)
    B, N = rows.shape
    bits, per, arr_len, os_ = params(mod - 1, N)
    padded = np.zeros((B, os_ * per), np.uint64)
    padded[:, :N] = rows
    padded = padded.reshape(B, os_, per)
    out = np.zeros((B, os_, 4), np.uint64)
    for j in range(per):
        k, sh = divmod(j * bits, 64)
        out[:, :, k] |= padded[:, :, j] << np.uint64(sh)
        if sh + bits > 64:
            out[:, :, k + 1] |= padded[:, :, j] >> np.uint64(64 - sh)
    return out


def unpack_rows(mod, N, packed):
    """uint64 [B][os][4] -> uint16 [B][N] under the ignore rules of unpack_ints."""
    bits, per, _, os_ = params(mod - 1, N)
    packed = np.asarray(packed, dtype=np.uint64).reshape(-1, os_, 4)
    out = np.zeros((packed.shape[0], os_, per), np.uint64)
    for j in range(per):
        k, sh = divmod(j * bits, 64)
        v = packed[:, :, k] >> np.uint64(sh)
        if sh + bits > 64:
            v = v | (packed[:, :, k + 1] << np.uint64(64 - sh))
        out[:, :, j] = v & np.uint64((1 << bits) - 1)
    return np.ascontiguousarray(out.reshape(-1, os_ * per)[:, :N]).astype(np.uint16)


def ignored_mask(mod, N):
    """uint64 [os][4]: every bit of a packed row that a reader must ignore -- the fields with index >= N and the bits of every
    element above per * bits."""
    bits, per, _, os_ = params(mod - 1, N)
    top = ((1 << 256) - 1) ^ ((1 << (per * bits)) - 1)
    return limbs_of([top | sum(((1 << bits) - 1) << (j * bits) for j in range(per) if i * per + j >= N) for i in range(os_)])


def set_ignored_bits(mod, N, packed):
    """A copy of the packed rows with EVERY ignored bit set."""
    mask = ignored_mask(mod, N)
    return np.asarray(packed, dtype=np.uint64).reshape(-1, mask.shape[0], 4) | mask


def np_sum_packed(mod, N, packed, offsets=None, K=None, weights=None):
    """out[g] = (sum of weights[r] * unpacked row r over group g) % mod: ciphertext_sum_ref.np_sum on the unpacked rows."""
    return sum_ref.np_sum(unpack_rows(mod, N, packed), mod, offsets=offsets, K=K, weights=weights)
