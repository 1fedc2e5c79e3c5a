// elementwise.hip -- MI355X (gfx950): the HBM-bound elementwise calls, each with its *_dev entry point:
//   stand-alone dividePolynomials(., I, mod) and addPolynomials on ciphertexts (index.js:358-401, :235-244): k_split_by_I, k_add_mod*
//   BN254 field packing (packOutput / unpackInput, index.js:572-620): k_pack, k_pack_bytes2, k_unpack, ntru_pack_params
#include "kernels_common.h"

// dividePolynomials(a, I, mod) for reduced dividends, elementwise (HBM-bound): a is [B][2N].
__global__ void k_split_by_I(int N, u32 mod, const u16 *__restrict__ a, long B, u16 *__restrict__ quot,
                             u16 *__restrict__ rem) {
  const long total = B * N;
  for (long idx = (long)blockIdx.x * blockDim.x + threadIdx.x; idx < total; idx += (long)gridDim.x * blockDim.x) {
    const long row = idx / N; const int k = (int)(idx - row * N);
    const u32 lo = a[row * 2 * N + k], hi = a[row * 2 * N + N + k];
    quot[idx] = (u16)((mod - hi % mod) % mod);
    rem[idx] = (u16)((lo + hi) % mod);
  }
}

// addPolynomials(a, b, mod) on [B][N] rows, elementwise (HBM-bound).  The rows are contiguous, so the batch is one flat
// array: 16 bytes (8 coefficients) per lane per access when the three base pointers are 16-byte aligned.
template <bool POW2>
__global__ void k_add_mod_vec(u32 mod, const u16x8 *__restrict__ a, const u16x8 *__restrict__ b, long nvec,
                              u16x8 *__restrict__ out) {
  for (long idx = (long)blockIdx.x * blockDim.x + threadIdx.x; idx < nvec; idx += (long)gridDim.x * blockDim.x) {
    const u16x8 x = a[idx], y = b[idx];
    u16x8 r;
    if (POW2) {
      r = (x + y) & (u16)(mod - 1);                     // q | 2^16: wrapped 16-bit sums are exact mod q
    } else {
#pragma unroll
      for (int k = 0; k < 8; k++) r[k] = (u16)(((u32)x[k] + (u32)y[k]) % mod);
    }
    out[idx] = r;
  }
}
__global__ void k_add_mod(u32 mod, const u16 *__restrict__ a, const u16 *__restrict__ b, long first, long total,
                          u16 *__restrict__ out) {
  for (long idx = first + (long)blockIdx.x * blockDim.x + threadIdx.x; idx < total; idx += (long)gridDim.x * blockDim.x)
    out[idx] = (u16)(((u32)a[idx] + (u32)b[idx]) % mod);
}

// ---- BN254 field-element packing (index.js:572-620): elementwise, HBM-bound ---------------------------------------
// One thread per 64-bit limb of the output: out[b][o] = sum_j data[b][o*per + j] << (j*bits), four LE limbs per element.
// T: u16 values (ciphertexts, witness arrays) or bytes (decrypted values, ternary arrays).
template <class T>
__global__ void k_pack(int bits, int per, int data_len, int out_size, const T *__restrict__ data, long B,
                       unsigned long long *__restrict__ out) {
  const long total = B * out_size * 4;
  for (long idx = (long)blockIdx.x * blockDim.x + threadIdx.x; idx < total; idx += (long)gridDim.x * blockDim.x) {
    const int l = (int)(idx & 3);
    const long eo = idx >> 2;
    const long b = eo / out_size;
    const int o = (int)(eo - b * out_size);
    const int lo_bit = 64 * l;
    int j0 = lo_bit / bits, j1 = (lo_bit + 63) / bits;
    if (j1 >= per) j1 = per - 1;
    unsigned long long limb = 0;
    for (int j = j0; j <= j1; j++) {
      const int i = o * per + j;
      const unsigned long long v = i < data_len ? data[b * data_len + i] : 0ull;
      const int sh = j * bits - lo_bit;
      limb |= sh >= 0 ? v << sh : v >> (-sh);
    }
    out[idx] = limb;
  }
}

// packOutput of BYTES with 2-bit fields (values of decryptBits, ternary rows: max_val 2 or 3; 126 values per element): one thread per
// output DWORD = 16 consecutive values = 16 consecutive bytes of the row (the eighth dword of an element holds 14), read as four
// dwords at whatever alignment they have.  (The generic kernel above reads 32 single bytes per 64-bit limb: 1.2 ms per 2^20 rows of
// N = 821 against 0.3 ms.)
__global__ void k_pack_bytes2(int data_len, int out_size, const uint8_t *__restrict__ data, long B, u32 *__restrict__ out) {
  const long total = B * out_size * 8;
  for (long idx = (long)blockIdx.x * blockDim.x + threadIdx.x; idx < total; idx += (long)gridDim.x * blockDim.x) {
    const long b = idx / (out_size * 8);
    const int dw = (int)(idx - b * out_size * 8), o = dw >> 3, k = dw & 7, i0 = 126 * o + 16 * k;
    const uint8_t *src = data + b * data_len + i0;
    u32 res = 0;
    if (i0 + 16 <= data_len) {
      u32 d[4];
#pragma unroll
      for (int c = 0; c < 4; c++) __builtin_memcpy(&d[c], src + 4 * c, 4);
      res = pack2x16(d, 0);
    } else {
      for (int j = 0; j < 16; j++) if (i0 + j < data_len) res |= ((u32)src[j] & 3u) << (2 * j);
    }
    out[idx] = k == 7 ? res & 0x0FFFFFFFu : res;
  }
}

// unpackInput before trimming: out[b][i*per + j] = (in[b][i] >> (j*bits)) & mask.
__global__ void k_unpack(int bits, int per, int packed_size, const unsigned long long *__restrict__ in, long B,
                         u16 *__restrict__ out) {
  const long total = B * packed_size * per;
  for (long idx = (long)blockIdx.x * blockDim.x + threadIdx.x; idx < total; idx += (long)gridDim.x * blockDim.x) {
    const long e = idx / per;
    const int j = (int)(idx - e * per);
    const unsigned long long *l = in + e * 4;
    const int pos = j * bits, w = pos >> 6, sft = pos & 63;
    unsigned long long v = l[w] >> sft;
    if (sft + bits > 64 && w + 1 < 4) v |= l[w + 1] << (64 - sft);
    out[idx] = (u16)(v & ((1u << bits) - 1u));
  }
}

// ---- host side: *_dev entry points ------------------------------------------------------------------------------------------

static int check_elementwise(const ntru_engine *eng, int N, int mod, long B) {
  if (!eng) return fail(NTRU_ERR_ARG, "engine is NULL");
  if (B < 0) return fail(NTRU_ERR_ARG, "negative batch size");
  if (N < 1 || mod < 2 || mod > 65536) return fail(NTRU_ERR_UNSUPPORTED, "need N >= 1 and 2 <= mod <= 65536");
  return NTRU_OK;
}

extern "C" int ntru_split_by_I_dev(ntru_engine_t *eng, int N, int mod, const uint16_t *d_a, int64_t B,
                                   uint16_t *d_quot, uint16_t *d_rem) {
  if (int rc = check_elementwise(eng, N, mod, B)) return rc;
  if (B == 0) return NTRU_OK;
  if (!d_a || !d_quot || !d_rem) return fail(NTRU_ERR_ARG, "ntru_split_by_I: NULL buffer");
  HIP_TRY(hipSetDevice(eng->device));
  hipLaunchKernelGGL(k_split_by_I, elementwise_grid(eng, B * N), dim3(256), 0, eng->stream, N, (u32)mod, d_a, (long)B,
                     d_quot, d_rem);
  HIP_TRY(hipGetLastError());
  return NTRU_OK;
}

extern "C" int ntru_add_batch_dev(ntru_engine_t *eng, int N, int mod, const uint16_t *d_a, const uint16_t *d_b,
                                  int64_t B, uint16_t *d_out) {
  if (int rc = check_elementwise(eng, N, mod, B)) return rc;
  if (B == 0) return NTRU_OK;
  if (!d_a || !d_b || !d_out) return fail(NTRU_ERR_ARG, "ntru_add_batch: NULL buffer");
  HIP_TRY(hipSetDevice(eng->device));
  const long total = (long)B * N;
  const bool aligned = (((uintptr_t)d_a | (uintptr_t)d_b | (uintptr_t)d_out) & 15) == 0;
  const long nvec = aligned ? total / 8 : 0;
  if (nvec) {
    if (is_pow2(mod))
      hipLaunchKernelGGL(k_add_mod_vec<true>, elementwise_grid(eng, nvec, true), dim3(256), 0, eng->stream, (u32)mod,
                         (const u16x8 *)d_a, (const u16x8 *)d_b, nvec, (u16x8 *)d_out);
    else
      hipLaunchKernelGGL(k_add_mod_vec<false>, elementwise_grid(eng, nvec, true), dim3(256), 0, eng->stream, (u32)mod,
                         (const u16x8 *)d_a, (const u16x8 *)d_b, nvec, (u16x8 *)d_out);
  }
  if (nvec * 8 < total)
    hipLaunchKernelGGL(k_add_mod, elementwise_grid(eng, total - nvec * 8), dim3(256), 0, eng->stream, (u32)mod, d_a, d_b,
                       nvec * 8, total, d_out);
  HIP_TRY(hipGetLastError());
  return NTRU_OK;
}

extern "C" int ntru_pack_params(int max_val, int data_len, int *bits, int *per_output, int *arr_len, int *output_size) {
  if (max_val < 1 || max_val > 65535 || data_len < 0 || !bits || !per_output || !arr_len || !output_size)
    return fail(NTRU_ERR_ARG, "ntru_pack_params: need 1 <= max_val <= 65535, data_len >= 0 and non-NULL outputs");
  int b = 0;
  while ((max_val >> b) != 0) b++;                    // floor(log2(maxVal) + 1), index.js:573
  const int n = 252 / b;                              // index.js:574
  int al = ((data_len + n - 1) / n) * n;              // index.js:575-578
  if (al < 3 * n) al = 3 * n;
  int os = (al + n - 1) / n;                          // index.js:580
  if (os < 3) os = 3;
  *bits = b; *per_output = n; *arr_len = al; *output_size = os;
  return NTRU_OK;
}

extern "C" int ntru_pack_batch_dev(ntru_engine_t *eng, int max_val, int data_len, const uint16_t *d_data, int64_t B,
                                   uint64_t *d_out) {
  if (!eng) return fail(NTRU_ERR_ARG, "engine is NULL");
  if (B < 0) return fail(NTRU_ERR_ARG, "negative batch size");
  int bits, per, al, os;
  if (int rc = ntru_pack_params(max_val, data_len, &bits, &per, &al, &os)) return rc;
  if (B == 0) return NTRU_OK;
  if ((!d_data && data_len) || !d_out) return fail(NTRU_ERR_ARG, "ntru_pack_batch: NULL buffer");
  HIP_TRY(hipSetDevice(eng->device));
  hipLaunchKernelGGL(k_pack<u16>, elementwise_grid(eng, B * os * 4), dim3(256), 0, eng->stream, bits, per, data_len, os, d_data,
                     (long)B, (unsigned long long *)d_out);
  HIP_TRY(hipGetLastError());
  return NTRU_OK;
}

// The same for an array of BYTES (decryptBits' value, quotient2, r, m: values <= 255): packOutput without widening it first.
extern "C" int ntru_pack_bytes_batch_dev(ntru_engine_t *eng, int max_val, int data_len, const uint8_t *d_data, int64_t B,
                                         uint64_t *d_out) {
  if (!eng) return fail(NTRU_ERR_ARG, "engine is NULL");
  if (B < 0) return fail(NTRU_ERR_ARG, "negative batch size");
  if (max_val > 255) return fail(NTRU_ERR_ARG, "ntru_pack_bytes_batch: max_val must fit a byte");
  int bits, per, al, os;
  if (int rc = ntru_pack_params(max_val, data_len, &bits, &per, &al, &os)) return rc;
  if (B == 0) return NTRU_OK;
  if ((!d_data && data_len) || !d_out) return fail(NTRU_ERR_ARG, "ntru_pack_bytes_batch: NULL buffer");
  HIP_TRY(hipSetDevice(eng->device));
  if (bits == 2) {                                         // ternary rows / decrypted values: 16 values per output dword
    hipLaunchKernelGGL(k_pack_bytes2, elementwise_grid(eng, B * os * 8), dim3(256), 0, eng->stream, data_len, os, d_data, (long)B, (u32 *)d_out);
    HIP_TRY(hipGetLastError());
    return NTRU_OK;
  }
  hipLaunchKernelGGL(k_pack<uint8_t>, elementwise_grid(eng, B * os * 4), dim3(256), 0, eng->stream, bits, per, data_len, os, d_data,
                     (long)B, (unsigned long long *)d_out);
  HIP_TRY(hipGetLastError());
  return NTRU_OK;
}

extern "C" int ntru_unpack_batch_dev(ntru_engine_t *eng, int max_val, int packed_bits, const uint64_t *d_in,
                                     int packed_size, int64_t B, uint16_t *d_out) {
  if (!eng) return fail(NTRU_ERR_ARG, "engine is NULL");
  if (B < 0 || packed_size < 0) return fail(NTRU_ERR_ARG, "negative size");
  if (max_val < 1 || max_val > 65535) return fail(NTRU_ERR_ARG, "need 1 <= max_val <= 65535");
  int bits = 0;
  while ((max_val >> bits) != 0) bits++;
  const int per = packed_bits / bits;
  if (per < 1 || per * bits > 256) return fail(NTRU_ERR_ARG, "packed_bits does not hold a whole number of values within 256 bits");
  if (B == 0 || packed_size == 0) return NTRU_OK;
  if (!d_in || !d_out) return fail(NTRU_ERR_ARG, "ntru_unpack_batch: NULL buffer");
  HIP_TRY(hipSetDevice(eng->device));
  hipLaunchKernelGGL(k_unpack, elementwise_grid(eng, B * packed_size * per), dim3(256), 0, eng->stream, bits, per,
                     packed_size, (const unsigned long long *)d_in, (long)B, d_out);
  HIP_TRY(hipGetLastError());
  return NTRU_OK;
}
