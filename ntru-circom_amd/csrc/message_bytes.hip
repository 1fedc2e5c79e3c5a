// message_bytes.hip -- byte messages as packed bits: the device side of the reference's stringToBits / bitsToString (index.js:538-556)
// and of encryptStr / decryptStr (index.js:80-86) built on them: kernels, *_dev entry points and
// ntru_pipeline_bytes_batch (the regular host-pointer forms: ntru_host.hip).
//
//   row b, coefficient 8 i + j  =  (bytes[b][i] >> (7 - j)) & 1        i < nbytes, most significant bit first (index.js:542)
//   row b, coefficient k        =  0                                   8 nbytes <= k < N: the pad
//
// A message block crosses the bus as nbytes bytes instead of N; the [B][N] coefficient rows the scheme kernels read and write exist on
// the device only.  Both kernels are bound by the N bytes per row of the coefficient array:
//   * k_bytes_to_rows treats the [B][N] output as ONE flat byte array (rows of N bytes start at any offset: N = 821 is odd).  A lane
//     owns 16 bytes at a 16-byte aligned address and stores them at once; they may belong to two rows (three for N < 16).  For each
//     row segment the lane reads the at most three message bytes that hold its coefficients.  The bytes before the first and behind
//     the last aligned address (< 16 each) are written by one lane each.
//   * k_rows_to_bytes gives a workgroup a TILE of whole rows (about 16 KB).  Its lanes load the tile as aligned 16-byte pieces, squeeze
//     each piece to 16 bits and OR the part that belongs to a row into the tile's bit image in the LDS; the row's flag bits go into
//     an LDS byte the same way (LDS atomics, none on global memory).  The image is the tile's stretch of the [B][nbytes] output: it
//     leaves as aligned 16-byte stores, with the < 16 bytes at either end, which share their 16 bytes with the neighbouring tiles,
//     stored one by one.  The flags [rows] leave the same way.  Loads that would leave the array (first and last piece) go byte by byte.
// The scheme calls run in passes of at most 65536 rows: the coefficient rows of a pass live in the engine-owned scratch buffer and
// are still on chip when the scheme kernel (called as it is) reads them.
#include <hip/hip_runtime.h>

#include <cstdint>
#include <cstdio>
#include <cstring>
#include <string>

#include "kernels_common.h"

namespace {

constexpr int MB_THREADS = 256;
constexpr int MB_TILE_BYTES = 16384;           // coefficient bytes per tile of k_rows_to_bytes (whole rows; N <= NTRU_MAX_N fits 8 times)
constexpr int MB_LDS_WORDS = MB_TILE_BYTES / 32 + 8;   // one bit per coefficient (or one flag byte per row, N >= 8) + slack for the 20-byte reads
constexpr int MB_BLOCKS_PER_CU = 8;
constexpr int64_t MB_PASS = 1 << 16;           // rows per pass of the scheme calls, as the key inversion's Newton temporaries

typedef u32 u32x4 __attribute__((ext_vector_type(4)));

// ---- bytes -> rows ------------------------------------------------------------------------------------------------------------------

// Coefficients col .. col + 15 of the row whose message bytes are at `row`, as bits 0 .. 15 (the pad reads as 0).
__device__ __forceinline__ u32 row_bits16(const uint8_t *row, int nbytes, int col) {
  const int i = col >> 3;
  u32 w = 0;                                            // the 24 stream bits from byte i on, first coefficient in bit 23
  if (i < nbytes) w = (u32)row[i] << 16;
  if (i + 1 < nbytes) w |= (u32)row[i + 1] << 8;
  if (i + 2 < nbytes) w |= (u32)row[i + 2];
  return (__brev(w) >> (8 + (col & 7))) & 0xffffu;      // reversed: coefficient 8 i + s in bit 8 + s
}

// Bits 0 .. cnt - 1 = the cnt <= 16 bytes of the flat [B][N] array from (row, col) on.
__device__ __forceinline__ u32 flat_bits16(const uint8_t *bytes, int N, int nbytes, long row, int col, int cnt) {
  u32 bits = 0;
  for (int j = 0; j < cnt;) {
    const int seg = cnt - j < N - col ? cnt - j : N - col;
    bits |= (row_bits16(bytes + row * nbytes, nbytes, col) & ((1u << seg) - 1u)) << j;
    j += seg;
    col = 0;
    row++;
  }
  return bits;
}

__global__ void __launch_bounds__(MB_THREADS) k_bytes_to_rows(int N, int nbytes, const uint8_t *__restrict__ bytes, long total,
                                                              uint8_t *__restrict__ m) {
  const long head_room = (long)(-(uintptr_t)m & 15);
  const long head = head_room < total ? head_room : total;
  const long nvec = (total - head) >> 4;
  const long tid = (long)blockIdx.x * MB_THREADS + threadIdx.x, stride = (long)gridDim.x * MB_THREADS;
  if (tid < nvec) {
    // (row, col) of this lane's 16 bytes: one division, then steps of the grid's stride
    const long pos = head + 16 * tid, step = 16 * stride;
    long row = pos / N;
    int col = (int)(pos - row * N);
    const long step_rows = step / N;
    const int step_cols = (int)(step - step_rows * N);
    for (long i = tid; i < nvec; i += stride) {
      const u32 bits = flat_bits16(bytes, N, nbytes, row, col, 16);
      u32x4 o;
#pragma unroll
      for (int c = 0; c < 4; c++) o[c] = nibble_to_bytes((bits >> (4 * c)) & 15u);
      *(u32x4 *)(m + head + 16 * i) = o;
      row += step_rows;
      col += step_cols;
      if (col >= N) { col -= N; row++; }
    }
  }
  // the < 16 bytes in front of the first aligned address and behind the last one: one lane each (of different waves)
  if (blockIdx.x == gridDim.x - 1 && (threadIdx.x == 0 || threadIdx.x == 64)) {
    const long at = threadIdx.x == 0 ? 0 : head + 16 * nvec;
    const int cnt = (int)(threadIdx.x == 0 ? head : total - at);
    if (cnt > 0) {
      const long row = at / N;
      const u32 bits = flat_bits16(bytes, N, nbytes, row, (int)(at - row * N), cnt);
      for (int j = 0; j < cnt; j++) m[at + j] = (uint8_t)((bits >> j) & 1u);
    }
  }
}

// ---- rows -> bytes ------------------------------------------------------------------------------------------------------------------

// The 16 bytes at p (16-byte aligned); bytes outside the array [lo, hi) read as 0 and are not touched.
__device__ __forceinline__ u32x4 load_piece(const uint8_t *p, const uint8_t *lo, const uint8_t *hi) {
  if (p >= lo && p + 16 <= hi) return *(const u32x4 *)p;
  u32x4 v = {0u, 0u, 0u, 0u};
#pragma unroll
  for (int j = 0; j < 16; j++)
    if (p + j >= lo && p + j < hi) v[j >> 2] |= (u32)p[j] << (8 * (j & 3));
  return v;
}

// Bit t of the result = bit 0 of byte t of d.
__device__ __forceinline__ u32 gather_low_bits(u32 d) { return ((d & 0x01010101u) * 0x01020408u) >> 24; }

// One piece of a tile: `off` = offset of its byte 0 from the tile's first byte (-15 .. tlen - 1); the tile is tlen bytes = whole rows
// of N, the first `msg` coefficients of a row are message bits.
__device__ __forceinline__ void deposit_piece(const u32x4 v, int off, int tlen, int N, int msg, u32 *s_bits, u32 *s_flags) {
  u32 one = 0, big = 0;                                 // per byte of the piece: its bit 0; whether it is above 1
#pragma unroll
  for (int c = 0; c < 4; c++) {
    const u32 d = v[c];
    one |= gather_low_bits(d) << (4 * c);
    big |= gather_low_bits(((((d >> 1) & 0x7f7f7f7fu) + 0x7f7f7f7fu) & 0x80808080u) >> 7) << (4 * c);
  }
  const u32 nz = one | big;
  int j = off < 0 ? -off : 0;
  const int end = tlen - off < 16 ? tlen - off : 16;
  u32 row = (u32)(off + j) / (u32)N;
  int col = off + j - (int)row * N;
  while (j < end) {
    const int seg = end - j < N - col ? end - j : N - col;
    const int nm = msg - col < 0 ? 0 : (msg - col < seg ? msg - col : seg);     // message coefficients among the seg
    const u32 all = (1u << seg) - 1u, mm = (1u << nm) - 1u;
    const u32 b = (one >> j) & mm;
    u32 f = 0;
    if ((big >> j) & mm) f |= NTRU_FLAG_NOT_BITS;
    if ((nz >> j) & all & ~mm) f |= NTRU_FLAG_PAD_NONZERO;
    if (b) {
      const u32 at = row * (u32)msg + (u32)col;         // coefficient k of row r in bit r * msg + k of the image, byte-wise little endian
      const unsigned long long sh = (unsigned long long)b << (at & 31u);
      atomicOr(&s_bits[at >> 5], (u32)sh);
      if (sh >> 32) atomicOr(&s_bits[(at >> 5) + 1], (u32)(sh >> 32));
    }
    if (f) atomicOr(&s_flags[row >> 2], f << (8 * (row & 3u)));
    j += seg;
    col = 0;
    row++;
  }
}

// Writes the first len bytes of the LDS image to dst: aligned 16-byte stores, the < 16 bytes at either end one by one.  REV: reverse
// the bits of every byte (the image holds the first coefficient of a byte in bit 0, the message has it in bit 7).
template <bool REV>
__device__ __forceinline__ void flush_image(const u32 *lds, uint8_t *dst, int len) {
  const int head_room = (int)(-(uintptr_t)dst & 15);
  const int head = head_room < len ? head_room : len;
  const int nv = (len - head) >> 4;
  for (int i = threadIdx.x; i < nv; i += MB_THREADS) {
    const int o = head + 16 * i, w = o >> 2;
    u32 d[5];
#pragma unroll
    for (int k = 0; k < 5; k++) d[k] = lds[w + k];
    u32x4 out;
#pragma unroll
    for (int k = 0; k < 4; k++) {
      const u32 x = __builtin_amdgcn_alignbyte(d[k + 1], d[k], (u32)(o & 3));
      out[k] = REV ? __builtin_bswap32(__brev(x)) : x;
    }
    *(u32x4 *)(dst + o) = out;
  }
  const int tail = head + 16 * nv, edge = head + (len - tail);
  for (int i = threadIdx.x; i < edge; i += MB_THREADS) {
    const int o = i < head ? i : tail + (i - head);
    const u32 x = (lds[o >> 2] >> (8 * (o & 3))) & 0xffu;
    dst[o] = (uint8_t)(REV ? __brev(x) >> 24 : x);
  }
}

__global__ void __launch_bounds__(MB_THREADS) k_rows_to_bytes(int N, int nbytes, const uint8_t *__restrict__ value, long B, int R,
                                                              uint8_t *__restrict__ bytes, uint8_t *__restrict__ flags) {
  __shared__ u32 s_bits[MB_LDS_WORDS];
  __shared__ u32 s_flags[MB_LDS_WORDS];
  const int tid = threadIdx.x, msg = 8 * nbytes;
  const uint8_t *vend = value + B * N;
  const long ntiles = (B + R - 1) / R;
  for (long t = blockIdx.x; t < ntiles; t += gridDim.x) {
    const long r0 = t * R;
    const int rows = (int)(B - r0 < R ? B - r0 : R);
    const uint8_t *ts = value + r0 * N;
    const int tlen = rows * N;
    const int lead = (int)((uintptr_t)ts & 15);                   // bytes between the aligned address at or below the tile and the tile
    const int npieces = (lead + tlen + 15) >> 4;
    for (int i = tid; i < (rows * nbytes + 3) / 4 + 5; i += MB_THREADS) s_bits[i] = 0;
    for (int i = tid; i < (rows + 3) / 4 + 5; i += MB_THREADS) s_flags[i] = 0;
    __syncthreads();
    for (int c0 = 0; c0 < npieces; c0 += 4 * MB_THREADS) {       // four pieces per lane in flight
      u32x4 v[4];
#pragma unroll
      for (int k = 0; k < 4; k++) {
        const int c = c0 + k * MB_THREADS + tid;
        v[k] = u32x4{0u, 0u, 0u, 0u};
        if (c < npieces) v[k] = load_piece(ts - lead + 16 * (long)c, value, vend);
      }
#pragma unroll
      for (int k = 0; k < 4; k++) {
        const int c = c0 + k * MB_THREADS + tid;
        if (c < npieces) deposit_piece(v[k], 16 * c - lead, tlen, N, msg, s_bits, s_flags);
      }
    }
    __syncthreads();
    flush_image<true>(s_bits, bytes + r0 * nbytes, rows * nbytes);
    if (flags) flush_image<false>(s_flags, flags + r0, rows);
    __syncthreads();                                              // the next tile clears the images
  }
}

// ---- host side --------------------------------------------------------------------------------------------------------------------

int check_bytes_args(const ntru_engine *eng, int N, int nbytes, int64_t B, const char *who) {
  if (N < 8 || N > NTRU_MAX_N)
    return fail(NTRU_ERR_ARG, std::string(who) + ": need 8 <= N <= " + std::to_string(NTRU_MAX_N) + ", got N = " + std::to_string(N));
  if (nbytes < 1 || nbytes > N / 8)
    return fail(NTRU_ERR_ARG, std::string(who) + ": need 1 <= nbytes <= N / 8 = " + std::to_string(N / 8) + ", got " + std::to_string(nbytes));
  if (B < 0) return fail(NTRU_ERR_ARG, std::string(who) + ": negative batch size");
  if (!eng) return fail(NTRU_ERR_ARG, "engine is NULL");
  return NTRU_OK;
}

dim3 grid_of(const ntru_engine *eng, long work_blocks) {
  const long cap = (long)eng->cus * MB_BLOCKS_PER_CU;
  return dim3((unsigned)(work_blocks < 1 ? 1 : (work_blocks > cap ? cap : work_blocks)));
}

}  // namespace

extern "C" int ntru_bytes_to_rows_dev(ntru_engine_t *eng, int N, int nbytes, const uint8_t *d_bytes, int64_t B, uint8_t *d_m) {
  if (int rc = check_bytes_args(eng, N, nbytes, B, "ntru_bytes_to_rows")) return rc;
  if (B == 0) return NTRU_OK;
  if (!d_bytes || !d_m) return fail(NTRU_ERR_ARG, "ntru_bytes_to_rows: NULL buffer");
  HIP_TRY(hipSetDevice(eng->device));
  const long total = (long)B * N;
  hipLaunchKernelGGL(k_bytes_to_rows, grid_of(eng, (total / 16 + MB_THREADS - 1) / MB_THREADS), dim3(MB_THREADS), 0, eng->stream, N, nbytes,
                     d_bytes, total, d_m);
  HIP_TRY(hipGetLastError());
  note_kernel(eng, "k_bytes_to_rows");
  return NTRU_OK;
}

extern "C" int ntru_rows_to_bytes_dev(ntru_engine_t *eng, int N, int nbytes, const uint8_t *d_value, int64_t B, uint8_t *d_bytes,
                                      uint8_t *d_flags) {
  if (int rc = check_bytes_args(eng, N, nbytes, B, "ntru_rows_to_bytes")) return rc;
  if (B == 0) return NTRU_OK;
  if (!d_value || !d_bytes) return fail(NTRU_ERR_ARG, "ntru_rows_to_bytes: NULL buffer");
  HIP_TRY(hipSetDevice(eng->device));
  const int R = MB_TILE_BYTES / N;                       // >= 8 rows: N <= NTRU_MAX_N
  hipLaunchKernelGGL(k_rows_to_bytes, grid_of(eng, ((long)B + R - 1) / R), dim3(MB_THREADS), 0, eng->stream, N, nbytes, d_value, (long)B, R,
                     d_bytes, d_flags);
  HIP_TRY(hipGetLastError());
  note_kernel(eng, "k_rows_to_bytes");
  return NTRU_OK;
}

extern "C" int ntru_encrypt_bytes_batch_dev(ntru_engine_t *eng, int N, int q, int nbytes, const uint16_t *d_h, const uint8_t *d_r,
                                            const uint8_t *d_bytes, int64_t B, uint16_t *d_e, uint16_t *d_quotE) {
  if (int rc = check_bytes_args(eng, N, nbytes, B, "ntru_encrypt_bytes_batch")) return rc;
  if (int rc = ntru_encrypt_batch_dev(eng, N, q, nullptr, nullptr, nullptr, 0, nullptr, nullptr)) return rc;   // parameter checks
  if (B == 0) return NTRU_OK;
  if (!d_h || !d_r || !d_bytes || !d_e) return fail(NTRU_ERR_ARG, "ntru_encrypt_bytes_batch: NULL buffer");
  ScratchHold hold(eng, (size_t)std::min<int64_t>(B, MB_PASS) * N);
  if (hold.rc) return hold.rc;
  uint8_t *d_m = (uint8_t *)hold.p;
  return for_each_pass(B, MB_PASS, [&](int64_t o, int64_t n) -> int {
    if (int rc = ntru_bytes_to_rows_dev(eng, N, nbytes, d_bytes + o * nbytes, n, d_m)) return rc;
    return ntru_encrypt_batch_dev(eng, N, q, d_h, d_r + o * N, d_m, n, d_e + o * N, rows_at(d_quotE, o * N));
  });
}

extern "C" int ntru_decrypt_bytes_batch_dev(ntru_engine_t *eng, int N, int q, int p, int nbytes, const int8_t *d_f, const uint8_t *d_fp,
                                            const uint16_t *d_e, int64_t B, uint8_t *d_bytes, uint8_t *d_flags) {
  if (int rc = check_bytes_args(eng, N, nbytes, B, "ntru_decrypt_bytes_batch")) return rc;
  if (int rc = ntru_decrypt_batch_dev(eng, N, q, p, nullptr, nullptr, nullptr, 0, nullptr, nullptr, nullptr, nullptr)) return rc;
  if (B == 0) return NTRU_OK;
  if (!d_f || !d_fp || !d_e || !d_bytes) return fail(NTRU_ERR_ARG, "ntru_decrypt_bytes_batch: NULL buffer");
  ScratchHold hold(eng, (size_t)std::min<int64_t>(B, MB_PASS) * N);
  if (hold.rc) return hold.rc;
  uint8_t *d_value = (uint8_t *)hold.p;
  return for_each_pass(B, MB_PASS, [&](int64_t o, int64_t n) -> int {
    if (int rc = ntru_decrypt_batch_dev(eng, N, q, p, d_f, d_fp, d_e + o * N, n, d_value, nullptr, nullptr, nullptr)) return rc;
    return ntru_rows_to_bytes_dev(eng, N, nbytes, d_value, n, d_bytes + o * nbytes, rows_at(d_flags, o));
  });
}

// ---- host-pointer form (the regular ones -- bytes_to_rows, rows_to_bytes, encrypt_bytes, decrypt_bytes -- are in ntru_host.hip) -------

// ntru_pipeline_batch with the plaintext as bytes at both ends: sampler -> bytes_to_rows -> encryptBits -> decryptBits -> rows_to_bytes
// per chunk.  m and value are device-only rows of the chunk; msg, msg_out and flags are what crosses the bus.
extern "C" int ntru_pipeline_bytes_batch(ntru_engine_t *eng, int N, int q, int p, const uint16_t *h, const int8_t *f, const uint8_t *fp,
                                         const uint32_t *key, uint64_t first_item, int n1, int n2, const uint8_t *r, int nbytes,
                                         const uint8_t *msg, int64_t B, uint8_t *r_out, uint16_t *e, uint8_t *msg_out, uint8_t *flags) {
  if (int rc = check_bytes_args(eng, N, nbytes, B, "ntru_pipeline_bytes_batch")) return rc;
  const bool decrypt = f != nullptr || fp != nullptr;
  if (decrypt && (!f || !fp)) return fail(NTRU_ERR_ARG, "ntru_pipeline_bytes_batch: the decrypt stage needs both f and fp");
  if (!decrypt && (msg_out || flags)) return fail(NTRU_ERR_ARG, "ntru_pipeline_bytes_batch: `msg_out` and `flags` need the decrypt stage (f, fp)");
  if ((key != nullptr) == (r != nullptr)) return fail(NTRU_ERR_ARG, "ntru_pipeline_bytes_batch: give either a sampler key or r");
  if (!e && !msg_out && !flags && !(r_out && key)) return fail(NTRU_ERR_ARG, "ntru_pipeline_bytes_batch: no output asked for");
  // parameter checks of every stage (B = 0 calls return after them)
  if (int rc = ntru_encrypt_batch_dev(eng, N, q, nullptr, nullptr, nullptr, 0, nullptr, nullptr)) return rc;
  if (decrypt) if (int rc = ntru_decrypt_batch_dev(eng, N, q, p, nullptr, nullptr, nullptr, 0, nullptr, nullptr, nullptr, nullptr)) return rc;
  if (key) if (int rc = ntru_sample_ternary_dev(eng, N, n1, n2, p - 1, key, first_item, 0, nullptr)) return rc;
  if (B == 0) return NTRU_OK;
  if (!h || !msg) return fail(NTRU_ERR_ARG, "ntru_pipeline_bytes_batch: NULL buffer");
  const bool collect = msg_out || flags;
  Pipeline P(eng);
  const int ih = P.in(h, (size_t)N * 2, true), ib = P.in(msg, nbytes);
  const int jf = decrypt ? P.in(f, N, true) : -1, jfp = decrypt ? P.in(fp, N, true) : -1;
  const int ir = r ? P.in(r, N) : (r_out ? P.out(r_out, N) : P.tmp(N));
  const int ie = e ? P.out(e, (size_t)N * 2) : P.tmp((size_t)N * 2);
  const int im = P.tmp(N);
  const int iv = collect ? P.tmp(N) : -1;
  const int io = !collect ? -1 : (msg_out ? P.out(msg_out, nbytes) : P.tmp(nbytes));
  const int ifl = flags ? P.out(flags, 1) : -1;
  return P.run(B, ntru_chunk_items(B), [&](int64_t o, int64_t n, void **d) {
    if (key) if (int rc = ntru_sample_ternary_dev(eng, N, n1, n2, p - 1, key, first_item + (uint64_t)o, n, (uint8_t *)d[ir])) return rc;
    if (int rc = ntru_bytes_to_rows_dev(eng, N, nbytes, (const uint8_t *)d[ib], n, (uint8_t *)d[im])) return rc;
    if (int rc = ntru_encrypt_batch_dev(eng, N, q, (const uint16_t *)d[ih], (const uint8_t *)d[ir], (const uint8_t *)d[im], n,
                                        (uint16_t *)d[ie], nullptr)) return rc;
    if (!collect) return (int)NTRU_OK;
    if (int rc = ntru_decrypt_batch_dev(eng, N, q, p, (const int8_t *)d[jf], (const uint8_t *)d[jfp], (const uint16_t *)d[ie], n,
                                        (uint8_t *)d[iv], nullptr, nullptr, nullptr)) return rc;
    return ntru_rows_to_bytes_dev(eng, N, nbytes, (const uint8_t *)d[iv], n, (uint8_t *)d[io], ifl >= 0 ? (uint8_t *)d[ifl] : nullptr);
  });
}
