// kernels_common.h -- what the kernel translation units of libntru_engine.so share: scalar types, the workgroup shape, small device
// helpers, and the host-side launch helpers (persistent launch with the grid from the occupancy query).
#ifndef NTRU_KERNELS_COMMON_H
#define NTRU_KERNELS_COMMON_H

#include <hip/hip_runtime.h>

#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <type_traits>

#include "engine_internal.h"

typedef unsigned short u16;
typedef unsigned int u32;
typedef u16 u16x2 __attribute__((ext_vector_type(2)));
typedef u16 u16x8 __attribute__((ext_vector_type(8)));      // 16 bytes per lane and access of the streaming elementwise kernels

#define WAVES_PER_BLOCK 4
#define BLOCK_THREADS (WAVES_PER_BLOCK * 64)

static __device__ __forceinline__ u16x2 as_pair(u32 v) { return __builtin_bit_cast(u16x2, v); }
static __device__ __forceinline__ u32 as_u32(u16x2 v) { return __builtin_bit_cast(u32, v); }

// x mod a small runtime modulus; p = 3 (every NTRU parameter set) gets the constant-divisor sequence.
static __device__ __forceinline__ u32 mod_small(u32 x, u32 m) { return m == 3u ? x % 3u : x % m; }

// The centred lift followed by mod p, index.js:117: x > q/2 ? (x + 1) % p : x % p, with `add` in place of its 1 (ntru_lift_addend).
static __device__ __forceinline__ u32 lift_value(u32 x, u32 q, u32 p, u32 add) { return mod_small(2 * x > q ? x + add : x, p); }

// Order this wave's LDS writes before its later LDS reads (regions touched here are private to one wave).
static __device__ __forceinline__ void wave_lds_fence() {
  __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "workgroup");
  __builtin_amdgcn_wave_barrier();
}

// How many lanes below this one are set in a wave ballot.
static __device__ __forceinline__ u32 lanes_below(unsigned long long ballot) {
  return __builtin_amdgcn_mbcnt_hi((u32)(ballot >> 32), __builtin_amdgcn_mbcnt_lo((u32)ballot, 0u));
}

// Inclusive prefix sum of s[0 .. THREADS) by a workgroup of THREADS lanes (Hillis-Steele, in place).  The caller has written s[tid]
// and passed a barrier; the last thing done here is a barrier.
template <int THREADS>
static __device__ __forceinline__ void wg_inclusive_scan(u32 *s, int tid) {
  for (int d = 1; d < THREADS; d <<= 1) {
    const u32 v = tid >= d ? s[tid - d] : 0u;
    __syncthreads();
    s[tid] += v;
    __syncthreads();
  }
}

// ---- the tag of the scanning and counting calls (scan_hits.hip, count_bytes.hip) ---------------------------------------------------
// At most NTRU_SCAN_MAX_TAG bytes, read on the host when the call enqueues; it reaches the kernels by value.
static_assert(NTRU_SCAN_MAX_TAG == 32, "ScanTag holds eight words");
struct ScanTag {
  u32 w[NTRU_SCAN_MAX_TAG / 4];                // byte j of the tag in bits 8 (j % 4) .. of word j / 4
  int off, len;
};
static inline ScanTag tag_of(int tag_off, int tag_len, const uint8_t *tag) {
  ScanTag t;
  memset(&t, 0, sizeof t);
  for (int j = 0; j < tag_len; j++) t.w[j >> 2] |= (u32)tag[j] << (8 * (j & 3));
  t.off = tag_off;
  t.len = tag_len;
  return t;
}
// Do the bytes [tag.off, tag.off + tag.len) of the message m equal the tag?  (tag.len is uniform: the loop is scalar control flow
// around byte loads.)
static __device__ __forceinline__ bool tag_matches(const uint8_t *__restrict__ m, const ScanTag &tag) {
  m += tag.off;
  u32 diff = 0;
#pragma unroll
  for (int j = 0; j < NTRU_SCAN_MAX_TAG; j++)
    if (j < tag.len) diff |= (u32)m[j] ^ ((tag.w[j >> 2] >> (8 * (j & 3))) & 0xffu);
  return diff == 0;
}

// ---- bit spreads between packed small values and bytes ---------------------------------------------------------------------------
// bit j of a nibble -> bit 0 of byte j, and back
static __host__ __device__ __forceinline__ constexpr u32 nibble_to_bytes(u32 nib) { return (nib * 0x00204081u) & 0x01010101u; }
static __host__ __device__ __forceinline__ constexpr u32 bytes_to_nibble(u32 b) { return ((b * 0x00204081u) >> 21) & 15u; }
// four 2-bit values at bit `sh` of the four bytes of d -> one byte, value j in bits 2j .. 2j + 1
static __host__ __device__ __forceinline__ constexpr u32 pack2x4(u32 d, int sh) {
  u32 t = (d >> sh) & 0x03030303u;
  t |= t >> 6;
  return (t | (t >> 12)) & 0xFFu;
}
// the same for sixteen values in four dwords of bytes -> one dword (packOutput's 2-bit fields: value j in bits 2j .. 2j + 1)
static __host__ __device__ __forceinline__ constexpr u32 pack2x16(const u32 (&d)[4], int sh) {
  u32 out = 0;
  for (int c = 0; c < 4; c++) out |= pack2x4(d[c], sh) << (8 * c);
  return out;
}
// the inverse of pack2x4(., 0): the low byte of b, four 2-bit symbols -> four bytes
static __host__ __device__ __forceinline__ constexpr u32 unpack2x4(u32 b) {
  u32 t = b & 0xFFu;
  t = (t | (t << 12)) & 0x000F000Fu;
  return (t | (t << 6)) & 0x03030303u;
}
constexpr bool bit_spreads_invert() {
  for (u32 n = 0; n < 16; n++)
    if (bytes_to_nibble(nibble_to_bytes(n)) != n) return false;
  for (u32 b = 0; b < 256; b++) {
    for (int sh = 0; sh < 8; sh += 2)
      if (pack2x4(unpack2x4(b) << sh, sh) != b) return false;
    const u32 d[4] = {unpack2x4(b), unpack2x4(b ^ 0xFFu), unpack2x4(b >> 1), unpack2x4(b * 7u)};
    if (pack2x16(d, 0) != (b | (b ^ 0xFFu) << 8 | (b >> 1) << 16 | ((b * 7u) & 0xFFu) << 24)) return false;
  }
  return true;
}
static_assert(bit_spreads_invert(), "unpack-then-pack is the identity on every byte, and so is spread-then-gather on every nibble");

// Launches a persistent kernel on eng->stream: as many workgroups as are co-resident (occupancy query for this kernel, block size
// and LDS size) x CUs, capped by the work available (work_blocks >= 1).  A grid larger than residency would run its tail at a
// fraction of the chip.  The dynamic-LDS limit of a kernel is raised at its first use, inside ntru_blocks_per_cu.
template <class Kern, class... Args>
static int launch_resident(ntru_engine *eng, Kern kern, long work_blocks, int threads, size_t lds, Args... args) {
  int per_cu = 0;
  if (int rc = ntru_blocks_per_cu(eng, (const void *)kern, threads, lds, &per_cu)) return rc;
  const long resident = (long)eng->cus * per_cu;
  hipLaunchKernelGGL(kern, dim3((unsigned)(work_blocks < resident ? work_blocks : resident)), dim3(threads), lds, eng->stream, args...);
  HIP_TRY(hipGetLastError());
  return NTRU_OK;
}

#endif
