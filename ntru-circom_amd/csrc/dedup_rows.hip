// dedup_rows.hip -- MI355X (gfx950): finding the duplicate ciphertexts of a batch on the device, dense or packed rows, against an optional
// set of rows accepted earlier (include/ntru_engine.h "removing duplicates").  Kernels, *_dev entry points and the host-pointer forms.
//
// Two rows are equal when every coefficient agrees modulo `mod` (any 2 <= mod <= 65536).  The S prior rows and the B new rows form one
// index space 0 .. S + B - 1; first[b] is the smallest index of a row equal to new row b, `unique` lists the new rows that are their
// own first occurrence, in row order.
//
//   k_dedup_fingerprint   fp[i] = (sum over k of term(salt, k, row_i[k] mod `mod`)) & keep, a sum modulo 2^64 of multiply-xorshift terms
//                         keyed by the position, so neither the lane that adds a term nor the order of the additions matters.  A row
//                         is U units (dense: eight u16 coefficients, one 16-byte load; packed: one field element, two 16-byte
//                         loads); U <= 32: floor(64 / U) rows sit side by side in a wave, else a wave walks one row.
//                         The last unit of a dense row is masked by the column index; the last rows of an array, where the 20 bytes
//                         of load8_raw would leave it, are read element by element (pairs8_checked).
//   the sort              ntru_argsort_keys_dev (permutation.hip) of the fingerprints: stable, so inside a run of equal fingerprints the
//                         indices ascend.
//   k_dedup_neighbours    sorted position j against j - 1 ONLY: flag[j] = 2 (fingerprints equal) | 1 (and the reduced rows equal).
//                         2^20 identical rows cost one row comparison each.
//   k_dedup_walk          the heads of a segment (flag & 1 == 0) whose fingerprint equals their predecessor's (flag == 2): true
//                         collisions, B^2 / 2^65 expected at 64 bits.  Each walks back through its fingerprint run, compares the
//                         full rows with the earlier heads and keeps the furthest-back equal one: res[j] = its index.
//   k_dedup_mark / k_dedup_offsets / k_dedup_emit
//                         compaction of the entries with flag & 1 == 0, as scan_hits.hip does it: one count per 256 entries, the
//                         exclusive prefix over the blocks in one workgroup with a carry, positions from offset + waves before +
//                         lanes below.  Used twice: the segment heads in sorted order, and the first occurrences in row order.
//   k_dedup_assign        position j -> its segment (offset + heads up to j) -> the head -> the head's index, or res[] for a collision
//                         head; first[] and the duplicate flag of the new rows.
// Positions come from prefix sums only: no global atomic, hence the same bytes whatever the launch shape, the salt or the width of the
// fingerprint.  Every dependency between workgroups is a kernel boundary: no workgroup waits for another.
#include <hip/hip_runtime.h>

#include <cstdint>
#include <cstdio>
#include <cstring>
#include <string>

#include "kernels_common.h"
#include "sum_groups_common.h"

namespace {

constexpr int DD_THREADS = 256;                  // lanes per workgroup of every kernel here = entries per compaction block
constexpr int DD_WAVES = DD_THREADS / 64;
typedef u32x4 u32x4_a8 __attribute__((aligned(8)));

// The prior rows and the new rows as one index space, and how a wave sees a row.
struct DdRows {
  const void *prior, *rows;   // dense: u16 [.][N]; packed: u64 [.][os][4]
  long S, T;                  // rows before the new ones; all rows
  int N;
  u32 mod, mask, recip;       // mask = mod - 1 for a power of two, else 0 and recip = ceil(2^32 / mod)
  int os, bits, per;          // the packed geometry (dense: unused)
  int U, L, side;             // units per row; lanes per row (U <= 32: U, else 64); rows per wave
};

// c mod `mod` for c < 65536: a mask, or floor(c / mod) = (c * ceil(2^32 / mod)) >> 32, exact because c * (recip * mod - 2^32) < 2^32.
__device__ __forceinline__ u32 dd_reduce(const DdRows &R, u32 c) { return R.mask ? c & R.mask : c - __umulhi(c, R.recip) * R.mod; }

// One term of the fingerprint: position and value in, a multiply-xorshift out (a bijection of the 64-bit word under any salt).
__device__ __forceinline__ u64 dd_term(u64 salt, u32 k, u32 c) {
  u64 z = (salt ^ (((u64)k << 32) | c)) * 0x9E3779B97F4A7C15ull;
  z ^= z >> 32;
  z *= 0xD6E8FEB86659FD93ull;
  return z ^ (z >> 32);
}

struct RowAt {
  const void *p;              // the row
  const u16 *lim;             // dense: the end of the array the row lies in
};
template <bool PACKED>
__device__ __forceinline__ RowAt row_at(const DdRows &R, long i) {
  const bool old = i < R.S;
  const void *base = old ? R.prior : R.rows;
  const long j = old ? i : i - R.S, n = old ? R.S : R.T - R.S;
  RowAt r;
  if (PACKED) {
    r.p = (const u64 *)base + j * R.os * 4;
    r.lim = nullptr;
  } else {
    r.p = (const u16 *)base + j * R.N;
    r.lim = (const u16 *)base + n * R.N;
  }
  return r;
}

// Eight coefficients of a dense row from p on, two per dword.
__device__ __forceinline__ void dense8(const u16 *p, const u16 *lim, u32 (&x)[4]) {
  if (p + 10 <= lim) {
    const u32 sh = half_dword(p);
    u32 d[5];
    load8_raw(p, sh, d);
    pairs8(sh, d, x);
  } else pairs8_checked(p, lim, x);
}

struct Limbs { u64 l[4]; };
__device__ __forceinline__ Limbs element_at(const u64 *p) {
  const u32x4 lo = *(const u32x4_a8 *)p, hi = *(const u32x4_a8 *)(p + 2);
  Limbs e;
  e.l[0] = (u64)lo[0] | ((u64)lo[1] << 32); e.l[1] = (u64)lo[2] | ((u64)lo[3] << 32);
  e.l[2] = (u64)hi[0] | ((u64)hi[1] << 32); e.l[3] = (u64)hi[2] | ((u64)hi[3] << 32);
  return e;
}
// the next field moves down to bit 0 (1 <= bits <= 16)
__device__ __forceinline__ void next_field(Limbs &e, int bits) {
  e.l[0] = (e.l[0] >> bits) | (e.l[1] << (64 - bits));
  e.l[1] = (e.l[1] >> bits) | (e.l[2] << (64 - bits));
  e.l[2] = (e.l[2] >> bits) | (e.l[3] << (64 - bits));
  e.l[3] >>= bits;
}

// f(k, a_k mod `mod`, b_k mod `mod`) for every coefficient k < N of unit u of the rows a and b (TWO == false: b is not read, b_k = 0).
// Fields with index >= N and the bits of an element above per * bits never reach f.
template <bool PACKED, bool TWO, class F>
__device__ __forceinline__ void visit_unit(const DdRows &R, const RowAt &a, const RowAt &b, int u, F f) {
  if (PACKED) {
    const int k0 = u * R.per;
    int nv = R.N - k0 < R.per ? R.N - k0 : R.per;
    if (nv <= 0) return;
    Limbs ea = element_at((const u64 *)a.p + 4 * u), eb = ea;
    if (TWO) eb = element_at((const u64 *)b.p + 4 * u);
    const u32 fm = (1u << R.bits) - 1u;
    for (int j = 0; j < nv; j++) {
      f((u32)(k0 + j), dd_reduce(R, (u32)ea.l[0] & fm), TWO ? dd_reduce(R, (u32)eb.l[0] & fm) : 0u);
      next_field(ea, R.bits);
      if (TWO) next_field(eb, R.bits);
    }
  } else {
    u32 xa[4], xb[4] = {0u, 0u, 0u, 0u};
    dense8((const u16 *)a.p + 8 * u, a.lim, xa);
    if (TWO) dense8((const u16 *)b.p + 8 * u, b.lim, xb);
#pragma unroll
    for (int i = 0; i < 8; i++) {
      const int k = 8 * u + i;
      if (k < R.N) f((u32)k, dd_reduce(R, (xa[i >> 1] >> (16 * (i & 1))) & 0xffffu), dd_reduce(R, (xb[i >> 1] >> (16 * (i & 1))) & 0xffffu));
    }
  }
}

// Do the reduced rows i and j differ in one of this lane's units (lane ul of the L lanes of a row)?
template <bool PACKED>
__device__ __forceinline__ u32 rows_differ(const DdRows &R, long i, long j, int ul, int L) {
  const RowAt a = row_at<PACKED>(R, i), b = row_at<PACKED>(R, j);
  u32 diff = 0;
  for (int u = ul; u < R.U; u += L) visit_unit<PACKED, true>(R, a, b, u, [&](u32, u32 ca, u32 cb) { diff |= ca ^ cb; });
  return diff;
}

__device__ __forceinline__ u64 shfl64(u64 v, int src) {
  const u32 lo = (u32)__shfl((int)(u32)v, src, 64), hi = (u32)__shfl((int)(u32)(v >> 32), src, 64);
  return (u64)lo | ((u64)hi << 32);
}

// This lane's place among the rows of its wave.
struct Place {
  int sub, ul;                // row of the wave, lane of the row
  long item;                  // wave * side + sub
  bool active;
};
__device__ __forceinline__ Place place_of(const DdRows &R, long items) {
  const int lane = threadIdx.x & 63;
  const long wave = (long)blockIdx.x * DD_WAVES + (threadIdx.x >> 6);
  Place p;
  p.sub = lane / R.L;
  p.ul = lane - p.sub * R.L;
  p.item = wave * R.side + p.sub;
  p.active = p.sub < R.side && p.item < items;
  return p;
}

template <bool PACKED>
__global__ void __launch_bounds__(DD_THREADS) k_dedup_fingerprint(DdRows R, u64 salt, u64 keep, u64 *__restrict__ fp) {
  const Place pl = place_of(R, R.T);
  u64 acc = 0;
  if (pl.active) {
    const RowAt a = row_at<PACKED>(R, pl.item);
    for (int u = pl.ul; u < R.U; u += R.L) visit_unit<PACKED, false>(R, a, a, u, [&](u32 k, u32 c, u32) { acc += dd_term(salt, k, c); });
  }
  const int lane = threadIdx.x & 63;
  for (int dist = 1; dist < R.L; dist <<= 1) {      // uniform loop: lane ul ends with the sum of lanes ul .. of its row
    const u64 t = shfl64(acc, lane + dist);
    if (pl.ul + dist < R.L) acc += t;
  }
  if (pl.active && pl.ul == 0) fp[pl.item] = acc & keep;
}

// flag[j] for the sorted position j: 0, 2 (the fingerprint of position j - 1 is the same) or 3 (and so is the reduced row).
template <bool PACKED>
__global__ void __launch_bounds__(DD_THREADS) k_dedup_neighbours(DdRows R, const u64 *__restrict__ fp, const long long *__restrict__ order,
                                                                 uint8_t *__restrict__ flag) {
  const Place pl = place_of(R, R.T);
  bool fpeq = false;
  u32 diff = 0;
  if (pl.active && pl.item > 0) {
    const u64 a = (u64)order[pl.item], b = (u64)order[pl.item - 1];
    if (a < (u64)R.T && b < (u64)R.T && fp[a] == fp[b]) {
      fpeq = true;
      diff = rows_differ<PACKED>(R, (long)a, (long)b, pl.ul, R.L);
    }
  }
  const u64 differ = __ballot(diff != 0);            // every lane of the wave is here
  if (pl.active && pl.ul == 0) {
    const u64 mine = (R.L == 64 ? ~0ull : (1ull << R.L) - 1ull) << (pl.sub * R.L);
    flag[pl.item] = fpeq ? ((differ & mine) ? 2 : 3) : 0;
  }
}

// One wave per 64 sorted positions; a collision head among them is walked by the whole wave.
template <bool PACKED>
__global__ void __launch_bounds__(DD_THREADS) k_dedup_walk(DdRows R, const long long *__restrict__ order, const uint8_t *__restrict__ flag,
                                                           long long *__restrict__ res) {
  const int lane = threadIdx.x & 63;
  const long first = ((long)blockIdx.x * DD_WAVES + (threadIdx.x >> 6)) * 64;
  if (first >= R.T) return;                         // uniform per wave; no workgroup barrier below
  u64 todo = __ballot(first + lane < R.T && flag[first + lane] == 2);
  while (todo) {                                    // uniform loop
    const long j = first + __builtin_ctzll(todo);
    todo &= todo - 1;
    const u64 a = (u64)order[j];
    long best = j, p = j;
    do {                                            // flag[j] has bit 1, so p - 1 >= 0 lies in the run; the run ends where bit 1 does
      p--;
      const u64 b = (u64)order[p];
      if ((flag[p] & 1) == 0 && a < (u64)R.T && b < (u64)R.T) {           // a head: the rows behind it equal it
        const u32 diff = rows_differ<PACKED>(R, (long)a, (long)b, lane, 64);
        if (__ballot(diff != 0) == 0) best = p;
      }
    } while (p > 0 && (flag[p] & 2));
    if (lane == 0) res[j] = order[best];
  }
}

// counts[block] = the entries of the block with flag & 1 == 0.
__global__ void __launch_bounds__(DD_THREADS) k_dedup_mark(const uint8_t *__restrict__ flag, long n, u32 *__restrict__ counts) {
  __shared__ u32 s_wave[DD_WAVES];
  const int tid = threadIdx.x;
  const long i = (long)blockIdx.x * DD_THREADS + tid;
  const u64 ballot = __ballot(i < n && (flag[i] & 1) == 0);
  if ((tid & 63) == 0) s_wave[tid >> 6] = (u32)__popcll(ballot);
  __syncthreads();
  if (tid == 0) {
    u32 c = 0;
#pragma unroll
    for (int w = 0; w < DD_WAVES; w++) c += s_wave[w];
    counts[blockIdx.x] = c;
  }
}

// One workgroup.  offsets[b] = sum of counts[0 .. b - 1], DD_THREADS blocks per round of a loop with a carry; *total = the sum of all.
__global__ void __launch_bounds__(DD_THREADS) k_dedup_offsets(const u32 *__restrict__ counts, long nblocks, long long *__restrict__ offsets,
                                                              long long *__restrict__ total) {
  __shared__ u32 s_sum[DD_THREADS];
  const int tid = threadIdx.x;
  long long carry = 0;
  for (long b0 = 0; b0 < nblocks; b0 += DD_THREADS) {                       // uniform loop
    const long b = b0 + tid;
    const u32 c = b < nblocks ? counts[b] : 0u;
    s_sum[tid] = c;
    __syncthreads();
    wg_inclusive_scan<DD_THREADS>(s_sum, tid);
    if (b < nblocks) offsets[b] = carry + (long long)(s_sum[tid] - c);
    carry += (long long)s_sum[DD_THREADS - 1];
    __syncthreads();                                                         // every lane has read the round's total
  }
  if (tid == 0 && total) *total = carry;
}

// This entry's rank among the entries of its block with `hit`, and the number of hits of the waves before it.
__device__ __forceinline__ u32 rank_in_block(bool hit, u32 *s_wave) {
  const int tid = threadIdx.x;
  const u64 ballot = __ballot(hit);
  if ((tid & 63) == 0) s_wave[tid >> 6] = (u32)__popcll(ballot);
  __syncthreads();
  u32 before = lanes_below(ballot);
#pragma unroll
  for (int w = 0; w < DD_WAVES; w++)
    if (w < (tid >> 6)) before += s_wave[w];
  return before;
}

// list[offsets[block] + rank] = i for the entries with flag & 1 == 0: ascending.
__global__ void __launch_bounds__(DD_THREADS) k_dedup_emit(const uint8_t *__restrict__ flag, long n, const long long *__restrict__ offsets,
                                                           long long *__restrict__ list) {
  __shared__ u32 s_wave[DD_WAVES];
  const long i = (long)blockIdx.x * DD_THREADS + threadIdx.x;
  const bool hit = i < n && (flag[i] & 1) == 0;
  const u32 rank = rank_in_block(hit, s_wave);
  const long long pos = offsets[blockIdx.x] + rank;
  if (hit && pos < n) list[pos] = i;
}

// Sorted position j: the head of its segment, the head's resolved index; for a new row first[] and dup[] (1: not a first occurrence).
__global__ void __launch_bounds__(DD_THREADS) k_dedup_assign(const uint8_t *__restrict__ flag, long T, long S,
                                                             const long long *__restrict__ offsets, const long long *__restrict__ heads,
                                                             const long long *__restrict__ order, const long long *__restrict__ res,
                                                             long long *__restrict__ first, uint8_t *__restrict__ dup) {
  __shared__ u32 s_wave[DD_WAVES];
  const long j = (long)blockIdx.x * DD_THREADS + threadIdx.x;
  const bool head = j < T && (flag[j] & 1) == 0;
  const u32 rank = rank_in_block(head, s_wave);
  if (j >= T) return;
  const long long seg = offsets[blockIdx.x] + rank + (head ? 1 : 0) - 1;   // position 0 is a head: seg >= 0
  if (seg < 0 || seg >= T) return;
  const long long h = heads[seg];
  if (h < 0 || h >= T) return;
  const long long r = flag[h] == 2 ? res[h] : order[h], idx = order[j];
  if (idx < S || idx >= T) return;
  if (first) first[idx - S] = r;
  dup[idx - S] = r != idx;
}

// ---- host side ----------------------------------------------------------------------------------------------------------------------

struct Work {
  size_t fp, order, res, heads, flag, dup, counts, offsets, total;
};
Work carve_work(int64_t T) {
  const size_t n = (size_t)(T < 1 ? 1 : T), blocks = (n + DD_THREADS - 1) / DD_THREADS;
  Carve c;
  Work w;
  w.fp = c.take(n * 8); w.order = c.take(n * 8); w.res = c.take(n * 8); w.heads = c.take(n * 8);
  w.flag = c.take(n); w.dup = c.take(n); w.counts = c.take(blocks * 4); w.offsets = c.take(blocks * 8);
  w.total = c.total;
  return w;
}

// The checks that need no engine.  *os = 0 for dense rows.
int check_dedup(const std::string &name, bool packed, int N, int mod, const void *prior, int64_t S, const void *rows, int64_t B,
                int fingerprint_bits, const void *work, bool need_work, const void *first, const void *unique, const void *count, int *os,
                int *bits, int *per) {
  if (B < 0) return fail(NTRU_ERR_ARG, name + ": negative batch size");
  if (S < 0) return fail(NTRU_ERR_ARG, name + ": negative number of prior rows");
  if (S > NTRU_DEDUP_MAX_ROWS || B > NTRU_DEDUP_MAX_ROWS - S)
    return fail(NTRU_ERR_ARG, name + ": need S + B <= NTRU_DEDUP_MAX_ROWS = " + std::to_string(NTRU_DEDUP_MAX_ROWS) + ", got " +
                                  std::to_string(S) + " + " + std::to_string(B));
  if (fingerprint_bits < 0 || fingerprint_bits > 64)
    return fail(NTRU_ERR_ARG, name + ": need 0 <= fingerprint_bits <= 64, got " + std::to_string(fingerprint_bits));
  if (int rc = ntru_check_ring_mod(name + ": ", N, mod)) return rc;
  if (!count) return fail(NTRU_ERR_ARG, name + ": count is NULL");
  if (B > 0 && !rows) return fail(NTRU_ERR_ARG, name + ": NULL buffer (" + (packed ? "packed" : "rows") + ")");
  if (B > 0 && need_work && !work) return fail(NTRU_ERR_ARG, name + ": NULL buffer (work)");
  if (S > 0 && !prior) return fail(NTRU_ERR_ARG, name + ": prior is NULL with S > 0");
  *os = 0; *bits = 0; *per = 0;
  if (packed) {
    int al;
    if (int rc = ntru_pack_params(mod - 1, N, bits, per, &al, os)) return rc;
  }
  const size_t row_bytes = packed ? (size_t)*os * 32 : (size_t)N * 2;
  const struct { const void *p; size_t n; const char *what; } r[5] = {{first, (size_t)B * 8, "first"}, {unique, (size_t)B * 8, "unique"},
                                                                      {count, 8, "count"}, {rows, (size_t)B * row_bytes, packed ? "packed" : "rows"},
                                                                      {prior, (size_t)S * row_bytes, "prior"}};
  for (int a = 0; a < 3; a++)
    for (int b = a + 1; b < 5; b++)
      if (ntru_ranges_overlap(r[a].p, r[a].n, r[b].p, r[b].n)) return fail(NTRU_ERR_ARG, name + ": " + r[a].what + " overlaps " + r[b].what);
  return NTRU_OK;
}

// Enqueues everything on eng->stream; B > 0.
int dedup_flow(ntru_engine *eng, bool packed, int N, int mod, int os, int bits, int per, const void *d_prior, int64_t S, const void *d_rows,
               int64_t B, uint64_t salt, int fingerprint_bits, char *d_work, int64_t *d_first, int64_t *d_unique, int64_t *d_count) {
  HIP_TRY(hipSetDevice(eng->device));
  DdRows R;
  R.prior = d_prior; R.rows = d_rows; R.S = S; R.T = S + B; R.N = N;
  R.mod = (u32)mod; R.mask = is_pow2(mod) ? (u32)mod - 1u : 0u;
  R.recip = (u32)((0x100000000ull + (u32)mod - 1u) / (u32)mod);
  R.os = os; R.bits = bits; R.per = per;
  R.U = packed ? os : (N + 7) / 8;
  R.L = R.U <= 32 ? R.U : 64;
  R.side = 64 / R.L;
  const long T = R.T;
  const Work w = carve_work(T);
  u64 *fp = (u64 *)(d_work + w.fp);
  long long *order = (long long *)(d_work + w.order), *res = (long long *)(d_work + w.res), *heads = (long long *)(d_work + w.heads),
            *offsets = (long long *)(d_work + w.offsets);
  uint8_t *flag = (uint8_t *)d_work + w.flag, *dup = (uint8_t *)d_work + w.dup;
  u32 *counts = (u32 *)(d_work + w.counts);
  const u64 keep = fingerprint_bits == 64 ? ~0ull : (1ull << fingerprint_bits) - 1ull;
  const dim3 block(DD_THREADS);
  const dim3 by_row((unsigned)(((T + R.side - 1) / R.side + DD_WAVES - 1) / DD_WAVES));
  const dim3 by_entry((unsigned)((T + DD_THREADS - 1) / DD_THREADS)), by_new((unsigned)((B + DD_THREADS - 1) / DD_THREADS));
  const hipStream_t st = eng->stream;
  if (packed) hipLaunchKernelGGL(k_dedup_fingerprint<true>, by_row, block, 0, st, R, (u64)salt, keep, fp);
  else hipLaunchKernelGGL(k_dedup_fingerprint<false>, by_row, block, 0, st, R, (u64)salt, keep, fp);
  HIP_TRY(hipGetLastError());
  if (int rc = ntru_argsort_keys_dev(eng, (const uint64_t *)fp, T, (int64_t *)order)) return rc;
  if (packed) {
    hipLaunchKernelGGL(k_dedup_neighbours<true>, by_row, block, 0, st, R, (const u64 *)fp, (const long long *)order, flag);
    hipLaunchKernelGGL(k_dedup_walk<true>, by_entry, block, 0, st, R, (const long long *)order, (const uint8_t *)flag, res);
  } else {
    hipLaunchKernelGGL(k_dedup_neighbours<false>, by_row, block, 0, st, R, (const u64 *)fp, (const long long *)order, flag);
    hipLaunchKernelGGL(k_dedup_walk<false>, by_entry, block, 0, st, R, (const long long *)order, (const uint8_t *)flag, res);
  }
  // the segment heads, in sorted order
  hipLaunchKernelGGL(k_dedup_mark, by_entry, block, 0, st, (const uint8_t *)flag, T, counts);
  hipLaunchKernelGGL(k_dedup_offsets, dim3(1), block, 0, st, (const u32 *)counts, (long)by_entry.x, offsets, (long long *)nullptr);
  hipLaunchKernelGGL(k_dedup_emit, by_entry, block, 0, st, (const uint8_t *)flag, T, (const long long *)offsets, heads);
  hipLaunchKernelGGL(k_dedup_assign, by_entry, block, 0, st, (const uint8_t *)flag, T, (long)S, (const long long *)offsets,
                     (const long long *)heads, (const long long *)order, (const long long *)res, (long long *)d_first, dup);
  // the first occurrences, in row order
  hipLaunchKernelGGL(k_dedup_mark, by_new, block, 0, st, (const uint8_t *)dup, (long)B, counts);
  hipLaunchKernelGGL(k_dedup_offsets, dim3(1), block, 0, st, (const u32 *)counts, (long)by_new.x, offsets, (long long *)d_count);
  if (d_unique)
    hipLaunchKernelGGL(k_dedup_emit, by_new, block, 0, st, (const uint8_t *)dup, (long)B, (const long long *)offsets, (long long *)d_unique);
  HIP_TRY(hipGetLastError());
  note_kernel(eng, d_unique ? "k_dedup_emit" : "k_dedup_offsets");
  return NTRU_OK;
}

int dedup_dev(ntru_engine *eng, const char *who, bool packed, int N, int mod, const void *d_prior, int64_t S, const void *d_rows, int64_t B,
              uint64_t salt, int fingerprint_bits, void *d_work, int64_t *d_first, int64_t *d_unique, int64_t *d_count) {
  int os, bits, per;
  if (int rc = check_dedup(who, packed, N, mod, d_prior, S, d_rows, B, fingerprint_bits, d_work, true, d_first, d_unique, d_count, &os, &bits,
                           &per))
    return rc;
  if (B > 0) {
    const size_t wb = carve_work(S + B).total;
    const struct { const void *p; size_t n; const char *what; } o[3] = {{d_first, (size_t)B * 8, "first"}, {d_unique, (size_t)B * 8, "unique"},
                                                                        {d_count, 8, "count"}};
    for (int a = 0; a < 3; a++)
      if (ntru_ranges_overlap(o[a].p, o[a].n, d_work, wb)) return fail(NTRU_ERR_ARG, std::string(who) + ": " + o[a].what + " overlaps work");
  }
  if (!eng) return fail(NTRU_ERR_ARG, "engine is NULL");
  HIP_TRY(hipSetDevice(eng->device));
  if (B == 0) {
    HIP_TRY(hipMemsetAsync(d_count, 0, 8, eng->stream));
    return NTRU_OK;
  }
  return dedup_flow(eng, packed, N, mod, os, bits, per, d_prior, S, d_rows, B, salt, fingerprint_bits, (char *)d_work, d_first, d_unique, d_count);
}

// The S + B rows, the workspace and the outputs live in eng->shared_dev for the call; the rows go up through the chunked pipeline, each
// chunk copied from its staging buffer to its place behind the others.
int dedup_host(ntru_engine *eng, const char *who, bool packed, int N, int mod, const void *prior, int64_t S, const void *rows, int64_t B,
               uint64_t salt, int fingerprint_bits, int64_t *first, int64_t *unique, int64_t *count) {
  int os, bits, per;
  if (int rc = check_dedup(who, packed, N, mod, prior, S, rows, B, fingerprint_bits, nullptr, false, first, unique, count, &os, &bits, &per))
    return rc;
  if (!eng) return fail(NTRU_ERR_ARG, "engine is NULL");
  count[0] = 0;
  if (B == 0) return NTRU_OK;
  HIP_TRY(hipSetDevice(eng->device));
  const size_t row_bytes = packed ? (size_t)os * 32 : (size_t)N * 2;
  Carve c;
  const size_t at_prior = c.take((size_t)S * row_bytes), at_rows = c.take((size_t)B * row_bytes),
               at_work = c.take(carve_work(S + B).total), at_first = c.take((size_t)B * 8), at_unique = c.take((size_t)B * 8), at_count = c.take(8);
  ResidentHold hold(eng, who, c.total);
  if (hold.rc) return hold.rc;
  char *d_prior = hold.p + at_prior, *d_rows = hold.p + at_rows;
  int64_t *d_first = first ? (int64_t *)(hold.p + at_first) : nullptr, *d_unique = unique ? (int64_t *)(hold.p + at_unique) : nullptr,
          *d_count = (int64_t *)(hold.p + at_count);
  const struct { const void *src; char *dst; int64_t n; } up[2] = {{prior, d_prior, S}, {rows, d_rows, B}};
  for (int a = 0; a < 2; a++) {
    if (up[a].n == 0) continue;
    Pipeline P(eng);
    const int ir = P.in(up[a].src, row_bytes);
    char *dst = up[a].dst;
    if (int rc = P.run(up[a].n, ntru_chunk_items(up[a].n), [&](int64_t o, int64_t n, void **d) -> int {
          HIP_TRY(hipMemcpyAsync(dst + (size_t)o * row_bytes, d[ir], (size_t)n * row_bytes, hipMemcpyDeviceToDevice, eng->stream));
          return NTRU_OK;
        }))
      return rc;
  }
  if (int rc = dedup_flow(eng, packed, N, mod, os, bits, per, S ? d_prior : nullptr, S, d_rows, B, salt, fingerprint_bits, hold.p + at_work, d_first,
                          d_unique, d_count))
    return rc;
  HIP_TRY(hipStreamSynchronize(eng->stream));
  HIP_TRY(hipMemcpy(count, d_count, 8, hipMemcpyDeviceToHost));
  if (first) HIP_TRY(hipMemcpy(first, d_first, (size_t)B * 8, hipMemcpyDeviceToHost));
  if (unique && count[0] > 0) HIP_TRY(hipMemcpy(unique, d_unique, (size_t)std::min<int64_t>(count[0], B) * 8, hipMemcpyDeviceToHost));
  return NTRU_OK;
}

}  // namespace

extern "C" int ntru_dedup_workspace_bytes(int N, int64_t total_rows, size_t *bytes) {
  const std::string name = "ntru_dedup_workspace_bytes";
  if (!bytes) return fail(NTRU_ERR_ARG, name + ": bytes is NULL");
  if (N < 2 || N > NTRU_MAX_N) return fail(NTRU_ERR_ARG, name + ": need 2 <= N <= " + std::to_string(NTRU_MAX_N) + ", got N = " + std::to_string(N));
  if (total_rows < 0 || total_rows > NTRU_DEDUP_MAX_ROWS)
    return fail(NTRU_ERR_ARG, name + ": need 0 <= total_rows <= NTRU_DEDUP_MAX_ROWS = " + std::to_string(NTRU_DEDUP_MAX_ROWS) + ", got " +
                                  std::to_string(total_rows));
  *bytes = carve_work(total_rows).total;
  return NTRU_OK;
}

extern "C" int ntru_dedup_rows_dev(ntru_engine_t *eng, int N, int mod, const uint16_t *d_prior, int64_t S, const uint16_t *d_rows, int64_t B,
                                   uint64_t salt, int fingerprint_bits, void *d_work, int64_t *d_first, int64_t *d_unique, int64_t *d_count) {
  return dedup_dev(eng, "ntru_dedup_rows", false, N, mod, d_prior, S, d_rows, B, salt, fingerprint_bits, d_work, d_first, d_unique, d_count);
}

extern "C" int ntru_dedup_packed_dev(ntru_engine_t *eng, int N, int mod, const uint64_t *d_prior, int64_t S, const uint64_t *d_packed, int64_t B,
                                     uint64_t salt, int fingerprint_bits, void *d_work, int64_t *d_first, int64_t *d_unique, int64_t *d_count) {
  return dedup_dev(eng, "ntru_dedup_packed", true, N, mod, d_prior, S, d_packed, B, salt, fingerprint_bits, d_work, d_first, d_unique, d_count);
}

extern "C" int ntru_dedup_rows(ntru_engine_t *eng, int N, int mod, const uint16_t *prior, int64_t S, const uint16_t *rows, int64_t B,
                               uint64_t salt, int fingerprint_bits, int64_t *first, int64_t *unique, int64_t *count) {
  return dedup_host(eng, "ntru_dedup_rows", false, N, mod, prior, S, rows, B, salt, fingerprint_bits, first, unique, count);
}

extern "C" int ntru_dedup_packed(ntru_engine_t *eng, int N, int mod, const uint64_t *prior, int64_t S, const uint64_t *packed, int64_t B,
                                 uint64_t salt, int fingerprint_bits, int64_t *first, int64_t *unique, int64_t *count) {
  return dedup_host(eng, "ntru_dedup_packed", true, N, mod, prior, S, packed, B, salt, fingerprint_bits, first, unique, count);
}
