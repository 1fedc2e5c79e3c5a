// permutation.hip -- MI355X (gfx950): the order of a mix step drawn on the device, and a whole mix step from a key (include/ntru_engine.h
// "drawing the mix order").  Kernels, *_dev entry points and the host-pointer forms.
//
//   k_perm_keys     the sort keys: one lane computes one ChaCha20 block (RFC 8439, always 20 rounds) = the eight 64-bit keys of items
//                   8 c .. 8 c + 7 under block counter c and nonce (perm_id_lo, perm_id_hi, "PERM"); the wave's 512 keys go through
//                   the LDS so that every store is 64 consecutive keys.
//   the sort        a stable least-significant-digit radix sort of (key, 32-bit index) pairs, eight passes of one byte.  Per pass:
//     k_perm_hist     one workgroup per tile of PT_TILE keys: the tile's digit histogram (LDS counters) -> hist[tile][digit];
//     k_perm_offsets  one workgroup per digit: the exclusive prefix of that digit's counts over the tiles, PT_THREADS tiles per round
//                     of a loop with a carry, written in place, and the digit's total;
//     k_perm_scatter  one workgroup per tile: the exclusive prefix of the 256 totals (the digit's base) + the tile's offset + the
//                     rank of the key among the tile's keys of the same digit, in key order: PT_ROUNDS rounds of 256 consecutive
//                     keys; inside a round a wave matches equal digits with one ballot per digit bit, mbcnt counts the lanes below,
//                     the first lane of every group leaves the group's size in a per-wave digit table in the LDS and the waves
//                     before add up; after the round lane d advances digit d's base by the round's count.
//                   Pass 0 reads the caller's keys with the position as the index; the last pass writes indices only.
//   k_perm_finish   widens the sorted indices to int64_t src and writes dst[src[j]] = j when asked.
// Positions come from prefix sums only: no global atomic, hence a stable order and the same bytes whatever the launch shape.  Every
// dependency between workgroups is a kernel boundary: no workgroup waits for another.  The only size boundaries are the tile
// (PT_TILE keys) and the round of k_perm_offsets' loop (PT_THREADS tiles = 2^18 keys).
#include <hip/hip_runtime.h>

#include <cstdint>
#include <cstdio>
#include <cstring>
#include <string>
#include <vector>

#include "sampler_common.h"

typedef unsigned long long u64;

constexpr int PT_THREADS = 256;                    // lanes per workgroup of every kernel here
constexpr int PT_WAVES = PT_THREADS / 64;
constexpr int PT_ROUNDS = 4;                       // rounds of PT_THREADS consecutive keys per tile
constexpr int PT_TILE = PT_THREADS * PT_ROUNDS;    // keys per tile
constexpr int PT_DIGITS = 256;                     // one byte per pass
constexpr int PT_PASSES = 8;
static_assert(PT_DIGITS == PT_THREADS, "lane d owns digit d");
static_assert((long)PT_TILE * PT_THREADS <= (1L << 18), "every size boundary lies at or below 2^18 keys");
static_assert(NTRU_PERM_MAX_B <= (1LL << 32), "positions and indices are 32-bit");

// keys[i] for i in [0, n): lane t of the grid computes block t.
__global__ void __launch_bounds__(PT_THREADS) k_perm_keys(ChaChaKey key, u32 id_lo, u32 id_hi, long n, u64 *__restrict__ keys) {
  __shared__ u64 s_keys[PT_WAVES][64 * 8 + 64];     // a lane's eight keys at 9 l .. 9 l + 7: odd pitch against bank conflicts
  const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
  const long wave_first = ((long)blockIdx.x * PT_THREADS + w * 64) * 8;      // the first key of this wave
  if (wave_first >= n) return;                      // uniform per wave; no workgroup barrier below
  const u32 ctr = (u32)(wave_first / 8) + lane;
  u32 ks[16];
  chacha_block<10>(key, ctr, id_lo, id_hi, NTRU_PERM_NONCE2, ks);
#pragma unroll
  for (int j = 0; j < 8; j++) s_keys[w][9 * lane + j] = (u64)ks[2 * j] | ((u64)ks[2 * j + 1] << 32);
  wave_lds_fence();
#pragma unroll
  for (int s = 0; s < 8; s++) {
    const int k = 64 * s + lane;                    // the wave's k-th key: key k & 7 of lane k >> 3
    const long i = wave_first + k;
    if (i < n) keys[i] = s_keys[w][9 * (k >> 3) + (k & 7)];
  }
}

static __device__ __forceinline__ u32 digit_of(u64 key, int shift) { return (u32)(key >> shift) & (PT_DIGITS - 1); }

// hist[tile][d] = the keys of the tile whose digit is d.
__global__ void __launch_bounds__(PT_THREADS) k_perm_hist(const u64 *__restrict__ keys, long n, int shift, u32 *__restrict__ hist) {
  __shared__ u32 s_hist[PT_DIGITS];
  const int tid = threadIdx.x;
  const long first = (long)blockIdx.x * PT_TILE;
  s_hist[tid] = 0;
  __syncthreads();
#pragma unroll
  for (int r = 0; r < PT_ROUNDS; r++) {
    const long i = first + r * PT_THREADS + tid;
    if (i < n) atomicAdd(&s_hist[digit_of(keys[i], shift)], 1u);          // LDS counters: the sum does not depend on the order
  }
  __syncthreads();
  hist[(long)blockIdx.x * PT_DIGITS + tid] = s_hist[tid];
}

// Workgroup d: hist[t][d] <- sum of hist[0 .. t - 1][d] for every tile t, total[d] <- the sum over all tiles.
__global__ void __launch_bounds__(PT_THREADS) k_perm_offsets(u32 *hist, int tiles, u32 *__restrict__ total) {
  __shared__ u32 s_sum[PT_THREADS];
  const int tid = threadIdx.x, d = blockIdx.x;
  u32 carry = 0;
  for (int t0 = 0; t0 < tiles; t0 += PT_THREADS) {                          // uniform loop
    const int t = t0 + tid;
    const u32 c = t < tiles ? hist[(long)t * PT_DIGITS + d] : 0u;
    s_sum[tid] = c;
    __syncthreads();
    wg_inclusive_scan<PT_THREADS>(s_sum, tid);
    if (t < tiles) hist[(long)t * PT_DIGITS + d] = carry + s_sum[tid] - c;
    carry += s_sum[PT_THREADS - 1];
    __syncthreads();                                                         // every lane has read the round's total
  }
  if (tid == 0) total[d] = carry;
}

// offs = hist after k_perm_offsets.  idx_in == NULL: the index of key i is i.  keys_out == NULL: indices only.
__global__ void __launch_bounds__(PT_THREADS) k_perm_scatter(const u64 *__restrict__ keys_in, const u32 *__restrict__ idx_in, long n,
                                                            int shift, const u32 *__restrict__ offs, const u32 *__restrict__ total,
                                                            u64 *__restrict__ keys_out, u32 *__restrict__ idx_out) {
  __shared__ u32 s_base[PT_DIGITS];                 // where the tile's next key of digit d goes
  __shared__ u32 s_wave[PT_WAVES][PT_DIGITS];       // this round's keys of digit d in wave w
  const int tid = threadIdx.x, w = tid >> 6;
  const long first = (long)blockIdx.x * PT_TILE;
  const u32 tot = total[tid];
  s_base[tid] = tot;
  __syncthreads();
  wg_inclusive_scan<PT_DIGITS>(s_base, tid);        // inclusive prefix of the totals
  s_base[tid] += offs[(long)blockIdx.x * PT_DIGITS + tid] - tot;
#pragma unroll
  for (int v = 0; v < PT_WAVES; v++) s_wave[v][tid] = 0;
  __syncthreads();
  for (int r = 0; r < PT_ROUNDS; r++) {             // uniform loop: barriers inside
    const long i = first + r * PT_THREADS + tid;
    const bool valid = i < n;
    const u64 key = valid ? keys_in[i] : 0ull;
    const u32 idx = valid ? (idx_in ? idx_in[i] : (u32)i) : 0u;
    const u32 d = digit_of(key, shift);
    u64 same = __ballot(valid);                     // the valid lanes of this wave with this lane's digit
#pragma unroll
    for (int b = 0; b < 8; b++) {
      const bool bit = (d >> b) & 1u;
      const u64 bal = __ballot(bit);
      same &= bit ? bal : ~bal;
    }
    const u32 below = lanes_below(same);
    if (valid && below == 0) s_wave[w][d] = (u32)__popcll(same);
    __syncthreads();
    u32 pos = s_base[d] + below;
#pragma unroll
    for (int v = 0; v < PT_WAVES; v++)
      if (v < w) pos += s_wave[v][d];
    __syncthreads();                                // every lane has its position: lane d may now advance digit d
    u32 c = 0;
#pragma unroll
    for (int v = 0; v < PT_WAVES; v++) {
      c += s_wave[v][tid];
      s_wave[v][tid] = 0;
    }
    s_base[tid] += c;
    if (valid && pos < (u32)n) {                    // (pos < n always holds for offsets that k_perm_hist / k_perm_offsets made)
      if (keys_out) keys_out[pos] = key;
      idx_out[pos] = idx;
    }
    __syncthreads();
  }
}

__global__ void __launch_bounds__(PT_THREADS) k_perm_finish(const u32 *__restrict__ idx, long n, long long *__restrict__ src,
                                                           long long *__restrict__ dst) {
  for (long j = (long)blockIdx.x * PT_THREADS + threadIdx.x; j < n; j += (long)gridDim.x * PT_THREADS) {
    const u32 s = idx[j];
    if (src) src[j] = (long long)s;
    if (dst && s < (u32)n) dst[s] = (long long)j;
  }
}

namespace {

// Enqueues on eng->stream: the keys (d_keys, or drawn under ck / perm_id when d_keys is NULL), the sort, the finish.  The scratch
// buffer is held until the last kernel is enqueued and released on return.
int perm_flow(ntru_engine *eng, const uint64_t *d_keys, const ChaChaKey *ck, uint64_t perm_id, int64_t B, int64_t *d_src, int64_t *d_dst) {
  HIP_TRY(hipSetDevice(eng->device));
  const int tiles = (int)((B + PT_TILE - 1) / PT_TILE);
  Carve c;
  const size_t at_k0 = c.take((size_t)B * 8), at_k1 = c.take((size_t)B * 8), at_i0 = c.take((size_t)B * 4), at_i1 = c.take((size_t)B * 4),
               at_hist = c.take((size_t)tiles * PT_DIGITS * 4), at_total = c.take(PT_DIGITS * 4);
  ScratchHold hold(eng, c.total);
  if (hold.rc) return hold.rc;
  u64 *kbuf[2] = {(u64 *)(hold.p + at_k0), (u64 *)(hold.p + at_k1)};
  u32 *ibuf[2] = {(u32 *)(hold.p + at_i0), (u32 *)(hold.p + at_i1)};
  u32 *d_hist = (u32 *)(hold.p + at_hist), *d_total = (u32 *)(hold.p + at_total);
  const u64 *in_keys = (const u64 *)d_keys;
  if (!in_keys) {                                   // drawn into the pair that pass 0 does not write
    const long blocks = (B + 7) / 8;
    hipLaunchKernelGGL(k_perm_keys, dim3((unsigned)((blocks + PT_THREADS - 1) / PT_THREADS)), dim3(PT_THREADS), 0, eng->stream, *ck,
                       (u32)perm_id, (u32)(perm_id >> 32), (long)B, kbuf[1]);
    in_keys = kbuf[1];
  }
  const u32 *in_idx = nullptr;
  for (int pass = 0; pass < PT_PASSES; pass++) {
    const int o = pass & 1;                         // pass 0 writes pair 0, pass 1 pair 1, ...
    u64 *out_keys = pass == PT_PASSES - 1 ? nullptr : kbuf[o];
    hipLaunchKernelGGL(k_perm_hist, dim3(tiles), dim3(PT_THREADS), 0, eng->stream, in_keys, (long)B, 8 * pass, d_hist);
    hipLaunchKernelGGL(k_perm_offsets, dim3(PT_DIGITS), dim3(PT_THREADS), 0, eng->stream, d_hist, tiles, d_total);
    hipLaunchKernelGGL(k_perm_scatter, dim3(tiles), dim3(PT_THREADS), 0, eng->stream, in_keys, in_idx, (long)B, 8 * pass,
                       (const u32 *)d_hist, (const u32 *)d_total, out_keys, ibuf[o]);
    in_keys = kbuf[o];
    in_idx = ibuf[o];
  }
  const long fblocks = (B + PT_THREADS - 1) / PT_THREADS, cap = (long)eng->cus * 8;
  hipLaunchKernelGGL(k_perm_finish, dim3((unsigned)(fblocks < cap ? fblocks : cap)), dim3(PT_THREADS), 0, eng->stream, in_idx, (long)B,
                     (long long *)d_src, (long long *)d_dst);
  HIP_TRY(hipGetLastError());
  note_kernel(eng, "k_perm_finish");
  return NTRU_OK;
}

// The checks of the draw that need no engine.
int check_draw(const std::string &name, const uint32_t *key, int64_t B, const void *src, const void *dst) {
  if (B < 0) return fail(NTRU_ERR_ARG, name + ": negative batch size");
  if (B > NTRU_PERM_MAX_B) return fail(NTRU_ERR_ARG, name + ": need B <= NTRU_PERM_MAX_B = " + std::to_string(NTRU_PERM_MAX_B) + ", got " + std::to_string(B));
  if (!key) return fail(NTRU_ERR_ARG, name + ": key is NULL");
  if (B > 0 && !src && !dst) return fail(NTRU_ERR_ARG, name + ": src and dst are both NULL");
  if (ntru_ranges_overlap(src, (size_t)B * 8, dst, (size_t)B * 8)) return fail(NTRU_ERR_ARG, name + ": src and dst overlap");
  return NTRU_OK;
}

// The checks of a mix step that need no engine, then those of the calls it is made of (engine, (N, q), the sampler's counts).
int check_mix(ntru_engine *eng, const std::string &name, int N, int q, int p, const void *h, const uint32_t *key, uint64_t first_item, int n1,
              int n2, const uint16_t *e_in, int64_t B, const void *r, const void *src, const uint16_t *e_out, const void *quotE, bool need_outputs) {
  if (B < 0) return fail(NTRU_ERR_ARG, name + ": negative batch size");
  if (B > NTRU_PERM_MAX_B) return fail(NTRU_ERR_ARG, name + ": need B <= NTRU_PERM_MAX_B = " + std::to_string(NTRU_PERM_MAX_B) + ", got " + std::to_string(B));
  if (!key) return fail(NTRU_ERR_ARG, name + ": key is NULL");
  if (p < 1 || p > 256) return fail(NTRU_ERR_ARG, name + ": need 1 <= p <= 256 (r holds p - 1 in a byte), got " + std::to_string(p));
  if (N < 1 || n1 < 0 || n2 < 0) return fail(NTRU_ERR_ARG, name + ": negative size");
  if (n1 + n2 > N) return fail(NTRU_ERR_ARG, name + ": The total of 1s and -1s cannot exceed the array length.");
  if (B > 0 && (!h || !e_in || !e_out || (need_outputs && (!r || !src)))) return fail(NTRU_ERR_ARG, name + ": NULL buffer");
  const size_t rows = (size_t)B * N * 2;
  if (ntru_ranges_overlap(e_in, rows, e_out, rows)) return fail(NTRU_ERR_ARG, name + ": e_in and e_out overlap");
  const struct { const void *p; size_t n; const char *what; } outs[4] = {
      {e_out, rows, "e_out"}, {quotE, rows, "quotE"}, {r, (size_t)B * N, "r"}, {src, (size_t)B * 8, "src"}};
  for (int a = 0; a < 4; a++)
    for (int b = a + 1; b < 4; b++)
      if (ntru_ranges_overlap(outs[a].p, outs[a].n, outs[b].p, outs[b].n))
        return fail(NTRU_ERR_ARG, name + ": " + outs[a].what + " and " + outs[b].what + " overlap");
  if (int rc = ntru_sample_ternary_dev(eng, N, n1, n2, p - 1, key, first_item, 0, nullptr)) return rc;
  return ntru_reencrypt_batch_dev(eng, N, q, nullptr, nullptr, nullptr, 0, nullptr, 0, nullptr, nullptr);
}

// The host form of the draw into host arrays (either may be NULL): the device arrays live in eng->shared_dev for the call.
int draw_to_host(ntru_engine *eng, const ChaChaKey &ck, uint64_t perm_id, int64_t B, int64_t *src, int64_t *dst) {
  HIP_TRY(hipSetDevice(eng->device));
  const size_t bytes = (size_t)B * 8;
  Carve c;
  const size_t at_src = c.take(bytes), at_dst = c.take(bytes);
  ResidentHold hold(eng, "ntru_draw_permutation", c.total);
  if (hold.rc) return hold.rc;
  int64_t *d_src = src ? (int64_t *)(hold.p + at_src) : nullptr;
  int64_t *d_dst = dst ? (int64_t *)(hold.p + at_dst) : nullptr;
  if (int rc = perm_flow(eng, nullptr, &ck, perm_id, B, d_src, d_dst)) return rc;
  HIP_TRY(hipStreamSynchronize(eng->stream));
  if (src) HIP_TRY(hipMemcpy(src, d_src, bytes, hipMemcpyDeviceToHost));
  if (dst) HIP_TRY(hipMemcpy(dst, d_dst, bytes, hipMemcpyDeviceToHost));
  return NTRU_OK;
}

}  // namespace

extern "C" int ntru_argsort_keys_dev(ntru_engine_t *eng, const uint64_t *d_keys, int64_t B, int64_t *d_order) {
  const std::string name = "ntru_argsort_keys";
  if (B < 0) return fail(NTRU_ERR_ARG, name + ": negative batch size");
  if (B > NTRU_PERM_MAX_B) return fail(NTRU_ERR_ARG, name + ": need B <= NTRU_PERM_MAX_B = " + std::to_string(NTRU_PERM_MAX_B) + ", got " + std::to_string(B));
  if (B > 0 && (!d_keys || !d_order)) return fail(NTRU_ERR_ARG, name + ": NULL buffer");
  if (ntru_ranges_overlap(d_keys, (size_t)B * 8, d_order, (size_t)B * 8)) return fail(NTRU_ERR_ARG, name + ": keys and order overlap");
  if (!eng) return fail(NTRU_ERR_ARG, "engine is NULL");
  if (B == 0) return NTRU_OK;
  return perm_flow(eng, d_keys, nullptr, 0, B, d_order, nullptr);
}

extern "C" int ntru_draw_permutation_dev(ntru_engine_t *eng, const uint32_t *key, uint64_t perm_id, int64_t B, int64_t *d_src,
                                         int64_t *d_dst) {
  if (int rc = check_draw("ntru_draw_permutation", key, B, d_src, d_dst)) return rc;
  if (!eng) return fail(NTRU_ERR_ARG, "engine is NULL");
  if (B == 0) return NTRU_OK;
  ChaChaKey ck;
  memcpy(ck.k, key, 32);
  return perm_flow(eng, nullptr, &ck, perm_id, B, d_src, d_dst);
}

extern "C" int ntru_draw_permutation(ntru_engine_t *eng, const uint32_t *key, uint64_t perm_id, int64_t B, int64_t *src, int64_t *dst) {
  if (int rc = check_draw("ntru_draw_permutation", key, B, src, dst)) return rc;
  if (!eng) return fail(NTRU_ERR_ARG, "engine is NULL");
  if (B == 0) return NTRU_OK;
  ChaChaKey ck;
  memcpy(ck.k, key, 32);
  return draw_to_host(eng, ck, perm_id, B, src, dst);
}

// The sort's temporaries are released (perm_flow has returned) before the re-encrypt takes the scratch buffer for itself; the stream
// orders the reuse.
extern "C" int ntru_mix_batch_dev(ntru_engine_t *eng, int N, int q, int p, const uint16_t *d_h, const uint32_t *key, uint64_t first_item,
                                  int n1, int n2, uint64_t perm_id, const uint16_t *d_e_in, int64_t B, uint8_t *d_r, int64_t *d_src,
                                  uint16_t *d_e_out, uint16_t *d_quotE) {
  if (int rc = check_mix(eng, "ntru_mix_batch", N, q, p, d_h, key, first_item, n1, n2, d_e_in, B, d_r, d_src, d_e_out, d_quotE, true)) return rc;
  if (B == 0) return NTRU_OK;
  if (int rc = ntru_sample_ternary_dev(eng, N, n1, n2, p - 1, key, first_item, B, d_r)) return rc;
  ChaChaKey ck;
  memcpy(ck.k, key, 32);
  if (int rc = perm_flow(eng, nullptr, &ck, perm_id, B, d_src, nullptr)) return rc;
  return ntru_reencrypt_batch_dev(eng, N, q, d_h, d_r, d_e_in, B, d_src, B, d_e_out, d_quotE);
}

extern "C" int ntru_mix_batch(ntru_engine_t *eng, int N, int q, int p, const uint16_t *h, const uint32_t *key, uint64_t first_item, int n1,
                              int n2, uint64_t perm_id, const uint16_t *e_in, int64_t B, uint8_t *r_out, int64_t *src_out, uint16_t *e_out,
                              uint16_t *quotE) {
  if (int rc = check_mix(eng, "ntru_mix_batch", N, q, p, h, key, first_item, n1, n2, e_in, B, r_out, src_out, e_out, quotE, false)) return rc;
  if (B == 0) return NTRU_OK;
  ChaChaKey ck;
  memcpy(ck.k, key, 32);
  std::vector<int64_t> own;
  if (!src_out) {
    own.resize((size_t)B);
    src_out = own.data();
  }
  if (int rc = draw_to_host(eng, ck, perm_id, B, src_out, nullptr)) return rc;
  const ReencryptDraw draw = {key, first_item, n1, n2, p - 1, r_out};
  return ntru_reencrypt_host(eng, N, q, h, nullptr, &draw, e_in, B, src_out, B, e_out, quotE);
}
