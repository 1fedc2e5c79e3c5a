// ciphertext_sum.hip -- segmented, optionally weighted sums of ciphertext rows (the additive homomorphism of
// test/reference.test.js:46-61 folded over a whole group: addPolynomials, index.js:235-244, and multiplyPolynomialsByScalar) and
// the tally call that decrypts the sums: kernels, *_dev entry points and the host-pointer forms.
//
//   out[g][k] = (sum over the rows of group g of  w[row] * rows[row][k]) mod `mod`
//
// The work is bound by reading 2 N bytes per row once.  Decomposition (nothing of it depends on the group sizes, which the host
// never sees in the _dev form):
//   * the rows [first offset, last offset) are cut into Pb equal ROW BLOCKS, Pb from the grid (waves per CU x CUs / column tiles);
//     the kernel derives the block length from the offsets on the device;
//   * one wavefront owns (row block, column tile of 512 columns): lane l accumulates the 8 columns 512 t + 8 l .. + 7 of every row of
//     its block in registers, walking the groups that meet the block (a binary search finds the first);
//   * a group that lies inside one block is reduced and stored straight from the registers -- short groups never touch the split
//     machinery;
//   * a group that crosses a block boundary leaves one partial row per block it meets in scratch: slot 0 of a block for the group
//     that entered through the block's start, slot 1 for the group that leaves through its end (at most one each), and the block
//     records the group of slot 1.  k_sum_groups_finish then walks the Pb - 1 boundaries; where a group STARTS crossing, 32 x 32
//     threads add that group's partials in a fixed tree and store the row.
// Scratch is Pb x (2 N x 4 + 8) bytes: bounded by the grid and N, not by the batch.  Sums of integers do not depend on the order, so
// the result is independent of Pb, the grid and the kernel path.
//
// Rows have a pitch of 2 N bytes with N odd, so every other row starts on half a dword.  A 16-byte load from a 4-byte aligned
// address runs at the full rate and only sub-dword misalignment is slow (matrix_common.h), so a lane reads the ALIGNED 16 bytes at
// or just below its columns plus the following dword and shifts by 0 or 2 bytes (v_alignbyte; the shift is the same for the whole
// wave).  The only loads that could leave the array are those of the last row or two: they go element by element.
// Exactness: for a power-of-two modulus the u32 accumulators may wrap (2^32 is a multiple of mod); otherwise the accumulators are
// u64 (w x < 2^32, up to 2^31 rows) and partial rows are stored reduced.
#include <hip/hip_runtime.h>

#include <cstdint>
#include <cstdio>
#include <cstring>
#include <string>

#include "kernels_common.h"
#include "sum_groups_common.h"

namespace {

constexpr int SG_THREADS = 256;          // four independent waves
constexpr int SG_TILE = 512;             // columns per wave: 8 per lane
constexpr int SG_WAVES_PER_CU = 8;
constexpr int FIN_COLS = 32, FIN_SLICES = 32;   // k_sum_groups_finish: 1024 threads = 32 columns x 32 slices of the partial list
constexpr int FIN_Y = 32;

typedef u32 u32x3 __attribute__((ext_vector_type(3)));
typedef u32x3 u32x3_a4 __attribute__((aligned(4)));

// The 8 coefficients at p as u32, from load8_raw's five dwords (sum_groups_common.h): the pairs, split into halves.
__device__ __forceinline__ void split8(const u32 (&w)[4], u32 (&x)[8]) {
#pragma unroll
  for (int k = 0; k < 4; k++) {
    x[2 * k] = w[k] & 0xffffu;
    x[2 * k + 1] = w[k] >> 16;
  }
}
__device__ __forceinline__ void shift8(const u16 *p, const u32 (&d)[5], u32 (&x)[8]) {
  u32 w[4];
  pairs8(half_dword(p), d, w);
  split8(w, x);
}
// The same with every element checked against `lim`, the end of the array: the last rows only.
__device__ __forceinline__ void load8_checked(const u16 *p, const u16 *lim, u32 (&x)[8]) {
  u32 w[4];
  pairs8_checked(p, lim, w);
  split8(w, x);
}

template <bool POW2, bool WEIGHTED, class Acc>
__device__ __forceinline__ void accumulate(Acc (&acc)[8], const u32 (&x)[8], u32 w) {
#pragma unroll
  for (int k = 0; k < 8; k++) {
    if (!WEIGHTED) acc[k] += x[k];
    else if (POW2) acc[k] += (Acc)(x[k] * w);
    else acc[k] += (Acc)((u64)x[k] * w);
  }
}

// R consecutive rows from p on: every load is issued before the first sum needs one.
template <int R, bool POW2, bool WEIGHTED, class Acc>
__device__ __forceinline__ void row_batch(Acc (&acc)[8], const u16 *p, int N, const u16 *w) {
  u32 d[R][5];
#pragma unroll
  for (int j = 0; j < R; j++) load8_raw(p + j * (long)N, half_dword(p + j * (long)N), d[j]);
#pragma unroll
  for (int j = 0; j < R; j++) {
    u32 x[8];
    shift8(p + j * (long)N, d[j], x);
    accumulate<POW2, WEIGHTED>(acc, x, WEIGHTED ? (u32)w[j] : 1u);
  }
}

// Stores the nv <= 8 coefficients v at p (2-byte aligned): whole lanes as one 16-byte store from a 4-byte aligned address, or, half a
// dword off, as 2 + 12 + 2 bytes.
__device__ __forceinline__ void store8(u16 *p, const u32 (&v)[8], int nv) {
  if (nv >= 8) {
    if ((((uintptr_t)p >> 1) & 1u) == 0) {
      u32x4 o;
#pragma unroll
      for (int k = 0; k < 4; k++) o[k] = v[2 * k] | (v[2 * k + 1] << 16);
      *(u32x4_a4 *)p = o;
    } else {
      u32x3 o;
#pragma unroll
      for (int k = 0; k < 3; k++) o[k] = v[2 * k + 1] | (v[2 * k + 2] << 16);
      p[0] = (u16)v[0];
      *(u32x3_a4 *)(p + 1) = o;
      p[7] = (u16)v[7];
    }
  } else {
#pragma unroll
    for (int k = 0; k < 8; k++)
      if (k < nv) p[k] = (u16)v[k];
  }
}

template <bool POW2, bool WEIGHTED>
__global__ void __launch_bounds__(SG_THREADS) k_sum_groups(int N, u32 mod, Groups gr, const u16 *__restrict__ rows,
                                                           const u16 *__restrict__ wts, int NT, long Pb, u32 *__restrict__ part,
                                                           long *__restrict__ meta, u16 *__restrict__ out) {
  typedef typename std::conditional<POW2, u32, u64>::type Acc;
  const int lane = threadIdx.x & 63;
  const long wave = (long)blockIdx.x * (SG_THREADS / 64) + (threadIdx.x >> 6);
  const int tile = (int)(wave % NT);
  const long b = wave / NT;
  if (b >= Pb) return;
  const Cut cut = cut_of(gr, Pb);
  if (b >= cut.nb) return;
  const long r0 = cut.base + b * cut.R;
  const long r1 = r0 + cut.R < cut.end ? r0 + cut.R : cut.end;
  const bool last = r1 == cut.end;
  const int c0 = tile * SG_TILE + 8 * lane;
  const int nv = N - c0 < 8 ? N - c0 : 8;                        // this lane's columns: c0 .. c0 + nv - 1
  const u16 *lim = rows + (cut.end - gr.wlo) * N;
  // first group that meets the block: the first one that starts at or behind r0, or the one before it when that reaches into the block
  long g = 0;
  {
    long lo = 0, hi = gr.G;
    while (lo < hi) {
      const long mid = (lo + hi) >> 1;
      if (g_start(gr, mid) < r0) lo = mid + 1; else hi = mid;
    }
    g = lo;
    if (g > 0 && g_start(gr, g) > r0) g--;
  }
  long tail_g = -1;
  for (; g < gr.G; g++) {
    const long s = g_start(gr, g);
    if (s >= r1 && !last) break;
    const long e = g_start(gr, g + 1);
    const long a = s > r0 ? s : r0, z = e < r1 ? e : r1;
    Acc acc[8];
#pragma unroll
    for (int k = 0; k < 8; k++) acc[k] = 0;
    if (nv > 0) {
      long r = a;
      const u16 *p = rows + (r - gr.wlo) * N + c0;
      // rows whose loads stay inside the array for EVERY lane of the tile (the same for the whole wave): all but the last one or two
      const long room = (lim - rows) - (long)tile * SG_TILE - 8 * 63 - 10;   // elements between the array's end and lane 63's window of row wlo
      const long safe = room < 0 ? gr.wlo : room / N + gr.wlo + 1;
      const long zf = z < safe ? z : safe;
      for (; r + 8 <= zf; r += 8, p += 8 * (long)N) row_batch<8, POW2, WEIGHTED>(acc, p, N, WEIGHTED ? wts + (r - gr.wlo) : nullptr);
      for (; r + 4 <= zf; r += 4, p += 4 * (long)N) row_batch<4, POW2, WEIGHTED>(acc, p, N, WEIGHTED ? wts + (r - gr.wlo) : nullptr);
      for (; r < zf; r++, p += N) row_batch<1, POW2, WEIGHTED>(acc, p, N, WEIGHTED ? wts + (r - gr.wlo) : nullptr);
      for (; r < z; r++, p += N) {
        u32 x[8];
        load8_checked(p, lim, x);
        accumulate<POW2, WEIGHTED>(acc, x, WEIGHTED ? (u32)wts[r - gr.wlo] : 1u);
      }
    }
    u32 v[8];
#pragma unroll
    for (int k = 0; k < 8; k++) v[k] = POW2 ? (u32)acc[k] & (mod - 1) : mod_u64((u64)acc[k], mod);
    if (s >= r0 && e <= r1) {
      if (nv > 0) store8(out + g * N + c0, v, nv);
    } else {
      const int slot = s < r0 ? 0 : 1;
      if (slot) tail_g = g;
      u32 *q = part + (b * 2 + slot) * N + c0;
#pragma unroll
      for (int k = 0; k < 8; k++)
        if (k < nv) q[k] = v[k];
    }
  }
  if (tile == 0 && lane == 0) meta[b] = tail_g;
}

// Boundary j lies between the blocks j - 1 and j.  The group of slot 1 of block j - 1 starts crossing there: its partials are that
// slot and slot 0 of the blocks j .. (the block of its last row).
template <bool POW2>
__global__ void __launch_bounds__(FIN_COLS * FIN_SLICES) k_sum_groups_finish(int N, u32 mod, Groups gr, long Pb,
                                                                              const u32 *__restrict__ part,
                                                                              const long *__restrict__ meta, u16 *__restrict__ out) {
  __shared__ long s_meta[FIN_COLS * FIN_SLICES];
  __shared__ u32 s_acc[FIN_SLICES][FIN_COLS];
  const Cut cut = cut_of(gr, Pb);
  const int tid = threadIdx.x, col = tid & (FIN_COLS - 1), sl = tid / FIN_COLS;
  const int c = blockIdx.x * FIN_COLS + col;
  // the boundaries of this workgroup: j = 1 + blockIdx.y + i gridDim.y < nb; one load each, all in flight together
  const long first = 1 + blockIdx.y;
  const long n_it = cut.nb > first ? (cut.nb - first + gridDim.y - 1) / gridDim.y : 0;
  for (long i0 = 0; i0 < n_it; i0 += FIN_COLS * FIN_SLICES) {
    __syncthreads();
    if (i0 + tid < n_it) s_meta[tid] = meta[first + (i0 + tid) * gridDim.y - 1];
    __syncthreads();
    const long cnt = n_it - i0 < FIN_COLS * FIN_SLICES ? n_it - i0 : FIN_COLS * FIN_SLICES;
    for (long i = 0; i < cnt; i++) {
      const long g = s_meta[i];
      if (g < 0) continue;                                        // (the same for the whole workgroup)
      const long j = first + (i0 + i) * gridDim.y;
      const long b1 = (g_start(gr, g + 1) - 1 - cut.base) / cut.R;
      u32 acc = 0;
      if (c < N) {
        if (sl == 0) acc = part[((j - 1) * 2 + 1) * N + c];
        for (long bb = j + sl; bb <= b1; bb += FIN_SLICES) acc += part[(bb * 2) * N + c];
      }
      s_acc[sl][col] = acc;
      __syncthreads();
      if (sl == 0 && c < N) {
        u32 t = 0;
#pragma unroll 8
        for (int k = 0; k < FIN_SLICES; k++) t += s_acc[k][col];
        out[g * N + c] = (u16)(POW2 ? t & (mod - 1) : t % mod);   // not a power of two: partials < mod <= 65535, at most 2^15 of them
      }
      __syncthreads();
    }
  }
}

// ---- host side --------------------------------------------------------------------------------------------------------------------

}  // namespace

int ntru_check_sum_args(const ntru_engine *eng, int N, int mod, bool uniform, int64_t K, int64_t G, const char *who) {
  if (int rc = ntru_check_ring_mod(std::string(who) + ": ", N, mod)) return rc;
  if (G < 0) return fail(NTRU_ERR_ARG, std::string(who) + ": negative group count");
  if (uniform && K < 1) return fail(NTRU_ERR_ARG, std::string(who) + ": uniform groups need K >= 1, got " + std::to_string(K));
  if (uniform && G > 0 && K > (int64_t)0x7fffffffffffLL / G) return fail(NTRU_ERR_ARG, std::string(who) + ": G * K is out of range");
  if (!eng) return fail(NTRU_ERR_ARG, "engine is NULL");
  return NTRU_OK;
}

namespace {

// Enqueues the sums of the groups `w` of the dense rows at d_rows (row w.wlo first) into d_out (group 0 of w first).
int launch_sum(ntru_engine *eng, int N, int mod, const void *d_rows, const uint16_t *d_weights, const SumWindow &w, uint16_t *d_out) {
  const bool pow2 = is_pow2(mod);
  auto enqueue = [&](dim3 grid, const Groups &gr, int NT, long Pb, u32 *part, long *meta) {
    sum_variant(pow2, d_weights != nullptr, [&](auto p2, auto wt) {
      hipLaunchKernelGGL((k_sum_groups<decltype(p2)::value, decltype(wt)::value>), grid, dim3(SG_THREADS), 0, eng->stream, N, (u32)mod, gr,
                         (const u16 *)d_rows, d_weights, NT, Pb, part, meta, d_out);
    });
  };
  if (int rc = launch_sum_rows(eng, N, mod, w, (N + SG_TILE - 1) / SG_TILE, SG_WAVES_PER_CU, SG_THREADS, d_out, enqueue)) return rc;
  note_kernel(eng, "k_sum_groups", (int)pow2, d_weights ? 1 : 0);
  return NTRU_OK;
}

}  // namespace

// (behind launch_sum: the kernels keep the order in the code object that they had)
int ntru_launch_sum_finish(ntru_engine *eng, int N, int mod, const SumWindow &w, long Pb, const uint32_t *d_part, const long *d_meta,
                           uint16_t *d_out) {
  if (Pb <= 1) return NTRU_OK;
  const Groups gr = groups_of(w);
  const dim3 fgrid((unsigned)((N + FIN_COLS - 1) / FIN_COLS), (unsigned)std::min<long>(FIN_Y, Pb - 1));
  if (is_pow2(mod))
    hipLaunchKernelGGL(k_sum_groups_finish<true>, fgrid, dim3(FIN_COLS * FIN_SLICES), 0, eng->stream, N, (u32)mod, gr, Pb, d_part, d_meta,
                       d_out);
  else
    hipLaunchKernelGGL(k_sum_groups_finish<false>, fgrid, dim3(FIN_COLS * FIN_SLICES), 0, eng->stream, N, (u32)mod, gr, Pb, d_part, d_meta,
                       d_out);
  HIP_TRY(hipGetLastError());
  return NTRU_OK;
}

extern "C" int ntru_sum_groups_dev(ntru_engine_t *eng, int N, int mod, const uint16_t *d_rows, const uint16_t *d_weights,
                                   const int64_t *d_offsets, int64_t K, int64_t G, uint16_t *d_out) {
  if (int rc = ntru_check_sum_args(eng, N, mod, !d_offsets, K, G, "ntru_sum_groups")) return rc;
  if (G == 0) return NTRU_OK;
  if (!d_rows || !d_out) return fail(NTRU_ERR_ARG, "ntru_sum_groups: NULL buffer");
  const SumWindow w = {d_offsets, d_offsets ? 0 : K, 0, G, 0, 0x7fffffffffffffffL};
  return launch_sum(eng, N, mod, d_rows, d_weights, w, d_out);
}

extern "C" int ntru_tally_decrypt_batch_dev(ntru_engine_t *eng, int N, int q, int p, const int8_t *d_f, const uint8_t *d_fp,
                                            const uint16_t *d_rows, const uint16_t *d_weights, const int64_t *d_offsets, int64_t K,
                                            int64_t G, uint16_t *d_sum, uint8_t *d_value, uint16_t *d_quot1, uint16_t *d_rem1,
                                            uint8_t *d_quot2) {
  return tally_decrypt(
      eng, "ntru_tally_decrypt_batch", N, q, p, !d_offsets, K, G, d_f && d_fp && d_rows && d_sum && d_value, "d_sum",
      [&] { return ntru_sum_groups_dev(eng, N, q, d_rows, d_weights, d_offsets, K, G, d_sum); },
      [&] { return ntru_decrypt_batch_dev(eng, N, q, p, d_f, d_fp, d_sum, G, d_value, d_quot1, d_rem1, d_quot2); });
}

// ---- host-pointer forms -------------------------------------------------------------------------------------------------------------
// The rows flow through the chunked pipeline; the sums [G][N] and the offsets stay on the device for the whole call (eng->shared_dev).
// A chunk is a window of rows: the groups that lie inside it are stored, the group that reaches into it from the chunk before is summed
// on its own and added to what is already there (ntru_add_batch_dev), the group that leaves it stores its part for the next chunk.

int ntru_sum_groups_host(ntru_engine *eng, const char *who, int N, int mod, const void *rows, size_t row_bytes, const uint16_t *weights,
                         const int64_t *offsets, int64_t K, int64_t G, uint16_t *out, ntru_sum_launcher launch_sum) {
  if (int rc = ntru_check_sum_args(eng, N, mod, !offsets, K, G, who)) return rc;
  if (G == 0) return NTRU_OK;
  const std::string name(who);
  if (!out) return fail(NTRU_ERR_ARG, name + ": NULL buffer");
  if (offsets) {
    if (offsets[0] < 0) return fail(NTRU_ERR_ARG, name + ": offsets[0] is negative");
    for (int64_t g = 0; g < G; g++)
      if (offsets[g + 1] < offsets[g]) return fail(NTRU_ERR_ARG, name + ": offsets decrease at group " + std::to_string(g));
  }
  const int64_t lo = offsets ? offsets[0] : 0, hi = offsets ? offsets[G] : G * K, B = hi - lo;
  if (B > 0 && !rows) return fail(NTRU_ERR_ARG, name + ": NULL buffer");
  for (int64_t r = 0; weights && r < B; r++)
    if (weights[lo + r] >= mod) return fail(NTRU_ERR_ARG, name + ": weight of row " + std::to_string(lo + r) + " is not below mod");
  const size_t out_row = (size_t)N * 2, out_bytes = (size_t)G * out_row;
  if (B == 0) { memset(out, 0, out_bytes); return NTRU_OK; }
  HIP_TRY(hipSetDevice(eng->device));
  Carve c;
  const size_t out_at = c.take(out_bytes), off_at = c.take(offsets ? (size_t)(G + 1) * 8 : 0), tmp_at = c.total;
  ResidentHold hold(eng, who, tmp_at + out_row);                         // (the last array, one row, is not rounded up)
  if (hold.rc) return hold.rc;
  char *dev = hold.p;
  uint16_t *d_out = (uint16_t *)(dev + out_at), *d_tmp = (uint16_t *)(dev + tmp_at);
  const int64_t *d_off = offsets ? (const int64_t *)(dev + off_at) : nullptr;
  HIP_TRY(hipMemset(d_out, 0, out_bytes));                               // empty groups; every other row is stored by some chunk
  if (offsets) HIP_TRY(hipMemcpy(dev + off_at, offsets, (size_t)(G + 1) * 8, hipMemcpyHostToDevice));
  HIP_TRY(hipDeviceSynchronize());
  auto start_of = [&](int64_t g) { return offsets ? offsets[g] : g * K; };
  Pipeline P(eng);
  const int ir = P.in((const char *)rows + (size_t)lo * row_bytes, row_bytes), iw = weights ? P.in(weights + lo, 2) : -1;
  int rc = P.run(B, ntru_chunk_items(B), [&](int64_t o, int64_t n, void **d) {
    const int64_t a = lo + o, b = a + n;
    // first group that ends behind a, last group that starts before b: both hold rows of the window
    int64_t x = 0, y = G - 1;
    while (x < y) { const int64_t m = (x + y) >> 1; if (start_of(m + 1) > a) y = m; else x = m + 1; }
    const int64_t g_first = x;
    x = 0; y = G - 1;
    while (x < y) { const int64_t m = (x + y + 1) >> 1; if (start_of(m) < b) x = m; else y = m - 1; }
    const int64_t g_last = x;
    SumWindow gr;
    gr.off = d_off; gr.K = K; gr.wlo = a; gr.whi = b;
    const void *dr = d[ir];
    const uint16_t *dw = iw >= 0 ? (const uint16_t *)d[iw] : nullptr;
    int64_t g0 = g_first;
    if (start_of(g_first) < a) {                                         // reaches in from the chunk before: add to its part
      gr.g0 = g_first; gr.G = 1;
      if (gr.off) gr.off = d_off + g_first;
      if (int rc2 = accumulate_chunk(eng, N, mod, false, 1, d_out + g_first * N, d_tmp,
                                     [&](uint16_t *dst) { return launch_sum(eng, N, mod, dr, dw, gr, dst); }))
        return rc2;
      g0 = g_first + 1;
    }
    if (g0 > g_last) return (int)NTRU_OK;
    gr.g0 = g0; gr.G = g_last - g0 + 1;
    gr.off = d_off ? d_off + g0 : nullptr;
    return launch_sum(eng, N, mod, dr, dw, gr, d_out + g0 * N);
  });
  if (rc) return rc;
  HIP_TRY(hipMemcpy(out, d_out, out_bytes, hipMemcpyDeviceToHost));
  return NTRU_OK;
}

extern "C" int ntru_sum_groups(ntru_engine_t *eng, int N, int mod, const uint16_t *rows, const uint16_t *weights,
                               const int64_t *offsets, int64_t K, int64_t G, uint16_t *out) {
  return ntru_sum_groups_host(eng, "ntru_sum_groups", N, mod, rows, (size_t)N * 2, weights, offsets, K, G, out, launch_sum);
}

extern "C" int ntru_tally_decrypt_batch(ntru_engine_t *eng, int N, int q, int p, const int8_t *f, const uint8_t *fp,
                                        const uint16_t *rows, const uint16_t *weights, const int64_t *offsets, int64_t K, int64_t G,
                                        uint16_t *sum, uint8_t *value, uint16_t *quot1, uint16_t *rem1, uint8_t *quot2) {
  return tally_decrypt(                                  // (rows is tested by ntru_sum_groups_host, once it knows that there are rows)
      eng, "ntru_tally_decrypt_batch", N, q, p, !offsets, K, G, f && fp && sum && value, "sum",
      [&] { return ntru_sum_groups(eng, N, q, rows, weights, offsets, K, G, sum); },
      [&] { return ntru_decrypt_batch(eng, N, q, p, f, fp, sum, G, value, quot1, rem1, quot2); });
}
