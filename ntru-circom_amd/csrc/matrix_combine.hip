// matrix_combine.hip -- G linear combinations of the same B ciphertext rows in one pass: the additive homomorphism of
// ciphertext_sum.hip (addPolynomials, index.js:235-244, over rows scaled as multiplyPolynomialsByScalar does) with a weight MATRIX
// in place of one weight per row: kernels, the *_dev entry point and the host-pointer form.
//
//   out[g][k] = (sum over b of weights[b][g] * rows[b][k]) mod `mod`          out = W^T [G][B] . rows [B][N]
//
// One integer matrix product whose contraction runs over the batch axis.  The output is tiny and B is large, so the rows are cut
// into Pb ROW BLOCKS (a multiple of 32 rows each and at least 64, Pb from the grid); a block leaves an int32 partial [G][N] in scratch and
// k_combine_finish adds the Pb partials in a fixed order.  With Pb == 1 the row kernel stores the final rows itself.  No atomics:
// integer sums do not depend on the order, so the bytes are the same whatever Pb, the grid, the chunking or the kernel.
//
// k_combine_m<digit planes, output tiles> (power-of-two modulus, kernel paths 0, 4, 5): v_mfma_i32_32x32x32_i8, exact.  A workgroup of
// four waves owns (row block, 256 columns, 32 or 64 outputs: one tile of 32 for G <= 32, which keeps two workgroups on a CU) and walks
// its rows 64 at a time, two matrix instructions deep.  Both operands are u16: each is split into two balanced int8 digit planes,
// x = lo + 256 hi with lo = the low byte read as int8 and hi = ((x + 128) >> 8) read as int8.  lo.lo goes into one accumulator,
// lo.hi + hi.lo into a second one that counts 256-fold; hi.hi carries 2^16 and vanishes modulo every modulus of the domain, and so does
// whatever wraps out of the int32 accumulators (2^32 is a multiple of mod).  mod <= 256 needs the lo plane only (256 hi vanishes as
// well): the number of planes follows from the modulus's bit count, the bytes do not change.
// A lane's fragment is 16 consecutive contraction indices (matrix_common.h), and the contraction index is the batch row, so both
// operands pass through an LDS transpose: a thread loads 8 columns of two quads of consecutive rows (coalesced 16-byte loads from
// 4-byte aligned addresses + v_alignbyte, sum_groups_common.h), takes the digits (v_perm_b32 gathers the bytes of four rows) and writes
// one dword = 4 batch bytes per column, quad and plane.  The images are [slot][80 bytes] (64 batch bytes + 16: an odd multiple of 16,
// so that a fragment is one conflict-free ds_read_b128); column 8 c + j of the 256 sits in slot 32 j + c, which makes the dword writes
// of a half-wave (8 values of c x 4 row quads) hit 32 different banks; matrix tile j therefore holds the columns = j (mod 8), which
// only the epilogue has to know.  The next step's global loads are issued before the current step's matrix instructions.  A step
// whose rows and 16-byte windows all lie inside the block and the array -- every step but the last one or two of a launch -- loads
// without a test per row; with the tests in the loop the kernel ran at a quarter of the rate (EXPERIMENTS.md).
//
// k_combine_v (any modulus; every modulus on kernel paths 1-3): one thread per column, the rows of a block, four outputs at a time;
// u32 accumulators for a power of two, u64 otherwise (w x < 2^32, up to 2^31 rows) with partials stored reduced.  The slow,
// obviously right path, and the second on-device implementation the tests compare with.
#include <hip/hip_runtime.h>

#include <cstdint>
#include <cstdio>
#include <cstring>
#include <string>

#include "matrix_common.h"
#include "sum_groups_common.h"

namespace {

constexpr int CB_THREADS = 256;
constexpr int CB_COLS = 256;                 // columns per workgroup (both kernels)
constexpr int CM_ROWS = 64;                  // batch rows per step of k_combine_m: two matrix instructions deep
constexpr int CM_PITCH = CM_ROWS + 16;       // bytes per image slot: an odd multiple of 16
constexpr int CV_WG_PER_CU = 8;
constexpr int CV_OUTS = 4;                   // outputs per thread of k_combine_v
constexpr long CB_MIN_ROWS = 64;             // rows per row block, at least; a block is a multiple of it
constexpr long CB_MAX_BLOCKS = SUM_MAX_ROW_BLOCKS;   // row blocks: k_combine_finish adds that many reduced partials in a u32
constexpr size_t CB_MAX_PART = (size_t)256 << 20;

// The 8 coefficients at p (2-byte aligned) as 4 dwords of two: the row read of sum_groups_common.h, raw and then pairs.  The caller has
// checked that p + 10 elements lie inside the array.
__device__ __forceinline__ void load8_pairs(const u16 *p, u32 (&x)[4]) {
  const u32 sh = half_dword(p);
  u32 d[5];
  load8_raw(p, sh, d);
  pairs8(sh, d, x);
}

// Byte 0 (even) and byte 2 (odd) of four dwords, each as one dword with a's byte first: the low bytes of two packed columns of four rows.
__device__ __forceinline__ void gather4(u32 a, u32 b, u32 c, u32 d, u32 &even, u32 &odd) {
  const u32 ab = __builtin_amdgcn_perm(b, a, 0x06020400u), cd = __builtin_amdgcn_perm(d, c, 0x06020400u);   // a0 b0 a2 b2 | c0 d0 c2 d2
  even = __builtin_amdgcn_perm(cd, ab, 0x05040100u);
  odd = __builtin_amdgcn_perm(cd, ab, 0x07060302u);
}
// the hi digits of two packed u16: ((x + 128) >> 8) per half; at most 256, so the halves do not meet, and the low byte of each is the digit
__device__ __forceinline__ u32 hi_digits(u32 w) { return ((w >> 8) & 0x00ff00ffu) + ((w >> 7) & 0x00010001u); }

// Work unit of a workgroup: (row block b, output group gg, column tile); rows [b R, min(B, (b + 1) R)).
struct Unit {
  int tile, gg;
  long r0, r1;
  long b;
};
__device__ __forceinline__ Unit unit_of(long B, long R, int NT, int GG) {
  Unit u;
  long id = blockIdx.x;
  u.tile = (int)(id % NT); id /= NT;
  u.gg = (int)(id % GG);
  u.b = id / GG;
  u.r0 = u.b * R;
  u.r1 = u.r0 + R < B ? u.r0 + R : B;
  return u;
}

// PLANES digit planes per operand, GT output tiles of 32 per workgroup.  part == nullptr: one row block, the final rows go to out.
template <int PLANES, int GT>
__global__ void __launch_bounds__(CB_THREADS) k_combine_m(int N, u32 mod, const u16 *__restrict__ rows, const u16 *__restrict__ wts,
                                                          long B, int G, long R, int NT, int GG, u32 *__restrict__ part,
                                                          u16 *__restrict__ out) {
  constexpr int ROW_IMG = CB_COLS * CM_PITCH, W_IMG = 32 * GT * CM_PITCH;   // bytes per digit plane
  __shared__ __attribute__((aligned(16))) unsigned char img[PLANES * (ROW_IMG + W_IMG)];
  unsigned char *const rimg = img, *const wimg = img + PLANES * ROW_IMG;
  const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
  const int c8 = (t & 7) + 8 * wave, bq = (t >> 3) & 7;      // loader: column octet 0 .. 31 (and outputs c8, c8 + 32), row quads bq, bq + 8
  const Unit u = unit_of(B, R, NT, GG);
  const int c0 = u.tile * CB_COLS + 8 * c8, g0 = u.gg * 32 * GT;
  const long total = B * N;
  const u16 *lim = rows + total;

  u32 xw[8][4], ww[GT][8];                                   // rows rb + 32 (i >> 2) + 4 bq + (i & 3), i < 8
  // A step whose 64 rows all belong to the block and whose loads stay inside the array for EVERY lane of the tile (the same for the
  // whole workgroup; all but the last step or two of a launch): no test per row, every load is issued before the first is needed.
  // Columns behind N read into the next row and are never stored; an output behind G reads a weight of its row and drops it.
  const long room = total - ((long)u.tile * CB_COLS + 8 * 31 + 10);                   // elements between lane 31's window of row 0 and the end
  const long safe_end = room < 0 ? 0 : room / N + 1;                                    // rows below it may be read by every lane
  const int wcol[2] = {g0 + c8 < G ? g0 + c8 : G - 1, g0 + c8 + 32 < G ? g0 + c8 + 32 : G - 1};
  const bool wlive[2] = {g0 + c8 < G, g0 + c8 + 32 < G};
  auto load_step = [&](long rb) {
    if (rb + CM_ROWS <= u.r1 && rb + CM_ROWS <= safe_end) {
      const u16 *p = rows + (rb + 4 * bq) * N + c0;
      const u16 *w = wts + (rb + 4 * bq) * G;
#pragma unroll
      for (int i = 0; i < 8; i++) {
        const long ro = 32 * (i >> 2) + (i & 3);
        load8_pairs(p + ro * N, xw[i]);
#pragma unroll
        for (int h = 0; h < GT; h++) ww[h][i] = wlive[h] ? (u32)w[ro * G + wcol[h]] : 0u;
      }
      return;
    }
#pragma unroll
    for (int i = 0; i < 8; i++) {
      const long row = rb + 32 * (i >> 2) + 4 * bq + (i & 3);
      if (row < u.r1 && c0 < N) {
        const long at = row * N + c0;
        if (at + 10 <= total) load8_pairs(rows + at, xw[i]);
        else pairs8_checked(rows + at, lim, xw[i]);
      } else {
#pragma unroll
        for (int k = 0; k < 4; k++) xw[i][k] = 0;
      }
#pragma unroll
      for (int h = 0; h < GT; h++) {
        const int g = g0 + c8 + 32 * h;
        ww[h][i] = row < u.r1 && g < G ? (u32)wts[row * G + g] : 0u;       // rows behind the block: zero digits
      }
    }
  };
  auto store_step = [&]() {
#pragma unroll
    for (int q = 0; q < 2; q++) {
#pragma unroll
      for (int k = 0; k < 4; k++) {
        unsigned char *even = rimg + ((2 * k) * 32 + c8) * CM_PITCH + 32 * q + 4 * bq, *odd = even + 32 * CM_PITCH;
        const u32 a = xw[4 * q][k], b = xw[4 * q + 1][k], c = xw[4 * q + 2][k], d = xw[4 * q + 3][k];
        gather4(a, b, c, d, *(u32 *)even, *(u32 *)odd);
        if (PLANES == 2) gather4(hi_digits(a), hi_digits(b), hi_digits(c), hi_digits(d), *(u32 *)(even + ROW_IMG), *(u32 *)(odd + ROW_IMG));
      }
#pragma unroll
      for (int h = 0; h < GT; h++) {
        unsigned char *at = wimg + (c8 + 32 * h) * CM_PITCH + 32 * q + 4 * bq;
        const u32 a = ww[h][4 * q], b = ww[h][4 * q + 1], c = ww[h][4 * q + 2], d = ww[h][4 * q + 3];
        u32 unused;
        gather4(a, b, c, d, *(u32 *)at, unused);
        if (PLANES == 2) gather4(hi_digits(a), hi_digits(b), hi_digits(c), hi_digits(d), *(u32 *)(at + W_IMG), unused);
      }
    }
  };

  // acc0: lo . lo; acc1: lo . hi + hi . lo (counts 256-fold).  [output tile][column tile of this wave]
  v16i acc0[GT][2], acc1[GT][2];
#pragma unroll
  for (int a = 0; a < GT; a++)
#pragma unroll
    for (int c = 0; c < 2; c++)
#pragma unroll
      for (int i = 0; i < 16; i++) { acc0[a][c][i] = 0; acc1[a][c][i] = 0; }
  const int frag = (lane & 31) * CM_PITCH + 16 * (lane >> 5);
  auto mfma_step = [&]() {
#pragma unroll
    for (int ks = 0; ks < CM_ROWS / 32; ks++) {
      v4i fa[GT][PLANES], fb[2][PLANES];
#pragma unroll
      for (int pl = 0; pl < PLANES; pl++) {
#pragma unroll
        for (int c = 0; c < 2; c++) fb[c][pl] = *(const v4i *)(rimg + pl * ROW_IMG + (2 * wave + c) * 32 * CM_PITCH + frag + 32 * ks);
#pragma unroll
        for (int a = 0; a < GT; a++) fa[a][pl] = *(const v4i *)(wimg + pl * W_IMG + a * 32 * CM_PITCH + frag + 32 * ks);
      }
#pragma unroll
      for (int a = 0; a < GT; a++) {
#pragma unroll
        for (int c = 0; c < 2; c++) {
          acc0[a][c] = __builtin_amdgcn_mfma_i32_32x32x32_i8(fa[a][0], fb[c][0], acc0[a][c], 0, 0, 0);
          if (PLANES == 2) {
            acc1[a][c] = __builtin_amdgcn_mfma_i32_32x32x32_i8(fa[a][0], fb[c][1], acc1[a][c], 0, 0, 0);
            acc1[a][c] = __builtin_amdgcn_mfma_i32_32x32x32_i8(fa[a][1], fb[c][0], acc1[a][c], 0, 0, 0);
          }
        }
      }
    }
  };

  load_step(u.r0);
  for (long rb = u.r0; rb < u.r1; rb += CM_ROWS) {
    __syncthreads();                                   // the matrix instructions of the step before have read the images
    store_step();
    __syncthreads();
    if (rb + CM_ROWS < u.r1) load_step(rb + CM_ROWS);  // in flight behind this step's matrix instructions
    mfma_step();
  }

  // Result register i of a tile is output (i & 3) + 8 (i >> 2) + 4 (lane >> 5) of its 32, column slot lane & 31.
#pragma unroll
  for (int a = 0; a < GT; a++) {
#pragma unroll
    for (int c = 0; c < 2; c++) {
      const int col = u.tile * CB_COLS + 8 * (lane & 31) + 2 * wave + c;
#pragma unroll
      for (int i = 0; i < 16; i++) {
        const int g = g0 + 32 * a + (i & 3) + 8 * (i >> 2) + 4 * (lane >> 5);
        const u32 v = (u32)acc0[a][c][i] + (PLANES == 2 ? (u32)acc1[a][c][i] << 8 : 0u);
        if (g < G && col < N) {
          if (part) part[(u.b * G + g) * N + col] = v;
          else out[(long)g * N + col] = (u16)(v & (mod - 1));
        }
      }
    }
  }
}

template <bool POW2>
__global__ void __launch_bounds__(CB_THREADS) k_combine_v(int N, u32 mod, const u16 *__restrict__ rows, const u16 *__restrict__ wts,
                                                          long B, int G, long R, int NT, int GG, u32 *__restrict__ part,
                                                          u16 *__restrict__ out) {
  typedef typename std::conditional<POW2, u32, u64>::type Acc;
  const Unit u = unit_of(B, R, NT, GG);
  const int col = u.tile * CB_COLS + threadIdx.x, g0 = u.gg * CV_OUTS;
  if (col >= N) return;
  Acc acc[CV_OUTS];
#pragma unroll
  for (int k = 0; k < CV_OUTS; k++) acc[k] = 0;
  for (long r = u.r0; r < u.r1; r++) {
    const u32 x = rows[r * N + col];
#pragma unroll
    for (int k = 0; k < CV_OUTS; k++)
      if (g0 + k < G) acc[k] += (Acc)(x * (u32)wts[r * G + g0 + k]);         // x w < 2^32
  }
#pragma unroll
  for (int k = 0; k < CV_OUTS; k++) {
    if (g0 + k >= G) continue;
    const u32 v = POW2 ? (u32)acc[k] : mod_u64((u64)acc[k], mod);
    if (part) part[(u.b * G + g0 + k) * N + col] = v;
    else out[(long)(g0 + k) * N + col] = (u16)(POW2 ? v & (mod - 1) : v);
  }
}

// out[i] = (sum over the Pb partials of part[b][i]) mod `mod`, i over the G N results; partials that are not taken modulo a power of
// two arrive reduced (< 65536, at most CB_MAX_BLOCKS of them).
template <bool POW2>
__global__ void __launch_bounds__(CB_THREADS) k_combine_finish(long total, u32 mod, long Pb, const u32 *__restrict__ part,
                                                               u16 *__restrict__ out) {
  const long i = (long)blockIdx.x * CB_THREADS + threadIdx.x;
  if (i >= total) return;
  u32 t = 0;
  for (long b = 0; b < Pb; b++) t += part[b * total + i];
  out[i] = (u16)(POW2 ? t & (mod - 1) : t % mod);
}

// The argument checks of both forms, before the engine is looked at.
int check_combine(const ntru_engine *eng, int N, int mod, const uint16_t *rows, const uint16_t *weights, int64_t B, int G,
                  const uint16_t *out) {
  const std::string who = "ntru_combine_batch: ";
  if (int rc = ntru_check_ring_mod(who, N, mod)) return rc;
  if (G < 1 || G > NTRU_COMBINE_MAX_G)
    return fail(NTRU_ERR_ARG, who + "need 1 <= G <= " + std::to_string(NTRU_COMBINE_MAX_G) + ", got G = " + std::to_string(G));
  if (B < 0 || B > ((int64_t)1 << 31)) return fail(NTRU_ERR_ARG, who + "need 0 <= B <= 2^31, got B = " + std::to_string(B));
  if (!out) return fail(NTRU_ERR_ARG, who + "NULL buffer (out)");
  if (B > 0 && (!rows || !weights)) return fail(NTRU_ERR_ARG, who + std::string("NULL buffer (") + (rows ? "weights" : "rows") + ")");
  const size_t out_bytes = (size_t)G * N * 2;
  if (ntru_ranges_overlap(out, out_bytes, rows, (size_t)B * N * 2)) return fail(NTRU_ERR_ARG, who + "out overlaps rows");
  if (ntru_ranges_overlap(out, out_bytes, weights, (size_t)B * G * 2)) return fail(NTRU_ERR_ARG, who + "out overlaps weights");
  if (!eng) return fail(NTRU_ERR_ARG, "engine is NULL");
  return NTRU_OK;
}

// Enqueues out = W^T rows for B >= 1 rows.  The launcher's rule: k_combine_m for a power-of-two modulus on kernel paths 0, 4 and 5,
// k_combine_v for everything else.
int launch_combine(ntru_engine *eng, int N, int mod, const uint16_t *d_rows, const uint16_t *d_weights, int64_t B, int G,
                   uint16_t *d_out) {
  HIP_TRY(hipSetDevice(eng->device));
  const bool pow2 = is_pow2(mod);
  const bool matrix = pow2 && matrix_path_allowed(eng);
  const int planes = mod <= 256 ? 1 : 2, gt = G <= 32 ? 1 : 2;          // k_combine_m: digit planes, output tiles per workgroup
  typedef void (*Kern)(int, u32, const u16 *, const u16 *, long, int, long, int, int, u32 *, u16 *);
  const Kern kern = !matrix ? (pow2 ? k_combine_v<true> : k_combine_v<false>)
                            : planes == 1 ? (gt == 1 ? k_combine_m<1, 1> : k_combine_m<1, 2>) : (gt == 1 ? k_combine_m<2, 1> : k_combine_m<2, 2>);
  const int NT = (N + CB_COLS - 1) / CB_COLS, GG = matrix ? (G + 32 * gt - 1) / (32 * gt) : (G + CV_OUTS - 1) / CV_OUTS;
  // row blocks: from the grid (what is co-resident), no more than fit the partials' budget, each a multiple of CB_MIN_ROWS rows (fewer
  // are not worth a partial's round trip)
  int per_cu = CV_WG_PER_CU;
  if (matrix)
    if (int rc = ntru_blocks_per_cu(eng, (const void *)kern, CB_THREADS, 0, &per_cu)) return rc;
  const size_t part_row = (size_t)G * N * 4;
  long Pb = (long)eng->cus * per_cu / ((long)NT * GG);
  Pb = std::min<long>(Pb, std::min<long>(CB_MAX_BLOCKS, (long)(CB_MAX_PART / part_row)));
  if (Pb < 1) Pb = 1;
  const long R = ((B + Pb - 1) / Pb + CB_MIN_ROWS - 1) / CB_MIN_ROWS * CB_MIN_ROWS;
  Pb = (B + R - 1) / R;
  ScratchHold hold(eng, Pb > 1 ? (size_t)Pb * part_row : 0);
  if (hold.rc) return hold.rc;
  u32 *part = Pb > 1 ? (u32 *)hold.p : nullptr;
  const dim3 grid((unsigned)(Pb * GG * NT)), block(CB_THREADS);
  hipLaunchKernelGGL(kern, grid, block, 0, eng->stream, N, (u32)mod, (const u16 *)d_rows, (const u16 *)d_weights, (long)B, G, R, NT, GG, part,
                     d_out);
  if (matrix) note_kernel(eng, "k_combine_m", planes, gt);
  else note_kernel(eng, "k_combine_v", (int)pow2, -1);
  HIP_TRY(hipGetLastError());
  if (Pb > 1) {
    const long total = (long)G * N;
    const dim3 fgrid((unsigned)((total + CB_THREADS - 1) / CB_THREADS));
    if (pow2) hipLaunchKernelGGL(k_combine_finish<true>, fgrid, block, 0, eng->stream, total, (u32)mod, Pb, part, d_out);
    else hipLaunchKernelGGL(k_combine_finish<false>, fgrid, block, 0, eng->stream, total, (u32)mod, Pb, part, d_out);
    HIP_TRY(hipGetLastError());
  }
  return NTRU_OK;
}

}  // namespace

extern "C" int ntru_combine_batch_dev(ntru_engine_t *eng, int N, int mod, const uint16_t *d_rows, const uint16_t *d_weights,
                                      int64_t B, int G, uint16_t *d_out) {
  if (int rc = check_combine(eng, N, mod, d_rows, d_weights, B, G, d_out)) return rc;
  if (B == 0) {
    HIP_TRY(hipSetDevice(eng->device));
    HIP_TRY(hipMemsetAsync(d_out, 0, (size_t)G * N * 2, eng->stream));
    return NTRU_OK;
  }
  return launch_combine(eng, N, mod, d_rows, d_weights, B, G, d_out);
}

// The rows and their weight rows flow through the chunked pipeline side by side; the sums [G][N] stay on the device for the whole call
// (eng->shared_dev): the first chunk stores them, every later chunk stores its own beside them and adds (ntru_add_batch_dev over G rows).
extern "C" int ntru_combine_batch(ntru_engine_t *eng, int N, int mod, const uint16_t *rows, const uint16_t *weights, int64_t B, int G,
                                  uint16_t *out) {
  if (int rc = check_combine(eng, N, mod, rows, weights, B, G, out)) return rc;
  for (int64_t b = 0; b < B; b++)
    for (int g = 0; g < G; g++)
      if (weights[b * G + g] >= mod)
        return fail(NTRU_ERR_ARG, "ntru_combine_batch: weight of row " + std::to_string(b) + ", column " + std::to_string(g) +
                                      " is not below mod");
  const size_t out_bytes = (size_t)G * N * 2;
  if (B == 0) { memset(out, 0, out_bytes); return NTRU_OK; }
  HIP_TRY(hipSetDevice(eng->device));
  Carve c;
  const size_t out_at = c.take(out_bytes), tmp_at = c.take(out_bytes);
  ResidentHold hold(eng, "ntru_combine_batch", c.total);
  if (hold.rc) return hold.rc;
  uint16_t *d_out = (uint16_t *)(hold.p + out_at), *d_tmp = (uint16_t *)(hold.p + tmp_at);
  Pipeline P(eng);
  const int ir = P.in(rows, (size_t)N * 2), iw = P.in(weights, (size_t)G * 2);
  int rc = P.run(B, ntru_chunk_items(B), [&](int64_t o, int64_t n, void **d) {
    return accumulate_chunk(eng, N, mod, o == 0, G, d_out, d_tmp, [&](uint16_t *dst) {
      return launch_combine(eng, N, mod, (const uint16_t *)d[ir], (const uint16_t *)d[iw], n, G, dst);
    });
  });
  if (rc) return rc;
  HIP_TRY(hipMemcpy(out, d_out, out_bytes, hipMemcpyDeviceToHost));
  return NTRU_OK;
}
