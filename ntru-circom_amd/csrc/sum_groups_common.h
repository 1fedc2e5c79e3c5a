// sum_groups_common.h -- what the kernels that sum rows in groups share (ciphertext_sum.hip: dense rows; packed_ciphertexts.hip: rows of
// packed field elements): the groups of one launch, their cut into row blocks, the layout of the partial rows that
// k_sum_groups_finish completes, the launcher that sizes and carves the scratch for them, and the body of the tally calls; and, for
// every kernel that reads dense u16 rows eight columns per lane (ciphertext_sum.hip, matrix_combine.hip), the row reads.
//
// A launch covers the rows [first offset, last offset), cut into Pb equal ROW BLOCKS.  A group that crosses a block boundary leaves one
// partial row per block it meets in `part` (u32 [Pb][2][N]): slot 0 of a block for the group that entered through the block's start,
// slot 1 for the group that leaves through its end, and meta[block] (long [Pb]) records the group of slot 1, or -1.  Partial rows are
// reduced below mod unless mod is a power of two.  k_sum_groups_finish (ciphertext_sum.hip, ntru_launch_sum_finish) adds them up.
//
// The types sit in an unnamed namespace: each translation unit's kernels take its own copy, and the kernels' symbols stay what they were
// when ciphertext_sum.hip held these lines.  Across translation units the host passes the same six values as a SumWindow
// (engine_internal.h).
#ifndef NTRU_SUM_GROUPS_COMMON_H
#define NTRU_SUM_GROUPS_COMMON_H

#include "kernels_common.h"

typedef unsigned long long u64;
typedef u32 u32x4 __attribute__((ext_vector_type(4)));
typedef u32x4 u32x4_a4 __attribute__((aligned(4)));

namespace {

// Row blocks of one launch, at most: a finish kernel (k_sum_groups_finish, k_combine_finish) adds one partial per block, each reduced
// below 65536 when the modulus is no power of two, in a u32.
constexpr long SUM_MAX_ROW_BLOCKS = 32768;

// ---- eight u16 coefficients at p (2-byte aligned) ------------------------------------------------------------------------------------
// Rows have a pitch of 2 N bytes with N odd, so every other row starts on half a dword.  A 16-byte load from a 4-byte aligned address
// runs at the full rate, so a lane reads the ALIGNED 16 bytes at or just below p plus the dword behind them (load8_raw) and shifts by 0
// or 2 bytes (pairs8: v_alignbyte; the shift is the same for the whole wave).  The caller has checked that p + 10 elements lie inside
// the array, so a batch of these loads has no branch between them.  Both take sh = half_dword(p) from the caller: worked out once per
// read, k_combine_m compiles to the stream it had with the two steps in one function; worked out in each, it does not.
__device__ __forceinline__ u32 half_dword(const u16 *p) { return (u32)((uintptr_t)p >> 1) & 1u; }      // 1: p is the upper half of a dword
__device__ __forceinline__ void load8_raw(const u16 *p, u32 sh, u32 (&d)[5]) {
  const u16 *ap = p - sh;                             // 4-byte aligned; at most 2 bytes below p, inside p's own dword
  const u32x4 v = *(const u32x4_a4 *)ap;
  d[4] = *(const u32 *)(ap + 8);
  d[0] = v[0]; d[1] = v[1]; d[2] = v[2]; d[3] = v[3];
}
// the five dwords as four dwords of two coefficients, p[2 k] in the low half of x[k]
__device__ __forceinline__ void pairs8(u32 sh, const u32 (&d)[5], u32 (&x)[4]) {
#pragma unroll
  for (int k = 0; k < 4; k++) x[k] = __builtin_amdgcn_alignbyte(d[k + 1], d[k], 2u * sh);
}
// The same pairs element by element, every one checked against `lim`, the end of the array: the last row or two only.
__device__ __forceinline__ void pairs8_checked(const u16 *p, const u16 *lim, u32 (&x)[4]) {
#pragma unroll
  for (int k = 0; k < 4; k++) x[k] = (p + 2 * k < lim ? (u32)p[2 * k] : 0u) | (p + 2 * k + 1 < lim ? (u32)p[2 * k + 1] << 16 : 0u);
}

// The groups of one launch.  off != NULL: group g is rows [off[g], off[g + 1]); else rows [(g0 + g) K, (g0 + g + 1) K).  Both
// clamped to the window [wlo, whi) (the host form's chunk; everything for the _dev form); row r lies at rows + (r - wlo) N.
struct Groups {
  const long *off;
  long K, g0, G, wlo, whi;
};

__device__ __forceinline__ long g_start(const Groups &gr, long g) {
  const long s = gr.off ? gr.off[g] : (gr.g0 + g) * gr.K;
  return s < gr.wlo ? gr.wlo : (s > gr.whi ? gr.whi : s);
}

// rows [base, end) in blocks of R; blocks 0 .. nb - 1 exist (block 0 always does)
struct Cut {
  long base, end, R, nb;
};
__device__ __forceinline__ Cut cut_of(const Groups &gr, long Pb) {
  Cut c;
  c.base = g_start(gr, 0);
  c.end = g_start(gr, gr.G);
  const long T = c.end - c.base;
  c.R = T > Pb ? (T + Pb - 1) / Pb : 1;
  c.nb = T > 0 ? (T + c.R - 1) / c.R : 1;
  return c;
}

// x mod M for an accumulator of the sums that are not taken modulo a power of two
__device__ __forceinline__ u32 mod_u64(u64 x, u32 M) {
  if ((x >> 32) == 0) return (u32)x % M;
  u32 r = (u32)(x >> 32) % M;                       // two 16-bit Horner steps below: r < M <= 65536, so (r << 16) | . fits u32
  r = ((r << 16) | ((u32)x >> 16)) % M;
  return ((r << 16) | ((u32)x & 0xffffu)) % M;
}

inline Groups groups_of(const SumWindow &w) {
  Groups gr;
  gr.off = (const long *)w.off; gr.K = w.K; gr.g0 = w.g0; gr.G = w.G; gr.wlo = w.wlo; gr.whi = w.whi;
  return gr;
}

// Enqueues the sums of the groups `w` into d_out: a row kernel whose row needs `tiles` wavefronts of workgroups of `threads`, through
// enqueue(grid, Groups, tiles, Pb, part, meta), then k_sum_groups_finish.  The scratch is [Pb] long meta | [Pb][2][N] u32 part.
template <class Enqueue>
int launch_sum_rows(ntru_engine *eng, int N, int mod, const SumWindow &w, int tiles, int waves_per_cu, int threads, uint16_t *d_out,
                    Enqueue enqueue) {
  HIP_TRY(hipSetDevice(eng->device));
  // row blocks: from the grid (waves_per_cu x CUs), and for uniform groups, whose row count the host knows, no more than there are rows
  long Pb = (long)eng->cus * waves_per_cu / tiles;
  Pb = Pb < 1 ? 1 : (Pb > SUM_MAX_ROW_BLOCKS ? SUM_MAX_ROW_BLOCKS : Pb);
  if (!w.off) {
    long T = std::min<long>(w.whi, (w.g0 + w.G) * w.K) - std::max<long>(w.wlo, w.g0 * w.K);
    if (T < 1) T = 1;
    if (Pb > T) Pb = T;
  }
  ScratchHold hold(eng, (size_t)Pb * 8 + (size_t)Pb * 2 * N * 4);
  if (hold.rc) return hold.rc;
  long *meta = (long *)hold.p;
  u32 *part = (u32 *)(hold.p + (size_t)Pb * 8);
  const dim3 grid((unsigned)((Pb * tiles + threads / 64 - 1) / (threads / 64)));
  enqueue(grid, groups_of(w), tiles, Pb, part, meta);
  HIP_TRY(hipGetLastError());
  return ntru_launch_sum_finish(eng, N, mod, w, Pb, part, meta, d_out);
}

// f(power of two?, weighted?) with the two as std::integral_constant<bool>: the instantiations of a row kernel
template <class F>
void sum_variant(bool pow2, bool weighted, F f) {
  if (pow2) weighted ? f(std::true_type{}, std::true_type{}) : f(std::true_type{}, std::false_type{});
  else weighted ? f(std::false_type{}, std::true_type{}) : f(std::false_type{}, std::false_type{});
}

// The tally calls: the checks of the sum and of the decrypt, then sum() into the intermediate `inter` and decrypt() of it.  `buffers` is
// false when a buffer that the two need is NULL.
template <class Sum, class Decrypt>
int tally_decrypt(ntru_engine *eng, const char *who, int N, int q, int p, bool uniform, int64_t K, int64_t G, bool buffers,
                  const char *inter, Sum sum, Decrypt decrypt) {
  if (int rc = ntru_check_sum_args(eng, N, q, uniform, K, G, who)) return rc;
  if (int rc = ntru_decrypt_batch_dev(eng, N, q, p, nullptr, nullptr, nullptr, 0, nullptr, nullptr, nullptr, nullptr)) return rc;
  if (G == 0) return NTRU_OK;
  if (!buffers) return fail(NTRU_ERR_ARG, std::string(who) + ": NULL buffer (" + inter + " is needed as the intermediate)");
  if (int rc = sum()) return rc;
  return decrypt();
}

}  // namespace

#endif
