// peritem_common.h -- the per-item matrix-core machinery (family 4 with PER-ITEM operands) that more than one translation unit
// uses: wave geometry, digit planes, the reversed Toeplitz array built from one chunk per lane, and the quotient-keeping product
// with the chunk rows in registers.  Included by matrix_peritem.hip and matrix_peritem_scheme.hip; tools/peritem_mfma_model.py is
// the executable specification.
#ifndef NTRU_PERITEM_COMMON_H
#define NTRU_PERITEM_COMMON_H

#include "matrix_common.h"

// ---- family 4 for PER-ITEM operands: verifyKeysInputs (index.js:141-197) on the matrix cores ---------------------
// No matrix is shared by the batch, but one product c = a * s is itself a 32-row matrix product per tile distance
// d = kb - ib (tools/peritem_mfma_model.py): C[kb][k'] += sum_i' F[kb - d][i'] G_d[i'][k'] with F the 32-coefficient chunks
// of a (rows = output tiles) and G_d the Toeplitz tile of s (fragments of the reversed cyclic array the wave builds per item in
// its own LDS, as in the shared-key kernels).  One accumulator pair (low / high) holds the whole product of an item; a 13-bit
// operand contributes two digit planes with SEPARATE accumulators (value = acc0 + 128 acc1), so nothing is scaled.
// 2 NT - 1 (+1 for the split diagonal) matrix instructions per plane.  One item per wave, all LDS regions private to the wave,
// no workgroup barrier.  The chunk rows never touch the LDS: see "chunk rows in REGISTERS" below.
constexpr int PI_WAVES = 2;         // waves per workgroup (registers bound the residency); 4 measured the same
struct PGeom { int N, NT, tpitch; };
// Natural-order area of a wave: three periods + 64 bytes of the ternary / Toeplitz operand while its reversed array is built; later a
// product's results as a natural-order image written from the accumulator layout, where register i of lane (r, hh) holds index
// 32 ((i&3) + 8 (i>>2)) + 128 hh + r <= 1151 WHATEVER N is (tiles at and beyond NT hold junk that nobody reads): 2304 bytes of u16.
static __host__ __device__ inline size_t pi_nat_bytes(const PGeom &g) {
  const size_t periods = ((size_t)3 * g.N + 64 + 15) & ~(size_t)15;
  return periods > 2304 ? periods : 2304;
}

// Digit planes of 16 values (u16 pairs in x[8], element i0 + j; zero at and beyond N) -> natural-order int8 bytes, on
// packed 16-bit pairs.  mul: the operand is (mul v) mod q (p fq of index.js:155; 1 otherwise).  q > 256: v = d0 + 128 d1 with
// d0 = v & 127, d1 = v >> 7 <= 63 (the two planes have SEPARATE accumulators, so nothing needs a signed representative).
// q <= 256: ONE plane, the centred representative in [-q/2, q/2) (d1 = 0; the callers skip that plane's matrix instructions).
static __device__ __forceinline__ void pi_digits(const u32 (&x)[8], u32 q, u32 mul, int i0, int N, v4i &o0, v4i &o1) {
  const u32 qm2 = (q - 1) * 0x00010001u;
  u32 v[8];
#pragma unroll
  for (int c = 0; c < 8; c++) {
    const int left = N - (i0 + 2 * c);                     // valid elements of this pair
    const u32 keep = left >= 2 ? 0xFFFFFFFFu : (left == 1 ? 0x0000FFFFu : 0u);
    const u32 t = mul == 1u ? x[c] : as_u32(as_pair(x[c]) * (u16x2){(u16)mul, (u16)mul});
    v[c] = t & qm2 & keep;
  }
  if (q <= 256) {
    const u32 h2 = (q >> 1) * 0x00010001u;
#pragma unroll
    for (int c = 0; c < 4; c++) {
      const u32 a = as_u32(as_pair((as_u32(as_pair(v[2 * c]) + as_pair(h2)) & qm2)) - as_pair(h2));           // two's complement low bytes
      const u32 b = as_u32(as_pair((as_u32(as_pair(v[2 * c + 1]) + as_pair(h2)) & qm2)) - as_pair(h2));
      o0[c] = (int)__builtin_amdgcn_perm(b, a, 0x06040200u);
      o1[c] = 0;
    }
  } else {
#pragma unroll
    for (int c = 0; c < 4; c++) {
      const u32 a = v[2 * c], b = v[2 * c + 1];
      o0[c] = (int)__builtin_amdgcn_perm(b & 0x007F007Fu, a & 0x007F007Fu, 0x06040200u);
      o1[c] = (int)__builtin_amdgcn_perm((b >> 7) & 0x007F007Fu, (a >> 7) & 0x007F007Fu, 0x06040200u);
    }
  }
}

// Ternary operand bytes: any negative byte is -1 (ValTernary), bytes outside the mask (at and beyond N) are zero -- four at a time.
static __device__ __forceinline__ v4i pi_ternary(v4i v, const v4i &cmask) {
  v4i o;
#pragma unroll
  for (int c = 0; c < 4; c++) {
    const u32 w = (u32)(v[c] & cmask[c]);
    o[c] = (int)(w | ((w >> 7) & 0x01010101u) * 0xFFu);    // (1 in every negative byte, spread to 0xFF: no carries)
  }
  return o;
}

// ---- chunk rows in REGISTERS (k_verify_keys_m) -----------------------------------------------------------------------------------
// The A operand of tile distance d is the chunk matrix moved down by d rows: lane (r, hh) holds bytes 16 hh .. 16 hh + 15 of chunk
// r - d.  Going from d to d + 1 (d >= 0) every lane takes its lower neighbour's 16 bytes and nothing enters at row 0; going from d to
// d - 1 (d <= 0) every lane takes its upper neighbour's and nothing enters at row 31 (chunks >= NT are zero).  So the low part walks
// d = 1, 2, ... and the high part d = -1, -2, ..., each from the unshifted rows, with ONE v_and_b32_dpp per dword and step (wave_shr /
// wave_shl by one lane; the AND cuts the seam between the two half-waves: lane 32 would take lane 31's row, lane 31 lane 32's) and
// no LDS read for the rows at all.  [Round 3 had tried the shift the other way round -- the high part walking d upwards, a new row
// entering at lane 0 every step through a small LDS read and v_cndmask_b32_dpp: slower than reading the rows.]  The loops' LDS
// traffic is the fragment reads alone, shared by every plane that multiplies the same Toeplitz operand: 1 KB per step for the three
// planes of products 1 and 2 (fq lo / hi and fp against f) where the LDS-row form read 5 KB.  bench_micro/peritem_step.hip is the probe.

// A fresh copy of a lane-dependent value that the compiler cannot trace back: everything derived from it is computed where it is used,
// instead of being hoisted out of the item loop (per-lane addresses and masks of every phase: dozens of registers live for ever, i.e.
// spilled at three waves per SIMD).
static __device__ __forceinline__ int opaque(int v) { asm volatile("" : "+v"(v)); return v; }

// diag_low_mask (matrix_common.h) for kernels that make the mask once per PRODUCT instead of once per launch: byte jj of dword c is
// set iff r >= 16 hh + 4 c + jj, i.e. the n = clamp(r - 16 hh - 4 c + 1, 0, 4) low bytes -- a handful of instructions per dword
// where sixteen byte-wise compare / select pairs cost ~50.
static __device__ __forceinline__ void pi_diag_low_mask(int lane, u32 (&mlow)[4]) {
  const int u = (lane & 31) - 16 * (lane >> 5) + 1;
#pragma unroll
  for (int c = 0; c < 4; c++) {
    const int n = min(max(u - 4 * c, 0), 4);
    mlow[c] = n >= 4 ? 0xFFFFFFFFu : ((1u << (8 * n)) - 1u);
  }
}

static __device__ __forceinline__ v4i rows_up(v4i a, int seam) {          // lane l <- lane l - 1 (lane 0 <- 0)
  v4i o;
#pragma unroll
  for (int c = 0; c < 4; c++) o[c] = __builtin_amdgcn_update_dpp(0, a[c], 0x138, 0xf, 0xf, true) & seam;
  return o;
}
static __device__ __forceinline__ v4i rows_down(v4i a, int seam) {        // lane l <- lane l + 1 (lane 63 <- 0)
  v4i o;
#pragma unroll
  for (int c = 0; c < 4; c++) o[c] = __builtin_amdgcn_update_dpp(0, a[c], 0x130, 0xf, 0xf, true) & seam;
  return o;
}

// NPL planes F[p] (unshifted chunk rows of this lane, zero at and beyond N) against the Toeplitz fragments of T: L[p] / H[p] = low /
// high half of plane p's product.  Low and high parts advance together (two independent fragment reads and 2 NPL matrix
// instructions per trip, fragments requested one trip ahead, unrolled by two so that the two fragment sets rotate without moves).
template <int NPL>
static __device__ __forceinline__ void pi_product_reg(const v4i (&F)[NPL], const u32 *T, const PGeom &g, int lane_, v16i (&L)[NPL], v16i (&H)[NPL]) {
  const int lane = opaque(lane_), NT = g.NT;
  const int y0 = 32 * NT - 1 - (lane & 31) + 16 * (lane >> 5);
  const u32 *tb = T + (y0 & 3) * g.tpitch + (y0 >> 2);     // this lane's fragment of distance 0; distance d lies 8 d dwords below
  int seam_up = lane == 32 ? 0 : -1, seam_dn = lane == 31 ? 0 : -1;
  asm volatile("" : "+v"(seam_up), "+v"(seam_dn));         // (opaque: as a known 0 / -1 the AND becomes a select that cannot carry the DPP shift)
  auto frag = [&](int d) {                                 // |d| <= NT - 1; requests past the last step read the last fragment again
    d = d > NT - 1 ? NT - 1 : (d < 1 - NT ? 1 - NT : d);
    const u32 *p = tb - 8 * d;
    return (v4i){(int)p[0], (int)p[1], (int)p[2], (int)p[3]};
  };
  const v16i zero = {0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0};
  v4i AL[NPL], AH[NPL];
  const v4i w0 = frag(0);
  v4i wl_a = frag(1), wh_a = frag(-1), wl_b, wh_b;
  {                                                        // d = 0: split by the diagonal mask; the first term of every accumulator
    u32 mlow[4];
    pi_diag_low_mask(lane, mlow);
    const v4i wl = and4(w0, mlow);
    const v4i wh = {(int)((u32)w0[0] & ~mlow[0]), (int)((u32)w0[1] & ~mlow[1]), (int)((u32)w0[2] & ~mlow[2]), (int)((u32)w0[3] & ~mlow[3])};
#pragma unroll
    for (int p = 0; p < NPL; p++) {
      L[p] = __builtin_amdgcn_mfma_i32_32x32x32_i8(F[p], wl, zero, 0, 0, 0);
      H[p] = __builtin_amdgcn_mfma_i32_32x32x32_i8(F[p], wh, zero, 0, 0, 0);
      AL[p] = F[p]; AH[p] = F[p];
    }
  }
  auto trip = [&](const v4i &wl, const v4i &wh) {
#pragma unroll
    for (int p = 0; p < NPL; p++) {
      AL[p] = rows_up(AL[p], seam_up);
      L[p] = __builtin_amdgcn_mfma_i32_32x32x32_i8(AL[p], wl, L[p], 0, 0, 0);
      __builtin_amdgcn_sched_barrier(0);                   // the next plane's shifts issue under this matrix instruction
    }
#pragma unroll
    for (int p = 0; p < NPL; p++) {
      AH[p] = rows_down(AH[p], seam_dn);
      H[p] = __builtin_amdgcn_mfma_i32_32x32x32_i8(AH[p], wh, H[p], 0, 0, 0);
      __builtin_amdgcn_sched_barrier(0);
    }
  };
  int j = 1;
  for (; j + 1 < NT; j += 2) {
    wl_b = frag(j + 1); wh_b = frag(-(j + 1));
    trip(wl_a, wh_a);
    wl_a = frag(j + 2); wh_a = frag(-(j + 2));
    trip(wl_b, wh_b);
  }
  if (j < NT) trip(wl_a, wh_a);
}

// Per wave: three natural-order periods of the ternary operand (the source of its reversed array; later the remainder of product 3
// for the comparison with h), then the reversed array.  No chunk matrix: the rows live in registers.
static __host__ __device__ inline size_t pi_reg_wave_bytes(const PGeom &g) { return pi_nat_bytes(g) + (size_t)16 * g.tpitch; }

// Reversed cyclic array (4 byte-shifted copies) of a ternary / int8 operand of which this lane holds chunk ch (the 16 bytes sv:
// coefficients 16 ch .. 16 ch + 15, zero at and beyond N; any assignment of chunks to lanes): three periods in natural order (period
// k starts at byte k N, any alignment: unaligned LDS stores), then T[c][w] = bytes rev[4w + c + j], rev[y] = s[(Y0 - y) mod N], as
// byte-swapped reads.  The last chunk of a period is stored whole: its zero tail lands on the next period's first bytes, which the
// NEXT store instruction writes (the LDS executes one wave's instructions in order).
static __device__ __forceinline__ void pi_build_array_ch(unsigned char *nat, u32 *T, const PGeom &g, int lane_, int ch, v4i sv) {
  const int N = g.N, Y0 = 32 * g.NT - 1, lane = opaque(lane_);
  const bool holds = 16 * ch < N;
#pragma unroll
  for (int k = 0; k < 3; k++)
    if (holds) *(v4i *)(nat + k * N + 16 * ch) = sv;
  if (ch < 4) *(v4i *)(nat + 3 * N + 16 * ch) = sv;        // N >= 64
  wave_lds_fence();
  // Word w of copy c holds bytes nat[A .. A+3] reversed, A = E - c, E = Y0 + 2N - 3 - 4w.  E & 3 is the same for every
  // lane, so the four copies of a word come from three ALIGNED dwords around E >> 2 with one byte permute each
  // (an unaligned LDS dword read costs several aligned ones).
  const u32 *D = (const u32 *)nat;
  const int e = __builtin_amdgcn_readfirstlane((Y0 + 2 * N - 3) & 3);
  u32 sel[4]; int dk[4];
#pragma unroll
  for (int c = 0; c < 4; c++) {
    const int al = c <= e ? e - c : e - c + 4;                            // byte offset of A inside its dword
    dk[c] = c <= e ? 0 : -1;                                              // ... which is dword K or K - 1
    sel[c] = 0x00010203u + 0x01010101u * (u32)al;                         // bytes al+3, al+2, al+1, al of the pair (reversed)
  }
  // A lane makes FOUR consecutive words of all four copies per trip (one 16-byte store per copy) from six consecutive source dwords:
  // two trips cover a copy at N = 821 where word-per-lane trips took seven dependent LDS round trips.
  const int K0 = (Y0 + 2 * N - 3) >> 2;
  for (int w0 = 4 * lane; w0 < g.tpitch; w0 += 256) {      // tpitch is a multiple of 4 (and a copy's size of 16 bytes)
    int base = K0 - w0 - 4;                                // words w0 + j need dwords K0 - w0 - j - 1 .. K0 - w0 - j + 1
    base = base < 0 ? 0 : base;                            // (only pad words of a copy, which are never read, lie that far out)
    u32 d[6];
#pragma unroll
    for (int i = 0; i < 6; i++) d[i] = D[base + i];
#pragma unroll
    for (int c = 0; c < 4; c++) {
      v4i o;
#pragma unroll
      for (int j = 0; j < 4; j++)
        o[j] = (int)(dk[c] == 0 ? __builtin_amdgcn_perm(d[5 - j], d[4 - j], sel[c]) : __builtin_amdgcn_perm(d[4 - j], d[3 - j], sel[c]));
      *(v4i *)(T + c * g.tpitch + w0) = o;
    }
  }
  wave_lds_fence();
}

// ---- host side ----------------------------------------------------------------------------------------------------------
static inline PGeom make_pgeom(int N) {
  PGeom pg;
  pg.N = N; pg.NT = (N + 31) / 32; pg.tpitch = ((16 * pg.NT + 31) / 32) * 32 + 8;
  return pg;
}
// The per-item matrix kernels: modulus a power of two <= 8192 (two int8 digit planes), 64 <= N <= 1024; automatic from N = 128.
static inline bool peritem_applies(const ntru_engine *eng, int N, int q) {
  return matrix_path_allowed(eng) && is_pow2(q) && q <= 8192 && N <= 1024 && N >= (eng->path >= 4 ? 64 : 128);
}

#endif
