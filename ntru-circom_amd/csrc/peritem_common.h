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

// Per wave: the natural-order area (pi_nat_bytes: three periods of the ternary / Toeplitz operand, later a product's natural-order image,
// e.g. product 3's remainder for the comparison with h), then `arrays` (1 or 2) reversed arrays of four byte-shifted copies each.  No
// chunk matrix: the rows live in registers.  Used by every kernel body and by its launcher.
static __host__ __device__ inline size_t pi_wave_bytes(const PGeom &g, int arrays) { return pi_nat_bytes(g) + (size_t)arrays * 16 * g.tpitch; }

// Lane (r, hh) = 32 hh + r holds chunk 2 r + hh (16 coefficients) of every operand row -- the layout the matrix instruction wants its
// A operand in -- and accumulator register i of that lane holds index pi_ko(i) + pi_index_of(lane).
static __device__ __forceinline__ int pi_chunk_of(int lane) { return 2 * (lane & 31) + (lane >> 5); }
static __device__ __forceinline__ int pi_index_of(int lane) { return 128 * (lane >> 5) + (lane & 31); }
constexpr int pi_ko(int i) { return 32 * ((i & 3) + 8 * (i >> 2)); }

// One operand row of an item on its way from HBM into this lane's registers: 16 coefficients of NCH bytes each per lane.  An item's rows
// are requested one item AHEAD (a wave that fetched them where it needs them sat idle for a round trip to HBM per item) and stay in
// `raw` across the loop back-edge; take them with the row's own pointer, whose low four bits are the shift.
template <int NCH>
struct PiRow {
  RawChunks<NCH> raw;
  // Row `item` of rows[B][N], chunk ch of it.  The descriptor covers ONE row: the lanes whose chunk lies beyond it -- chunks NT .. 63 --
  // read zeros instead of fetching the next items' rows.
  template <class E>
  __device__ __forceinline__ void request(const E *rows, long item, int N, int ch) {
    static_assert(sizeof(E) == NCH, "16 coefficients per lane");
    const AlignedSrc s = aligned_src(rows + item * N, (long)NCH * N);
    raw = load_raw<NCH>(s, s.a0 + 16 * NCH * ch, 0);
  }
  __device__ __forceinline__ void take(const void *row, v4i (&v)[NCH]) const {
    shift_raw<NCH>(raw, __builtin_amdgcn_readfirstlane((int)((unsigned long long)row & 15)), v);
  }
  __device__ __forceinline__ v4i bytes(const void *row) const {              // NCH == 1
    v4i v[NCH];
    take(row, v);
    return v[0];
  }
  __device__ __forceinline__ void pairs(const void *row, u32 (&x)[8]) const {   // NCH == 2: what pi_digits wants
    v4i v[NCH];
    take(row, v);
#pragma unroll
    for (int c = 0; c < 4; c++) { x[c] = (u32)v[0][c]; x[4 + c] = (u32)v[NCH - 1][c]; }
  }
};

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

// Sixteen bytes modulo 3.  A key's fp is already reduced: one wave-wide test (is any byte >= 3?) skips the byte-wise division.
static __device__ __forceinline__ v4i pi_mod3_bytes(v4i v) {
  union { v4i v; unsigned char c[16]; } u; u.v = v;
  u32 big = 0;
#pragma unroll
  for (int c = 0; c < 4; c++) big |= ((((u32)u.v[c] & 0x7F7F7F7Fu) + 0x7D7D7D7Du) | (u32)u.v[c]) & 0x80808080u;
  if (__ballot(big != 0) != 0) {
#pragma unroll
    for (int j = 0; j < 16; j++) u.c[j] = (unsigned char)((u32)u.c[j] % 3u);
  }
  return u.v;
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

// The split (quotient-keeping) product loop, driven by a compile-time PLAN: planes F[p] (unshifted chunk rows of this lane, zero at and
// beyond N) against the Toeplitz fragments of one or two reversed arrays ("streams": stream s lies 4 s tpitch dwords above T), summed
// into accumulators L[a] / H[a] = low / high half.  A plan lists the terms acc += plane (x) stream and, for each, the plane behind
// whose shift it issues; the sched_barrier(0) closes the group of every plane, so that the next plane's shifts issue under the group's
// matrix instructions.  Low and high parts advance together (independent fragment reads, fragments requested one trip ahead, unrolled
// by two so that the two fragment sets rotate without moves).
struct PiTerm { int plane, stream, acc, after; };
template <class Plan, int NP, int NA>
static __device__ __forceinline__ void pi_product_plan(const v4i (&F)[NP], const u32 *T, const PGeom &g, int lane_, v16i (&L)[NA], v16i (&H)[NA]) {
  constexpr int NS = Plan::streams, NTERM = Plan::terms;
  const int lane = opaque(lane_), NT = g.NT;
  const int y0 = 32 * NT - 1 - (lane & 31) + 16 * (lane >> 5);
  const u32 *tb = T + (y0 & 3) * g.tpitch + (y0 >> 2);     // this lane's fragment of distance 0; distance d lies 8 d dwords below
  const int tstep = 4 * g.tpitch;
  int seam_up = lane == 32 ? 0 : -1, seam_dn = lane == 31 ? 0 : -1;
  asm volatile("" : "+v"(seam_up), "+v"(seam_dn));         // (opaque: as a known 0 / -1 the AND becomes a select that cannot carry the DPP shift)
  struct Fr { v4i w[NS]; };
  auto frag = [&](int d) {                                 // |d| <= NT - 1; requests past the last step read the last fragment again
    d = d > NT - 1 ? NT - 1 : (d < 1 - NT ? 1 - NT : d);
    Fr fr;
#pragma unroll
    for (int s = 0; s < NS; s++) {
      const u32 *p = tb - 8 * d + s * tstep;
      fr.w[s] = (v4i){(int)p[0], (int)p[1], (int)p[2], (int)p[3]};
    }
    return fr;
  };
  const v16i zero = {0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0};
  const Fr f0 = frag(0);
  Fr la = frag(1), ha = frag(-1), lb, hb;
  {                                                        // d = 0: split by the diagonal mask; the first term of every accumulator
    u32 mlow[4], mhigh[4];
    pi_diag_low_mask(lane, mlow);
#pragma unroll
    for (int c = 0; c < 4; c++) mhigh[c] = ~mlow[c];
    Fr wl, wh;
#pragma unroll
    for (int s = 0; s < NS; s++) { wl.w[s] = and4(f0.w[s], mlow); wh.w[s] = and4(f0.w[s], mhigh); }
#pragma unroll
    for (int t = 0; t < NTERM; t++) {
      constexpr auto first = [](int t_) { for (int u = 0; u < t_; u++) if (Plan::term(u).acc == Plan::term(t_).acc) return false; return true; };
      const PiTerm k = Plan::term(t);
      L[k.acc] = __builtin_amdgcn_mfma_i32_32x32x32_i8(F[k.plane], wl.w[k.stream], first(t) ? zero : L[k.acc], 0, 0, 0);
      H[k.acc] = __builtin_amdgcn_mfma_i32_32x32x32_i8(F[k.plane], wh.w[k.stream], first(t) ? zero : H[k.acc], 0, 0, 0);
    }
  }
  v4i AL[NP], AH[NP];
#pragma unroll
  for (int p = 0; p < NP; p++) { AL[p] = F[p]; AH[p] = F[p]; }
  auto trip = [&](const Fr &wl, const Fr &wh) {
#pragma unroll
    for (int p = 0; p < NP; p++) {
      AL[p] = rows_up(AL[p], seam_up);
#pragma unroll
      for (int t = 0; t < NTERM; t++)
        if (Plan::term(t).after == p) L[Plan::term(t).acc] = __builtin_amdgcn_mfma_i32_32x32x32_i8(AL[Plan::term(t).plane], wl.w[Plan::term(t).stream], L[Plan::term(t).acc], 0, 0, 0);
      __builtin_amdgcn_sched_barrier(0);                   // the next plane's shifts issue under these matrix instructions
    }
#pragma unroll
    for (int p = 0; p < NP; p++) {
      AH[p] = rows_down(AH[p], seam_dn);
#pragma unroll
      for (int t = 0; t < NTERM; t++)
        if (Plan::term(t).after == p) H[Plan::term(t).acc] = __builtin_amdgcn_mfma_i32_32x32x32_i8(AH[Plan::term(t).plane], wh.w[Plan::term(t).stream], H[Plan::term(t).acc], 0, 0, 0);
      __builtin_amdgcn_sched_barrier(0);
    }
  };
  int j = 1;
  for (; j + 1 < NT; j += 2) {
    lb = frag(j + 1); hb = frag(-(j + 1));
    trip(la, ha);
    la = frag(j + 2); ha = frag(-(j + 2));
    trip(lb, hb);
  }
  if (j < NT) trip(la, ha);
}

// NPL planes against ONE reversed array: L[p] / H[p] = low / high half of plane p's product.
template <int NPL>
struct PiPlanPlanes {
  static constexpr int streams = 1, terms = NPL;
  static constexpr PiTerm term(int t) { return {t, 0, t, t}; }
};
template <int NPL>
static __device__ __forceinline__ void pi_product_reg(const v4i (&F)[NPL], const u32 *T, const PGeom &g, int lane, v16i (&L)[NPL], v16i (&H)[NPL]) {
  pi_product_plan<PiPlanPlanes<NPL>>(F, T, g, lane, L, H);
}

// The epilogue of a split product: f(i, ko, lo, hi) for the sixteen accumulator registers with the digit planes combined (value = acc0 +
// 128 acc1), lo / hi = low / high half of coefficient ko + pi_index_of(lane): remainder = lo + hi, quotient = -hi (modulo q).
template <int NPL, class Fn>
static __device__ __forceinline__ void pi_for_split(const v16i *L, const v16i *H, Fn f) {     // L[0 .. NPL - 1], H likewise
#pragma unroll
  for (int i = 0; i < 16; i++) {
    const u32 lo = (u32)L[0][i] + (NPL == 1 ? 0u : 128u * (u32)L[NPL - 1][i]), hi = (u32)H[0][i] + (NPL == 1 ? 0u : 128u * (u32)H[NPL - 1][i]);
    f(i, pi_ko(i), lo, hi);
  }
}

// index.js:159: a remainder is invalid iff it has a non-zero coefficient above the constant one AND its constant one is not 1
// (length !== 1 && [0] !== 1).  Register i of lane kl = pi_index_of(lane) holds index ko_i + kl: it exists iff ko_i < N - kl (one compare
// against a per-lane limit, ko_i a constant); coefficient 0 is register 0 of lane 0.  Register 0 is no exception to the limit: below
// N = 160 the lanes kl = 128 .. 159 hold indices at and beyond N there (tiles >= NT: junk that must not count).
struct PiNotOne {
  u32 any_hi = 0, c0 = 0;
  __device__ __forceinline__ void see(int i, int ko, int kl, int N, u32 rv) {
    if (i == 0) { c0 = rv; any_hi |= kl == 0 || kl >= N ? 0u : rv; }
    else any_hi |= ko < N - kl ? rv : 0u;
  }
  __device__ __forceinline__ bool invalid(int kl) const {                   // wave-wide
    const bool nz_hi = any_hi != 0, first_not_one = kl == 0 && c0 != 1;
    return __ballot(nz_hi) != 0 && __ballot(first_not_one) != 0;
  }
};

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

// A launch of the family: one item per wave, PI_WAVES waves per workgroup, each with wave_bytes of LDS.
template <class Kern, class... Args>
static int launch_peritem(ntru_engine *eng, Kern kern, long B, size_t wave_bytes, Args... args) {
  return launch_resident(eng, kern, (B + PI_WAVES - 1) / PI_WAVES, 64 * PI_WAVES, PI_WAVES * wave_bytes, args...);
}

#endif
