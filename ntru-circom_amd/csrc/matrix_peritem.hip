// matrix_peritem.hip -- MI355X (gfx950), family 4 with PER-ITEM operands: verifyKeysInputs (index.js:141-197), the generic product
// multiplyPolynomials + dividePolynomials by I (index.js:319-401) and products with a ternary operand (public key, Newton rounds of
// the key inversion), one item per wavefront on the int8 matrix cores.  tools/peritem_mfma_model.py is the executable specification.
#include "peritem_common.h"

// The half of the reversed array that the distances d >= 0 read (products modulo x^N - 1: pi_product_cyc): words w < 8 NT + 8 of
// every copy, which look at stream bytes 2N - 36 .. 3N + 34 only -- ONE period and two margins.  So the period is stored once, at the
// 16-byte aligned PI_HALF_BASE, and the margins (the last <= 4 chunks in front of it, the first three behind it) by ONE store
// instruction of other lanes: an LDS access of 16 bytes off its natural alignment is replayed at 64 cycles per wave instruction
// (MI355X guide, LDS), and the three-period form pays that three times per array.  With the period aligned the byte phase of the
// words is 0 for every N: constant selectors.  (The margins first: the zero tail of the last chunk lands on the period's first
// bytes, which the period's own store then writes.)
constexpr int PI_HALF_BASE = 64;
static __device__ __forceinline__ void pi_build_array_half(unsigned char *nat, u32 *T, const PGeom &g, int lane_, int ch, v4i sv) {
  const int N = g.N, lane = opaque(lane_);
  const bool holds = 16 * ch < N, behind = ch < 3, front = holds && 16 * ch + 15 >= N - 36;
  if (N >= 160) {                                          // (chunks 0 .. 2 are none of the last four)
    if (behind || front) *(v4i *)(nat + PI_HALF_BASE + (behind ? N : -N) + 16 * ch) = sv;
  } else {
    if (front) *(v4i *)(nat + PI_HALF_BASE - N + 16 * ch) = sv;
    if (behind) *(v4i *)(nat + PI_HALF_BASE + N + 16 * ch) = sv;
  }
  if (holds) *(v4i *)(nat + PI_HALF_BASE + 16 * ch) = sv;
  wave_lds_fence();
  // Word w of copy c holds stream bytes A .. A + 3 reversed, A = E - c, E = PI_HALF_BASE + 32 NT - 4 - 4 w: a multiple of 4.
  const u32 *D = (const u32 *)nat;
  const int K0 = (PI_HALF_BASE >> 2) + 8 * g.NT - 1;
  for (int w0 = 4 * lane; w0 < 8 * g.NT + 8; w0 += 256) {
    const int base = K0 - w0 - 4;                          // >= 3; words w0 + j need dwords K0 - w0 - j - 1, K0 - w0 - j
    u32 d[6];
#pragma unroll
    for (int i = 0; i < 6; i++) d[i] = D[base + i];
#pragma unroll
    for (int c = 0; c < 4; c++) {
      v4i o;
#pragma unroll
      for (int j = 0; j < 4; j++)
        o[j] = (int)(c == 0 ? __builtin_amdgcn_perm(d[5 - j], d[4 - j], 0x00010203u)
                            : __builtin_amdgcn_perm(d[4 - j], d[3 - j], 0x00010203u + 0x01010101u * (u32)(4 - c)));
      *(v4i *)(T + c * g.tpitch + w0) = o;
    }
  }
  wave_lds_fence();
}

// ---- products modulo x^N - 1 ONLY (Newton rounds, public key): ONE matrix instruction per tile distance -------------------------
// The wrapped terms a[i] s[k - i + N] (i > k) meet the SAME fragment as the unwrapped ones of distance d when their rows come from a
// copy of `a` moved up by P = 32 NT - N places (tools/peritem_mfma_model.py product_cyclic_registers): row kb of distance d is chunk
// kb - d of a (kb >= d) or chunk kb - d + NT of the moved copy (kb < d).  So the rows walk UP one lane per distance, and chunk NT - d of
// the moved copy ENTERS at row 0 -- two lanes -- from a byte image of that copy in the wave's LDS (byte P + i = a[i]; every lane of a
// half-wave reads the same 16 bytes: a broadcast).  One v_cndmask_b32_dpp per dword does both (vcc = lanes 0 and 32: the entering
// halves; every other lane its lower neighbour's dword -- which also cuts the seam at lane 32).  The distance-0 tile is taken whole
// (above its diagonal lie the wrapped terms inside the tile), so the P coefficients that chunk kb + 1 of the moved copy shares with
// chunk kb of `a` are cut from the rows of the LAST distance, where that chunk sits at row kb.  NT matrix instructions and one
// accumulator per plane where the split form takes 2 NT and two.
constexpr int PI_IMG = 1152;        // bytes between the images of two planes (P + 32 NT <= 1055)

static __device__ __forceinline__ v4i rows_up_enter(const v4i a, const v4i e) {
  int o0, o1, o2, o3;                                      // (untied, early-clobber outputs: the rows ping-pong between two register tuples, no moves)
  asm volatile(
      "s_mov_b32 vcc_lo, 1\n\ts_mov_b32 vcc_hi, 1\n\ts_nop 1\n\t"
      "v_cndmask_b32_dpp %0, %4, %8, vcc wave_shr:1 row_mask:0xf bank_mask:0xf bound_ctrl:1\n\t"
      "v_cndmask_b32_dpp %1, %5, %9, vcc wave_shr:1 row_mask:0xf bank_mask:0xf bound_ctrl:1\n\t"
      "v_cndmask_b32_dpp %2, %6, %10, vcc wave_shr:1 row_mask:0xf bank_mask:0xf bound_ctrl:1\n\t"
      "v_cndmask_b32_dpp %3, %7, %11, vcc wave_shr:1 row_mask:0xf bank_mask:0xf bound_ctrl:1"
      : "=&v"(o0), "=&v"(o1), "=&v"(o2), "=&v"(o3)
      : "v"(a[0]), "v"(a[1]), "v"(a[2]), "v"(a[3]), "v"(e[0]), "v"(e[1]), "v"(e[2]), "v"(e[3])
      : "vcc");
  return (v4i){o0, o1, o2, o3};
}

// This lane's 16 bytes of a plane (chunk ch: coefficients 16 ch .. 16 ch + 15, zero at and beyond N) into the plane's image.
static __device__ __forceinline__ void pi_store_image(unsigned char *img, const PGeom &g, int ch, v4i bytes) {
  if (16 * ch < 32 * g.NT) *(v4i *)(img + (32 * g.NT - g.N) + 16 * ch) = bytes;     // (any alignment)
}

// NPL planes F[p] (this lane's unshifted chunk rows) whose images lie at img + p PI_IMG, against the fragments of T: C[p] = plane p's
// product modulo x^N - 1.  Fragment and entering rows are requested one trip ahead, unrolled by two so that the sets rotate without moves.
// The byte mask of the last distance (pi_product_cyc): rows <= NT - 2 lose their bytes 16 hh + j < P = 32 NT - N.  Once per item.
static __device__ __forceinline__ void pi_cyc_keep(const PGeom &g, int lane_, u32 (&keep)[4]) {
  const int lane = opaque(lane_), P = 32 * g.NT - g.N, u = (lane & 31) <= g.NT - 2 ? P - 16 * (lane >> 5) : 0;
#pragma unroll
  for (int c = 0; c < 4; c++) {
    const int n = min(max(u - 4 * c, 0), 4);
    keep[c] = n >= 4 ? 0u : ~((1u << (8 * n)) - 1u);
  }
}

template <int NPL>
static __device__ __forceinline__ void pi_product_cyc(const v4i (&F)[NPL], const unsigned char *img, const u32 *T, const PGeom &g, int lane_,
                                                      const u32 (&keep)[4], v16i (&C)[NPL]) {
  const int lane = opaque(lane_), NT = g.NT;
  const int y0 = 32 * NT - 1 - (lane & 31) + 16 * (lane >> 5);
  const u32 *tb = T + (y0 & 3) * g.tpitch + (y0 >> 2);     // this lane's fragment of distance 0; distance d lies 8 d dwords below
  const unsigned char *eb = img + 32 * NT + 16 * (lane >> 5);                // chunk NT - d of the image: 32 d bytes below
  auto frag = [&](int d) {
    const u32 *p = tb - 8 * d;
    return (v4i){(int)p[0], (int)p[1], (int)p[2], (int)p[3]};
  };
  struct Rows { v4i e[NPL]; };
  auto enter = [&](int d) {
    Rows r;
#pragma unroll
    for (int p = 0; p < NPL; p++) r.e[p] = *(const v4i *)(eb - 32 * d + p * PI_IMG);
    return r;
  };
  const v16i zero = {0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0};
  v4i A[NPL];
  const v4i w0 = frag(0);
  v4i w_a = frag(1), w_b;
  Rows e_a = enter(1), e_b;
#pragma unroll
  for (int p = 0; p < NPL; p++) {
    C[p] = __builtin_amdgcn_mfma_i32_32x32x32_i8(F[p], w0, zero, 0, 0, 0);
    A[p] = F[p];
  }
  auto trip = [&](const v4i &w, const Rows &e) {
#pragma unroll
    for (int p = 0; p < NPL; p++) {
      A[p] = rows_up_enter(A[p], e.e[p]);
      C[p] = __builtin_amdgcn_mfma_i32_32x32x32_i8(A[p], w, C[p], 0, 0, 0);
      __builtin_amdgcn_sched_barrier(0);
    }
  };
  auto last = [&](const v4i &w, const Rows &e) {           // distance NT - 1: rows <= NT - 2 lose their bytes 16 hh + j < P
#pragma unroll
    for (int p = 0; p < NPL; p++) {
      A[p] = and4(rows_up_enter(A[p], e.e[p]), keep);
      C[p] = __builtin_amdgcn_mfma_i32_32x32x32_i8(A[p], w, C[p], 0, 0, 0);
    }
  };
  int j = 1;
  for (; j + 1 <= NT - 2; j += 2) {
    w_b = frag(j + 1); e_b = enter(j + 1);
    trip(w_a, e_a);
    w_a = frag(j + 2); e_a = enter(j + 2);
    trip(w_b, e_b);
  }
  if (j <= NT - 2) {
    w_b = frag(j + 1); e_b = enter(j + 1);
    trip(w_a, e_a);
    last(w_b, e_b);
  } else {
    last(w_a, e_a);
  }
}

// verifyKeysInputs (index.js:141-197) for one key pair per wave, ALL THREE products in one pass over the tile distances.
// Lane (r, hh) = 32 hh + r holds chunk ch = 2 r + hh (16 coefficients) of every operand row -- the layout the matrix instruction
// wants its A operand in -- so the rows go from HBM to the matrix cores through registers only.  Product 3 is taken as
// p (fq * g): ((p fq) mod q) * g = p (fq * g) modulo q for the low and the high half alike, so its rows are the SAME two digit
// planes of fq that product 1 multiplies, and the factor p goes into its epilogue.  The three planes (fq lo, fq hi, fp mod 3)
// are shifted once per distance and direction and meet the fragments of BOTH reversed arrays (f: products 1 and 2; g: product 3):
// ten matrix instructions per trip for 24 lane-shift instructions (two loops took 40), one set of planes, one loop prologue, fq
// read once.  Five accumulator pairs = 160 registers: two waves per SIMD.  Same device: 2.12-2.13 ms per 2^18 against 2.18-2.20 ms for
// the two-loop form at three waves per SIMD (products 1 + 2, then product 3 with its own planes), 2.09 against 2.18 J per launch.
struct PiPlanVerify {                 // streams: f, g; accumulators 0, 1 = fq * f; 2, 3 = fq * g; 4 = fp * f
  static constexpr int streams = 2, terms = 5;
  static constexpr PiTerm term(int t) { return t < 4 ? PiTerm{t >> 1, t & 1, (t >> 1) + 2 * (t & 1), t >> 1} : PiTerm{2, 0, 4, 2}; }
};
__global__ __launch_bounds__(64 * PI_WAVES) __attribute__((amdgpu_waves_per_eu(2, 2))) void k_verify_keys_m(
    PGeom g, u32 q, const int8_t *__restrict__ f, const int8_t *__restrict__ gg, const u16 *__restrict__ fq,
    const uint8_t *__restrict__ fp, const u16 *__restrict__ h, long B, u16 *__restrict__ quot_fq,
    u16 *__restrict__ rem_fq, uint8_t *__restrict__ quot_fp, uint8_t *__restrict__ rem_fp, u16 *__restrict__ quot_h,
    u16 *__restrict__ rem_h, uint8_t *__restrict__ flags) {
  extern __shared__ __attribute__((aligned(16))) unsigned char lds[];
  const int lane = threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  unsigned char *nat = lds + (size_t)wave * pi_wave_bytes(g, 2);
  u32 *Tf = (u32 *)(nat + pi_nat_bytes(g)), *Tg = Tf + 4 * g.tpitch;
  const int N = g.N, NT = g.NT;
  const long item_step = (long)gridDim.x * PI_WAVES;
  // An item's operand rows are requested at the end of the PREVIOUS item's last epilogue (PiRow).
  PiRow<2> r_fq;
  PiRow<1> r_f, r_fp, r_g;
  auto request_rows = [&](long it) {
    const int ch = pi_chunk_of(opaque(lane));
    r_fq.request(fq, it, N, ch); r_f.request(f, it, N, ch); r_g.request(gg, it, N, ch); r_fp.request(fp, it, N, ch);
  };
  if ((long)blockIdx.x * PI_WAVES + wave < B) request_rows((long)blockIdx.x * PI_WAVES + wave);
  [[maybe_unused]] int stamp_iter = -1;                    // -DNTRU_STAMPS: phase stamps of the first items (tools/phase_stamps_peritem.py)
  for (long item = (long)blockIdx.x * PI_WAVES + wave; item < B; item += item_step) {
    const long row = item * N;
    u32 fl = 0;
    stamp_iter++;
    STAMP(0);
    // ---- operands: the reversed arrays of f and g, the planes fq lo / fq hi / fp mod 3 (index.js:155-166)
    v4i F[3];
    {
      const int ch = pi_chunk_of(opaque(lane));
      const v4i cmask = col_mask16(16 * ch, N);            // bytes of this lane's chunk that are below N
      pi_build_array_ch(nat, Tf, g, lane, ch, pi_ternary(r_f.bytes(f + row), cmask));
      pi_build_array_ch(nat, Tg, g, lane, ch, pi_ternary(r_g.bytes(gg + row), cmask));
      STAMP(1);                                            // the two reversed arrays
      u32 xq[8];
      r_fq.pairs(fq + row, xq);
      pi_digits(xq, q, 1u, 16 * ch, N, F[0], F[1]);
      F[2] = pi_mod3_bytes(r_fp.bytes(fp + row) & cmask);  // fp mod 3 as the third plane
    }
    // h is requested before the loop whose remainder it is compared with, as a natural-order row chunk (16 coefficients per lane);
    // the remainder gets into the same layout through the wave's LDS (the natural-order area is free again by then)
    PiRow<2> r_h;
    r_h.request(h, item, N, opaque(lane));
    STAMP(2);                                              // the three planes in registers
    // ---- the loop: L1 / H1 (two planes) = fq * f, L3 / H3 (two planes) = fq * g, L2 / H2 = fp * f: every shifted plane of fq feeds two
    // matrix instructions, the fp plane one
    v16i L[5], H[5];
    pi_product_plan<PiPlanVerify>(F, Tf, g, lane, L, H);
    const v16i *const L1 = L, *const H1 = H, *const L3 = L + 2, *const H3 = H + 2, &L2 = L[4], &H2 = H[4];
    STAMP(3);                                              // the matrix loop
    const int kl = pi_index_of(opaque(lane));
    {
      // stores through one-row descriptors: index k = 32 kb + r is a per-lane offset (128 hh + r) plus a compile-time
      // one per register, indices >= N fall outside the descriptor and are dropped -- no address arithmetic per store
      const __amdgpu_buffer_rsrc_t rs_r = rows_rsrc(rem_fq + row, 2L * N), rs_q = rows_rsrc(quot_fq + row, 2L * N);
      PiNotOne rem;                                        // index.js:159
      pi_for_split<2>(L1, H1, [&](int i, int ko, u32 lo, u32 hi) {
        const u32 rv = (lo + hi) & (q - 1);
        __builtin_amdgcn_raw_buffer_store_b16((u16)rv, rs_r, 2 * kl, 2 * ko, 0);
        __builtin_amdgcn_raw_buffer_store_b16((u16)((0u - hi) & (q - 1)), rs_q, 2 * kl, 2 * ko, 0);
        rem.see(i, ko, kl, N, rv);
      });
      if (rem.invalid(kl)) fl |= NTRU_FLAG_INVALID_FQ;
    }
    STAMP(4);                                              // product 1's epilogue
    {
      const __amdgpu_buffer_rsrc_t rs_r = rows_rsrc(rem_fp + row, (long)N), rs_q = rows_rsrc(quot_fp + row, (long)N);
      PiNotOne rem;                                        // as for product 1
#pragma unroll
      for (int i = 0; i < 16; i++) {
        const int ko = pi_ko(i);
        // |L + H|, |H| <= 127 N (f is an int8, fp < 3): a multiple of 3 above that keeps the dividend non-negative
        const u32 x = (u32)(L2[i] + H2[i] + 3 * 131072), y = (u32)(3 * 131072 - H2[i]);
        const u32 rv = x % 3u, qv = y % 3u;
        __builtin_amdgcn_raw_buffer_store_b8((uint8_t)rv, rs_r, kl, ko, 0);
        __builtin_amdgcn_raw_buffer_store_b8((uint8_t)qv, rs_q, kl, ko, 0);
        rem.see(i, ko, kl, N, rv);
      }
      if (rem.invalid(kl)) fl |= NTRU_FLAG_INVALID_FP;
    }
    STAMP(5);                                              // product 2's epilogue
    {
      // product 3 = p (fq * g) mod q (index.js:155,164): the factor p = 3 is applied here, to the low and the high half alike
      const __amdgpu_buffer_rsrc_t rs_r = rows_rsrc(rem_h + row, 2L * N), rs_q = rows_rsrc(quot_h + row, 2L * N);
      u16 *remx = (u16 *)nat;
      pi_for_split<2>(L3, H3, [&](int, int ko, u32 lo, u32 hi) {
        const u32 rv = (3u * (lo + hi)) & (q - 1);
        __builtin_amdgcn_raw_buffer_store_b16((u16)rv, rs_r, 2 * kl, 2 * ko, 0);
        __builtin_amdgcn_raw_buffer_store_b16((u16)((0u - 3u * hi) & (q - 1)), rs_q, 2 * kl, 2 * ko, 0);
        remx[ko + kl] = (u16)rv;                           // ko + kl <= 1151: inside the area for every N (pi_nat_bytes)
      });
      if (item + item_step < B) request_rows(item + item_step);   // the next item's rows: in flight from here on (the accumulators are dead)
      wave_lds_fence();
      STAMP(6);                                            // product 3's result stores issued
      // index.js:165: h[k] must equal the remainder for every k below h's trimmed length
      v4i hc[2];
      r_h.take(h + row, hc);
      const int i0 = 16 * opaque(lane);
      // Per lane two 16-bit sets in a SPLIT layout (coefficient i0 + 2 c in bit c, i0 + 2 c + 1 in bit 16 + c: what one packed
      // 16-bit minimum and one shift-or per dword give): nz = h is non-zero there, df = h differs from the remainder there;
      // coefficients at and beyond N are cut off the sets, not off the data.  h is invalid iff its FIRST difference from the
      // remainder lies at or below its LAST non-zero coefficient (index.js:165 compares below h's trimmed length); both are
      // found on the scalar side from one ballot and one v_readlane each.
      u32 nz = 0, df = 0;
      if (i0 < 32 * NT) {
        const v4i rc0 = *(const v4i *)(nat + 2 * i0), rc1 = *(const v4i *)(nat + 2 * i0 + 16);
#pragma unroll
        for (int c = 0; c < 8; c++) {
          const u32 hx = (u32)(c < 4 ? hc[0][c] : hc[1][c - 4]), rx = (u32)(c < 4 ? rc0[c] : rc1[c - 4]);
          nz |= as_u32(__builtin_elementwise_min(as_pair(hx), (u16x2){1, 1})) << c;
          df |= as_u32(__builtin_elementwise_min(as_pair(hx ^ rx), (u16x2){1, 1})) << c;
        }
        const int left = N - i0;                           // coefficients of this lane's chunk that exist
        const u32 ne = left >= 16 ? 0xFFu : (1u << ((left + 1) >> 1)) - 1u, no = left >= 16 ? 0xFFu : (1u << (left >> 1)) - 1u;
        const u32 valid = left <= 0 ? 0u : (ne | no << 16);
        nz &= valid; df &= valid;
      }
      auto last_of = [](u32 m) {                           // highest coefficient (0..15) of a non-empty split set
        const u32 ev = m & 0xFFFFu, od = m >> 16;
        const int te = ev ? 2 * (31 - __builtin_clz(ev)) : -1, to = od ? 2 * (31 - __builtin_clz(od)) + 1 : -1;
        return te > to ? te : to;
      };
      auto first_of = [](u32 m) {                          // lowest coefficient of a non-empty split set
        const u32 ev = m & 0xFFFFu, od = m >> 16;
        const int fe = ev ? 2 * __builtin_ctz(ev) : 64, fo = od ? 2 * __builtin_ctz(od) + 1 : 64;
        return fe < fo ? fe : fo;
      };
      const unsigned long long has = __ballot(nz != 0), dif = __ballot(df != 0);
      if (dif) {
        const int lf = __builtin_ctzll(dif);
        const int first_diff = 16 * lf + first_of((u32)__builtin_amdgcn_readlane((int)df, lf));
        int top = 0;                                       // the zero polynomial has trimmed length 1: index 0 is compared
        if (has) {
          const int lt = 63 - __builtin_clzll(has);
          top = 16 * lt + last_of((u32)__builtin_amdgcn_readlane((int)nz, lt));
        }
        if (first_diff <= top) fl |= NTRU_FLAG_INVALID_H;
      }
    }
    if (lane == 0) flags[item] = (uint8_t)fl;
    wave_lds_fence();
    STAMP(7);                                              // the comparison with h
  }
}

// One per-item product on the matrix cores: ((mul a) mod q) * s modulo x^N - 1 and q, a < 2^16 per item, s ternary per item:
// generatePublicKeyH (index.js:72-79, mul = p), whose quotient nobody asks for: pi_product_cyc, one matrix instruction per tile
// distance and digit plane.  ONE: a single int8 digit plane (q <= 256).
template <bool ONE>
__global__ __launch_bounds__(64 * PI_WAVES) __attribute__((amdgpu_waves_per_eu(ONE ? 4 : 3, 4))) void k_product_tern_m(
    PGeom g, u32 q, u32 mul, const u16 *__restrict__ a, const int8_t *__restrict__ s, long B, u16 *__restrict__ rem) {
  extern __shared__ __attribute__((aligned(16))) unsigned char lds[];
  constexpr int NPL = ONE ? 1 : 2;
  const int lane = threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  unsigned char *nat = lds + (size_t)wave * pi_wave_bytes(g, 1);
  u32 *T = (u32 *)(nat + pi_nat_bytes(g));
  const int N = g.N;
  // The operands of the NEXT item are requested as soon as this item's are in registers (the round trip to HBM runs under the matrix
  // loops and the result stores instead of in front of every item).
  const long item_step = (long)gridDim.x * PI_WAVES;
  PiRow<2> ra;
  PiRow<1> rs;
  auto request = [&](long it) {
    const int ch = pi_chunk_of(opaque(lane));
    ra.request(a, it, N, ch); rs.request(s, it, N, ch);
  };
  if ((long)blockIdx.x * PI_WAVES + wave < B) request((long)blockIdx.x * PI_WAVES + wave);
  for (long item = (long)blockIdx.x * PI_WAVES + wave; item < B; item += item_step) {
    const long row = item * N;
    v4i F[NPL];
    {
      const int ch = pi_chunk_of(opaque(lane));
      u32 xa[8];
      ra.pairs(a + row, xa);
      const v4i vs = rs.bytes(s + row);
      if (item + item_step < B) request(item + item_step);
      pi_build_array_half(nat, T, g, lane, ch, pi_ternary(vs, col_mask16(16 * ch, N)));     // (its last fence: nat is free for the planes' images)
      v4i o0, o1;
      pi_digits(xa, q, mul, 16 * ch, N, o0, o1);
      F[0] = o0;
      pi_store_image(nat, g, ch, o0);
      if (!ONE) { F[NPL - 1] = o1; pi_store_image(nat + PI_IMG, g, ch, o1); }
      wave_lds_fence();
    }
    v16i C[NPL];
    u32 keep[4];
    pi_cyc_keep(g, lane, keep);
    pi_product_cyc<NPL>(F, nat, T, g, lane, keep, C);
    {
      const int kl = pi_index_of(opaque(lane));     // see k_verify_keys_m: indices >= N are dropped
      const __amdgpu_buffer_rsrc_t rs_r = rows_rsrc(rem + row, 2L * N);
#pragma unroll
      for (int i = 0; i < 16; i++) {
        const int ko = pi_ko(i);
        const int c = C[0][i] + (ONE ? 0 : 128 * C[NPL - 1][i]);
        __builtin_amdgcn_raw_buffer_store_b16((u16)((u32)c & (q - 1)), rs_r, 2 * kl, 2 * ko, 0);
      }
    }
    wave_lds_fence();
  }
}

// One Newton round of the key inversion (polyInv, index.js:499-506) per item in ONE kernel, in its lifted form: v is right modulo
// 2^kb (kb <= 7 bits, the schedule of ntru_invert_key_batch_dev), f v = 1 + 2^kb e, and v <- v - 2^kb (e v mod 2^(m - kb)) is right
// modulo 2^m, m <= 2 kb.  Both products run on one int8 digit plane with the chunk rows in registers: f (x) v with f's reversed
// array and v (< 128) as the rows; then e -- at most kb bits per coefficient -- goes from the accumulator layout through a
// natural-order byte image in the LDS into the row layout (ONE read per lane), v's residues modulo 2^(m - kb) become the reversed
// array in f's place, and the second product's epilogue lifts v on the item's own row.
__global__ __launch_bounds__(64 * PI_WAVES) __attribute__((amdgpu_waves_per_eu(4, 4))) void k_newton_round_m(
    PGeom g, u32 kb, u32 m, const int8_t *__restrict__ f, u16 *v, long B) {
  extern __shared__ __attribute__((aligned(16))) unsigned char lds[];
  const int lane = threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  unsigned char *nat = lds + (size_t)wave * pi_wave_bytes(g, 1);
  u32 *T = (u32 *)(nat + pi_nat_bytes(g));
  const int N = g.N;
  const u32 mr = 1u << m, me = 1u << (m - kb);
  const long item_step = (long)gridDim.x * PI_WAVES;
  PiRow<2> rv;
  PiRow<1> rf;
  auto request = [&](long it) {
    const int ch = pi_chunk_of(opaque(lane));
    rv.request(v, it, N, ch); rf.request(f, it, N, ch);
  };
  if ((long)blockIdx.x * PI_WAVES + wave < B) request((long)blockIdx.x * PI_WAVES + wave);
  [[maybe_unused]] int stamp_iter = -1;                    // -DNTRU_STAMPS: phase stamps of the first items (tools/phase_stamps_peritem.py)
  for (long item = (long)blockIdx.x * PI_WAVES + wave; item < B; item += item_step) {
    const long row = item * N;
    stamp_iter++;
    STAMP(0);
    v4i b0;                                                // v modulo 2^(m - kb), centred: the second product's Toeplitz operand
    v4i F[1];
    {
      const int ch = pi_chunk_of(opaque(lane));
      u32 xv[8];
      rv.pairs(v + row, xv);
      const v4i vf = rf.bytes(f + row);
      v4i o1;
      pi_digits(xv, me, 1u, 16 * ch, N, b0, o1);
      pi_digits(xv, 256u, 1u, 16 * ch, N, F[0], o1);      // v < 2^kb <= 128: its own centred representative modulo 256
      STAMP(1);                                            // operands arrived, digits
      // f by its VALUE, as k_invert_key reduced it modulo 2 (not ValTernary's "any negative byte is -1": the round would start from
      // the inverse of another polynomial); |f v| <= 1024 * 128 * 127 < 2^31 per coefficient
      pi_build_array_half(nat, T, g, lane, ch, vf & col_mask16(16 * ch, N));                     // (its last fence: nat is free for v's image)
      pi_store_image(nat, g, ch, F[0]);
      wave_lds_fence();
    }
    STAMP(2);                                              // f's reversed array, v's image
    v16i C[1];
    u32 keep[4];
    pi_cyc_keep(g, lane, keep);
    pi_product_cyc<1>(F, nat, T, g, lane, keep, C);        // f v
    STAMP(3);
    if (item + item_step < B) request(item + item_step);   // the next item's rows (nobody lifts them before this wave does): a product ahead
    {
      const int ln = opaque(lane), kl = pi_index_of(ln), ch = pi_chunk_of(ln);
      u32 e[16];                                           // e = (f v - 1) / 2^kb modulo 2^(m - kb): bits kb .. m - 1 of f v - 1
#pragma unroll
      for (int i = 0; i < 16; i++)
        e[i] = __builtin_amdgcn_ubfe((u32)C[0][i] - (i == 0 && kl == 0 ? 1u : 0u), kb, m - kb);
      pi_build_array_half(nat, T, g, lane, ch, b0);          // (over f's array; its last fence orders the reads of nat before the writes below)
      unsigned char *img = nat + (32 * g.NT - N);          // e's image for the entering rows IS its natural-order byte image, P bytes up
#pragma unroll
      for (int i = 0; i < 16; i++) img[pi_ko(i) + kl] = (unsigned char)e[i];     // index <= 1023 + 31
      wave_lds_fence();
      F[0] = *(const v4i *)(img + 16 * ch) & col_mask16(16 * ch, N);       // (any alignment; bytes at and beyond N: whatever the product left there)
    }
    // v in the accumulator layout, for the lift (the row this item staged a moment ago: an L2 hit), in flight during the second product
    const __amdgpu_buffer_rsrc_t rs_v = rows_rsrc(v + row, 2L * N);
    const int kl2 = pi_index_of(opaque(lane));
    u16 vold[16];
#pragma unroll
    for (int i = 0; i < 16; i++) vold[i] = (u16)__builtin_amdgcn_raw_buffer_load_b16(rs_v, 2 * kl2, 2 * pi_ko(i), 0);
    STAMP(4);                                              // e, v's reversed array, e's image and rows
    pi_product_cyc<1>(F, nat, T, g, lane, keep, C);        // e v
    STAMP(5);
#pragma unroll
    for (int i = 0; i < 16; i++) {
      const int ko = pi_ko(i);
      u32 nv;                                              // vold - 2^kb (e v): of e v only its residue modulo 2^(m - kb) reaches the low m bits
      asm("v_mad_i32_i24 %0, %1, %2, %3" : "=v"(nv) : "v"(C[0][i]), "s"(0 - (int)(1u << kb)), "v"(vold[i]));   // |e v| < 2^23; vold's upper half: masked below
      __builtin_amdgcn_raw_buffer_store_b16((u16)(nv & (mr - 1)), rs_v, 2 * kl2, 2 * ko, 0);
    }
    wave_lds_fence();
    STAMP(6);                                              // the lift's stores issued
  }
}

// Generic per-item product on the matrix cores: both operands < q <= 8192 (multiplyPolynomials + dividePolynomials by I,
// index.js:319-401, with q a power of two).  With a = a0 + 128 a1 and b = b0 + 128 b1 the product is
// a0 b0 + 128 (a0 b1 + a1 b0) + 16384 a1 b1, and 16384 = 0 mod q: three plane products, two accumulator groups, two reversed arrays
// (the digit planes of b) per item, the rows of a0 and a1 in registers.
// ONE (q <= 256): one digit plane per operand.
template <bool ONE>
__global__ __launch_bounds__(64 * PI_WAVES) __attribute__((amdgpu_waves_per_eu(ONE ? 4 : 3, 4))) void k_polymul_m(
    PGeom g, u32 q, const u16 *__restrict__ a, const u16 *__restrict__ b, long B, u16 *__restrict__ quot, u16 *__restrict__ rem) {
  extern __shared__ __attribute__((aligned(16))) unsigned char lds[];
  const int lane = threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  unsigned char *nat = lds + (size_t)wave * pi_wave_bytes(g, ONE ? 1 : 2);
  u32 *T0 = (u32 *)(nat + pi_nat_bytes(g)), *T1 = T0 + 4 * g.tpitch;
  const int N = g.N, NT = g.NT;
  const bool want_q = quot != nullptr;
  const long item_step = (long)gridDim.x * PI_WAVES;         // the NEXT item's operands are requested early: see k_product_tern_m
  PiRow<2> rwa, rwb;
  auto request = [&](long it) {
    const int ch = pi_chunk_of(opaque(lane));
    rwa.request(a, it, N, ch); rwb.request(b, it, N, ch);
  };
  if ((long)blockIdx.x * PI_WAVES + wave < B) request((long)blockIdx.x * PI_WAVES + wave);
  [[maybe_unused]] int stamp_iter = -1;                    // -DNTRU_STAMPS: phase stamps of the first items (tools/phase_stamps_peritem.py)
  for (long item = (long)blockIdx.x * PI_WAVES + wave; item < B; item += item_step) {
    const long row = item * N;
    stamp_iter++;
    STAMP(0);
    v4i a0, a1;
    {
      const int ch = pi_chunk_of(opaque(lane));
      u32 xa[8], xb[8];
      rwa.pairs(a + row, xa);
      rwb.pairs(b + row, xb);
      STAMP(1);                                            // operands arrived
      if (item + item_step < B) request(item + item_step);
      v4i b0, b1;
      pi_digits(xa, q, 1u, 16 * ch, N, a0, a1);
      pi_digits(xb, q, 1u, 16 * ch, N, b0, b1);
      STAMP(2);                                            // digits
      pi_build_array_ch(nat, T0, g, lane, ch, b0);
      if (!ONE) pi_build_array_ch(nat, T1, g, lane, ch, b1);
      STAMP(3);                                            // reversed arrays
    }
    v16i XL[2], XH[2];                                     // group 0: a0 b0; group 1: a0 b1 + a1 b0
    if (ONE) {
      v4i F[1] = {a0};
      v16i L[1], H[1];
      pi_product_reg<1>(F, T0, g, lane, L, H);
      XL[0] = L[0]; XH[0] = H[0];
#pragma unroll
      for (int i = 0; i < 16; i++) { XL[1][i] = 0; XH[1][i] = 0; }
    } else {
      // as pi_product_plan, with the terms (a0, b0, X0) behind plane 0 and (a0, b1, X1), (a1, b0, X1) behind plane 1: written out, because
      // the plan form takes 142 registers here where this takes 140
      const int ln = opaque(lane);
      const int y0 = 32 * NT - 1 - (ln & 31) + 16 * (ln >> 5);
      const u32 *tb = T0 + (y0 & 3) * g.tpitch + (y0 >> 2);
      const int tstep = 4 * g.tpitch;                      // dwords from a fragment of b0 to the same fragment of b1
      int seam_up = ln == 32 ? 0 : -1, seam_dn = ln == 31 ? 0 : -1;
      asm volatile("" : "+v"(seam_up), "+v"(seam_dn));
      struct Fr { v4i w0, w1; };
      auto frag = [&](int d) {
        d = d > NT - 1 ? NT - 1 : (d < 1 - NT ? 1 - NT : d);
        const u32 *p = tb - 8 * d, *p1 = p + tstep;
        Fr fr;
        fr.w0 = (v4i){(int)p[0], (int)p[1], (int)p[2], (int)p[3]};
        fr.w1 = (v4i){(int)p1[0], (int)p1[1], (int)p1[2], (int)p1[3]};
        return fr;
      };
      const v16i zero = {0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0};
      const Fr f0 = frag(0);
      Fr la = frag(1), ha = frag(-1), lb, hb;
      {
        u32 mlow[4], mhigh[4];
        pi_diag_low_mask(ln, mlow);
#pragma unroll
        for (int c = 0; c < 4; c++) mhigh[c] = ~mlow[c];
        XL[0] = __builtin_amdgcn_mfma_i32_32x32x32_i8(a0, and4(f0.w0, mlow), zero, 0, 0, 0);
        XL[1] = __builtin_amdgcn_mfma_i32_32x32x32_i8(a0, and4(f0.w1, mlow), zero, 0, 0, 0);
        XL[1] = __builtin_amdgcn_mfma_i32_32x32x32_i8(a1, and4(f0.w0, mlow), XL[1], 0, 0, 0);
        XH[0] = __builtin_amdgcn_mfma_i32_32x32x32_i8(a0, and4(f0.w0, mhigh), zero, 0, 0, 0);
        XH[1] = __builtin_amdgcn_mfma_i32_32x32x32_i8(a0, and4(f0.w1, mhigh), zero, 0, 0, 0);
        XH[1] = __builtin_amdgcn_mfma_i32_32x32x32_i8(a1, and4(f0.w0, mhigh), XH[1], 0, 0, 0);
      }
      v4i AL0 = a0, AL1 = a1, AH0 = a0, AH1 = a1;
      auto trip = [&](const Fr &wl, const Fr &wh) {
        AL0 = rows_up(AL0, seam_up);
        XL[0] = __builtin_amdgcn_mfma_i32_32x32x32_i8(AL0, wl.w0, XL[0], 0, 0, 0);
        __builtin_amdgcn_sched_barrier(0);
        AL1 = rows_up(AL1, seam_up);
        XL[1] = __builtin_amdgcn_mfma_i32_32x32x32_i8(AL0, wl.w1, XL[1], 0, 0, 0);
        XL[1] = __builtin_amdgcn_mfma_i32_32x32x32_i8(AL1, wl.w0, XL[1], 0, 0, 0);
        __builtin_amdgcn_sched_barrier(0);
        AH0 = rows_down(AH0, seam_dn);
        XH[0] = __builtin_amdgcn_mfma_i32_32x32x32_i8(AH0, wh.w0, XH[0], 0, 0, 0);
        __builtin_amdgcn_sched_barrier(0);
        AH1 = rows_down(AH1, seam_dn);
        XH[1] = __builtin_amdgcn_mfma_i32_32x32x32_i8(AH0, wh.w1, XH[1], 0, 0, 0);
        XH[1] = __builtin_amdgcn_mfma_i32_32x32x32_i8(AH1, wh.w0, XH[1], 0, 0, 0);
        __builtin_amdgcn_sched_barrier(0);
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
    STAMP(4);                                              // matrix loops
    {
      const int kl = pi_index_of(opaque(lane));     // see k_verify_keys_m: indices >= N are dropped
      const __amdgpu_buffer_rsrc_t rs_r = rows_rsrc(rem + row, 2L * N);
      const __amdgpu_buffer_rsrc_t rs_q = rows_rsrc(want_q ? quot + row : nullptr, want_q ? 2L * N : 0L);
      pi_for_split<2>(XL, XH, [&](int, int ko, u32 lo, u32 hi) {
        __builtin_amdgcn_raw_buffer_store_b16((u16)((lo + hi) & (q - 1)), rs_r, 2 * kl, 2 * ko, 0);
        if (want_q) __builtin_amdgcn_raw_buffer_store_b16((u16)((0u - hi) & (q - 1)), rs_q, 2 * kl, 2 * ko, 0);
      });
    }
    wave_lds_fence();
    STAMP(5);                                              // result stores issued
  }
}
NTRU_STAMPS_READER(ntru_debug_read_stamps_pi)

// ---- host side ----------------------------------------------------------------------------------------------------------
int ntru_launch_polymul_matrix(ntru_engine *eng, int N, int mod, const uint16_t *d_a, const uint16_t *d_b, int64_t B, uint16_t *d_quot,
                               uint16_t *d_rem) {
  if (!peritem_applies(eng, N, mod)) return NTRU_NOT_TAKEN;
  const PGeom pg = make_pgeom(N);
  const bool one = mod <= 256;
  note_kernel(eng, "k_polymul_m");
  return launch_peritem(eng, one ? k_polymul_m<true> : k_polymul_m<false>, B, pi_wave_bytes(pg, one ? 1 : 2), pg, (u32)mod, d_a, d_b, (long)B,
                        d_quot, d_rem);
}

bool ntru_product_tern_matrix_applies(const ntru_engine *eng, int N, int q) { return peritem_applies(eng, N, q); }

int ntru_launch_product_tern_matrix(ntru_engine *eng, int N, int q, uint32_t mul, const uint16_t *d_a, const int8_t *d_s, long B,
                                    uint16_t *d_rem) {
  const PGeom pg = make_pgeom(N);
  return launch_peritem(eng, q <= 256 ? k_product_tern_m<true> : k_product_tern_m<false>, B, pi_wave_bytes(pg, 1), pg, (u32)q, (u32)mul, d_a,
                        d_s, B, d_rem);
}

int ntru_launch_verify_keys_matrix(ntru_engine *eng, int N, int q, int p, const int8_t *d_f, const int8_t *d_g, const uint16_t *d_fq,
                                   const uint8_t *d_fp, const uint16_t *d_h, int64_t B, uint16_t *d_quot_fq, uint16_t *d_rem_fq,
                                   uint8_t *d_quot_fp, uint8_t *d_rem_fp, uint16_t *d_quot_h, uint16_t *d_rem_h, uint8_t *d_flags) {
  if (p != 3 || !peritem_applies(eng, N, q)) return NTRU_NOT_TAKEN;
  const PGeom pg = make_pgeom(N);
  note_kernel(eng, "k_verify_keys_m");
  return launch_peritem(eng, k_verify_keys_m, B, pi_wave_bytes(pg, 2), pg, (u32)q, d_f, d_g, d_fq, d_fp, d_h, (long)B, d_quot_fq, d_rem_fq,
                        d_quot_fp, d_rem_fp, d_quot_h, d_rem_h, d_flags);
}


// One Newton round (v from kb to m bits) of the key inversion as ONE kernel: kb <= 7 (v below 128: one digit plane), per-item matrix path.
bool ntru_newton_round_matrix_applies(const ntru_engine *eng, int N, int kb, int m) {
  return kb <= 7 && m <= 2 * kb && m > kb && peritem_applies(eng, N, 1 << m);
}
int ntru_launch_newton_round_matrix(ntru_engine *eng, int N, int kb, int m, const int8_t *d_f, uint16_t *d_v, long B) {
  if (!ntru_newton_round_matrix_applies(eng, N, kb, m)) return NTRU_NOT_TAKEN;
  const PGeom pg = make_pgeom(N);
  return launch_peritem(eng, k_newton_round_m, B, pi_wave_bytes(pg, 1), pg, (u32)kb, (u32)m, d_f, d_v, B);
}

#ifdef NTRU_STAMPS
// (diagnostic build only: one Newton round as its own call, for tools/phase_stamps_peritem.py)
extern "C" int ntru_debug_newton_round(ntru_engine *eng, int N, int kb, int m, const int8_t *d_f, uint16_t *d_v, long B) {
  return ntru_launch_newton_round_matrix(eng, N, kb, m, d_f, d_v, B);
}
#endif
