// matrix_mulshared.hip -- a batch of full-range rows times ONE full-range polynomial, with the split by 1 - x^N: multiplyPolynomials(row, s,
// mod) followed by dividePolynomials(., I, mod) (index.js:319-355, 358-401) with s fixed over the batch: the kernel, the *_dev entry point
// and the host-pointer form.  Row b of quot / rem is byte for byte what ntru_polymul_split returns for (rows[b], s).
//
// k_mul_shared_m (power-of-two mod <= 8192, N <= 1024, kernel paths 0, 4, 5): batch x Toeplitz matrix of s on v_mfma_i32_32x32x32_i8,
// exact, with the geometry of matrix_common.h (32-row blocks, four waves, strips of <= 4 column tiles, reversed cyclic key arrays).
// Neither operand fits an int8, so both are split at 128:
//     e = e_lo + 128 e_hi     e_lo = e & 127 in [0, 127],              e_hi = e >> 7 in [0, 63]        (the stages of k_decrypt_m)
//     s = s0   + 128 s1       s0 = ((s + 64) & 127) - 64 in [-64, 63], s1 = ((s - s0) >> 7) & 63
//     e s = e_lo s0 + 64 (e_lo (2 s1) + (2 e_hi) s0)        (mod q)
// 2^14 e_hi s1 vanishes modulo every q of the range, and s1 may be taken modulo 64 because 128 . 64 = 8192 does.  Every plane is an
// int8 (2 s1 <= 126, 2 e_hi <= 126), every partial sum stays far inside an int32 (at most 1024 (127 . 126 + 126 . 64)), and the factor
// 64 may wrap because q divides 2^32.  Three plane products per contraction step, as many as decrypt's two products together.
// The two partial sums share ONE set of accumulators: pass B runs e_lo (2 s1) + (2 e_hi) s0 through the strip's contraction steps,
// its sums are shifted left by 6 in place, and pass A adds e_lo s0 on top (two sets of 4-tile accumulators would be 256 registers and
// leave nothing beside two workgroups per CU).  The epilogue is that of k_decrypt_m's product 1 without the lift:
// rem = (low + high) & (q - 1), quot = (-high) & (q - 1).  tools/mfma_model.py (mul_shared_*) is the executable specification.
//
// Everything else -- mod > 8192, a modulus that is no power of two, N > 1024, kernel paths 1-3 -- replicates s into the engine-owned
// scratch and runs the per-item product kernels of ntru_polymul_split_dev on it, in passes of at most 65536 rows: correct, not fast.
#include "matrix_common.h"

namespace {

constexpr int MS_RADIX = 128;                // both operands are split at 128
constexpr int MS_HALF = 64;                  // s0 lies in [-64, 63]; the doubled planes make pass B count 64-fold
constexpr u32 MS_S1_MASK = 0x3F;             // s1 modulo 64: 128 . 64 = 8192 vanishes
constexpr int MS_CARRY_SHIFT = 6;            // log2(MS_HALF): pass B's sums, shifted, are what pass A accumulates onto
constexpr int64_t MS_FALLBACK_PASS = 65536;  // rows per pass of the replicated path
static_assert(MS_RADIX == 2 * MS_HALF && (1 << MS_CARRY_SHIFT) == MS_HALF && MS_RADIX * (int)(MS_S1_MASK + 1) == 8192, "one split");

__device__ __forceinline__ int ms_s0(u32 s) { return (int)((s + MS_HALF) & (MS_RADIX - 1)) - MS_HALF; }
__device__ __forceinline__ u32 ms_s1x2(u32 s) { return 2u * (((s - (u32)ms_s0(s)) >> 7) & MS_S1_MASK); }

// One strip of NT_S column tiles from tile kb0 on, all 32 rows of the staged row block, all g.NT contraction steps, twice: pass B into
// zeroed accumulators, the shift, pass A on top.  stLo / stHi: this lane's row of the e_lo / 2 e_hi stage (+ 16 bytes for the upper
// half-wave); tb0 / tb1: this lane's fragment bases in the key arrays of s0 / 2 s1.  The fragment window works as in toeplitz_strip:
// NT_S slots, sub-step u of a block of NT_S steps has tile t on slot (t - u) mod NT_S, and the fragment needed next replaces the one
// the last tile just used.  Steps above the strip's diagonal (ib < kb0) add into `low`, steps below it into `high`, and the diagonal
// block splits its own tile by mlow.  This loop is plainer than toeplitz_strip's (accumulators zeroed, leading steps without a window).
template <int NT_S, class Epi>
__device__ __forceinline__ void mul_shared_strip(const unsigned char *__restrict__ stLo, const unsigned char *__restrict__ stHi,
                                                 const u32 *__restrict__ tb0, const u32 *__restrict__ tb1, const MGeom &g, int kb0,
                                                 const u32 (&mlow)[4], Epi epi) {
  v16i accL[NT_S], accH[NT_S];
#pragma unroll
  for (int t = 0; t < NT_S; t++)
#pragma unroll
    for (int i = 0; i < 16; i++) { accL[t][i] = 0; accH[t][i] = 0; }
  u32 mhigh[4];
#pragma unroll
  for (int c = 0; c < 4; c++) mhigh[c] = ~mlow[c];
  auto frag = [](const u32 *tb, int d) {
    const u32 *p = tb - 8 * d;
    return (v4i){(int)p[0], (int)p[1], (int)p[2], (int)p[3]};
  };
  // acc += stX . Toeplitz(tbX) (+ stY . Toeplitz(tbY) when TWO) over every contraction step
  auto pass = [&](auto two, const unsigned char *stX, const u32 *tbX, const unsigned char *stY, const u32 *tbY) __attribute__((always_inline)) {
    constexpr bool TWO = decltype(two)::value;
    v4i WX[NT_S], WY[NT_S];
    v4i ax = *(const v4i *)stX, ay = TWO ? *(const v4i *)stY : ax;
    auto mm = [&](v16i &acc, v4i wx, v4i wy) {
      acc = __builtin_amdgcn_mfma_i32_32x32x32_i8(ax, wx, acc, 0, 0, 0);
      if (TWO) acc = __builtin_amdgcn_mfma_i32_32x32x32_i8(ay, wy, acc, 0, 0, 0);
    };
    // The blocks are aligned with the diagonal (they start at steps = kb0 mod NT_S), so that which accumulator a tile adds into is
    // known when the block is unrolled.  The kb0 mod NT_S steps in front of the first block (all above the diagonal) run without a
    // window: a fragment per tile and step.
    const int lead = kb0 % NT_S;
    for (int ib = 0; ib < lead; ib++) {
#pragma unroll
      for (int t = 0; t < NT_S; t++) mm(accL[t], frag(tbX, kb0 + t - ib), TWO ? frag(tbY, kb0 + t - ib) : ax);
      ax = *(const v4i *)(stX + 32 * (ib + 1));          // lead < NT_S <= g.NT - kb0: a step of this strip
      if (TWO) ay = *(const v4i *)(stY + 32 * (ib + 1));
    }
#pragma unroll
    for (int t = 0; t < NT_S; t++) {                     // canonical window: slot t holds the fragment of offset kb0 + t - lead
      WX[t] = frag(tbX, kb0 + t - lead);
      WY[t] = TWO ? frag(tbY, kb0 + t - lead) : WX[t];
    }
    // contraction step ib as sub-step u; kind 0: every tile above the diagonal, 1: every tile below, 2: the strip's diagonal block
    auto step = [&](int ib, int u, auto kind) __attribute__((always_inline)) {
      constexpr int K = decltype(kind)::value;
      const int nx = ib + 1 < g.NT ? ib + 1 : ib;        // the last step requests its own operands again: nothing behind the stage is read
      const v4i nax = *(const v4i *)(stX + 32 * nx), nay = TWO ? *(const v4i *)(stY + 32 * nx) : nax;
#pragma unroll
      for (int tt = 1; tt <= NT_S; tt++) {               // tile 0's fragment was requested last: it goes last (see toeplitz_strip)
        const int t = tt % NT_S, sl = (t - u + NT_S) % NT_S;
        if (K == 0 || (K == 2 && t > u)) mm(accL[t], WX[sl], WY[sl]);
        else if (K == 1 || (K == 2 && t < u)) mm(accH[t], WX[sl], WY[sl]);
        else {
          mm(accL[t], and4(WX[sl], mlow), and4(WY[sl], mlow));
          mm(accH[t], and4(WX[sl], mhigh), and4(WY[sl], mhigh));
        }
      }
      WX[(NT_S - 1 - u) % NT_S] = frag(tbX, kb0 - nx);
      if (TWO) WY[(NT_S - 1 - u) % NT_S] = frag(tbY, kb0 - nx);
      ax = nax; ay = nay;
    };
    auto block = [&](int ib, auto kind) __attribute__((always_inline)) {
#pragma unroll
      for (int u = 0; u < NT_S; u++)
        if (decltype(kind)::value != 1 || ib + u < g.NT) step(ib + u, u, kind);   // only the last block below the diagonal may be cut short
    };
    int ib = lead;
    for (; ib < kb0; ib += NT_S) block(ib, std::integral_constant<int, 0>{});
    block(kb0, std::integral_constant<int, 2>{});
    for (ib = kb0 + NT_S; ib < g.NT; ib += NT_S) block(ib, std::integral_constant<int, 1>{});
  };
  pass(std::true_type{}, stLo, tb1, stHi, tb0);          // B: e_lo (2 s1) + (2 e_hi) s0
#pragma unroll
  for (int t = 0; t < NT_S; t++)
#pragma unroll
    for (int i = 0; i < 16; i++) {
      accL[t][i] = (int)((u32)accL[t][i] << MS_CARRY_SHIFT);
      accH[t][i] = (int)((u32)accH[t][i] << MS_CARRY_SHIFT);
    }
  pass(std::false_type{}, stLo, tb0, stLo, tb0);         // A: e_lo s0
  epi(accL, accH);
}

__global__ __launch_bounds__(BLOCK_THREADS, 2) void k_mul_shared_m(MGeom g, u32 q, const u16 *__restrict__ s, const u16 *__restrict__ rows,
                                                                  long B, u16 *__restrict__ quot, u16 *__restrict__ rem) {
  extern __shared__ __attribute__((aligned(16))) unsigned char lds[];
  // LDS: [2 e_hi stage][e_lo stage][key array of s0][key array of 2 s1]
  unsigned char *stHi = lds, *stLo = stHi + 32 * g.pitchA;
  u32 *T0 = (u32 *)(stLo + 32 * g.pitchA), *T1 = T0 + 4 * g.tpitch;
  const int lane0 = threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
  build_toeplitz_array(T0, g, [&](int i) { return ms_s0(s[i] & (q - 1)); }, (int)threadIdx.x, BLOCK_THREADS);
  build_toeplitz_array(T1, g, [&](int i) { return (int)ms_s1x2(s[i] & (q - 1)); }, (int)threadIdx.x, BLOCK_THREADS);
  const bool want_q = quot != nullptr;
  const long nrb = (B + 31) >> 5;
  const int nch = 2 * g.NT;
  const u32 qm2 = (q - 1) * 0x00010001u;
  for (long rb = blockIdx.x; rb < nrb; rb += gridDim.x) {
    // what follows from the lane is made again in every trip (see k_encrypt_m): kept across the trips, the masks and bases cost the
    // strips the registers that keep them free of scratch
    int lane = lane0, N = g.N, LD = g.ld;
    asm volatile("" : "+v"(lane), "+s"(N), "+s"(LD));
    const u32 *tb0 = frag_lane_base(T0, g, lane), *tb1 = frag_lane_base(T1, g, lane);
    const unsigned char *st0 = stLo + (lane & 31) * g.pitchA + 16 * (lane >> 5);
    const unsigned char *st1 = stHi + (lane & 31) * g.pitchA + 16 * (lane >> 5);
    u32 mlow[4];
    diag_low_mask(lane, mlow);
    const int lane_off = (lane >> 5) * 4 * LD + (lane & 31);
    const long b0 = rb << 5, left = (B - b0) * LD;
    const AlignedSrc src = aligned_src(rows + b0 * LD, 2 * left);
    // staging as in decrypt_m_body: a wave takes one row at a time, lane = 16 coefficients read as aligned 16-byte chunks and shifted
    // in registers; rows behind B read as zero
    constexpr int RPW = 32 / WAVES_PER_BLOCK;
    RawChunks<2> raw[RPW];
    int sh[RPW];
    __syncthreads();                                     // the strips of the row block before have read the stages
#pragma unroll
    for (int j = 0; j < RPW; j++) {
      const int pos0 = src.a0 + 2 * (wave + WAVES_PER_BLOCK * j) * LD;
      sh[j] = __builtin_amdgcn_readfirstlane(pos0 & 15);
      raw[j] = load_raw<2>(src, pos0 + 32 * lane, sh[j]);
    }
    u32 cmask[8];                                        // columns >= N of the last chunk(s) are zero; coefficients mod q
#pragma unroll
    for (int c = 0; c < 8; c++) {
      const int left2 = N - (16 * lane + 2 * c);
      cmask[c] = qm2 & (left2 >= 2 ? 0xFFFFFFFFu : (left2 == 1 ? 0x0000FFFFu : 0u));
    }
#pragma unroll
    for (int j = 0; j < RPW; j++) {
      const int row = wave + WAVES_PER_BLOCK * j;
      v4i v[2];                                          // 16 coefficients as u16 pairs
      shift_raw<2>(raw[j], sh[j], v);
      u32 lo[4], hi[4];
#pragma unroll
      for (int c = 0; c < 4; c++) {
        const u32 xa = (u32)v[c >> 1][2 * (c & 1)] & cmask[2 * c], xb = (u32)v[c >> 1][2 * (c & 1) + 1] & cmask[2 * c + 1];
        lo[c] = __builtin_amdgcn_perm(xb & 0x007F007Fu, xa & 0x007F007Fu, 0x06040200u);                  // e & 127
        hi[c] = __builtin_amdgcn_perm((xb >> 6) & 0x00FE00FEu, (xa >> 6) & 0x00FE00FEu, 0x06040200u);    // 2 (e >> 7)
      }
      if (lane < nch) {
        *(uint4 *)(stLo + row * g.pitchA + 16 * lane) = make_uint4(lo[0], lo[1], lo[2], lo[3]);
        *(uint4 *)(stHi + row * g.pitchA + 16 * lane) = make_uint4(hi[0], hi[1], hi[2], hi[3]);
      }
    }
    __syncthreads();                                     // stages (and, the first time, the key arrays) complete
    for_each_strip<4>(g.NT, wave, [&](int kb0, int nt) {
      auto epi = [&](auto &lo, auto &hi) {
        constexpr int NTS = sizeof(lo) / sizeof(lo[0]);
        // descriptors made here, from a re-materialised base, live in scalar registers only while they are used (see k_decrypt_m)
        long bb = b0;
        asm volatile("" : "+s"(bb));
        const long lf = (B - bb) * LD;
        const __amdgpu_buffer_rsrc_t rs_r = rows_rsrc(rem + bb * LD, 2 * lf);
        const __amdgpu_buffer_rsrc_t rs_q = rows_rsrc(want_q ? quot + bb * LD : nullptr, want_q ? 2 * lf : 0);
        int voff[NTS];                                   // a column behind N: an offset no store survives
#pragma unroll
        for (int t = 0; t < NTS; t++) voff[t] = 32 * (kb0 + t) + (lane & 31) < N ? 2 * lane_off : (int)0x80000000;
        auto out = [&](auto wq) {
#pragma unroll
          for (int i = 0; i < 16; i++) {                 // register i: row (i & 3) + 8 (i >> 2) (+ 4 in the upper half-wave)
            const int ro = (i & 3) + 8 * (i >> 2);
#pragma unroll
            for (int t = 0; t < NTS; t++) {
              const int so = 2 * (ro * LD + 32 * (kb0 + t));
              __builtin_amdgcn_raw_buffer_store_b16((u16)((u32)(lo[t][i] + hi[t][i]) & (q - 1)), rs_r, voff[t], so, ST_AUX);
              if (decltype(wq)::value) __builtin_amdgcn_raw_buffer_store_b16((u16)((u32)(0 - hi[t][i]) & (q - 1)), rs_q, voff[t], so, ST_AUX);
            }
          }
        };
        if (want_q) out(std::true_type{}); else out(std::false_type{});
      };
      switch (nt) {
        case 1: mul_shared_strip<1>(st0, st1, tb0, tb1, g, kb0, mlow, epi); break;
        case 2: mul_shared_strip<2>(st0, st1, tb0, tb1, g, kb0, mlow, epi); break;
        case 3: mul_shared_strip<3>(st0, st1, tb0, tb1, g, kb0, mlow, epi); break;
        default: mul_shared_strip<4>(st0, st1, tb0, tb1, g, kb0, mlow, epi); break;
      }
    });
  }
}

// s [N] -> out [n / N][N]
__global__ void k_mul_shared_replicate(const u16 *__restrict__ s, int N, long n, u16 *__restrict__ out) {
  for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (long)gridDim.x * blockDim.x) out[i] = s[i % N];
}

// The argument checks of both forms, before the engine is looked at.
int check_mul_shared(const ntru_engine *eng, int N, int mod, const uint16_t *s, const uint16_t *rows, int64_t B, const uint16_t *quot,
                     const uint16_t *rem) {
  const std::string who = "ntru_mul_shared_batch: ";
  if (B < 0) return fail(NTRU_ERR_ARG, who + "negative batch size");
  if (!ntru_engine_supports(N, mod))
    return fail(NTRU_ERR_UNSUPPORTED, who + "unsupported (N, mod): mod must be a power of two <= 65536 or satisfy N*(mod-1)^2 < 65536");
  if (B > 0 && (!s || !rows || !rem)) return fail(NTRU_ERR_ARG, who + std::string("NULL buffer (") + (!s ? "s" : !rows ? "rows" : "rem") + ")");
  const size_t all = (size_t)B * N * 2, one = (size_t)N * 2;
  for (const uint16_t *o : {rem, quot}) {
    const std::string name = o == rem ? "rem" : "quot";
    if (ntru_ranges_overlap(o, all, rows, all)) return fail(NTRU_ERR_ARG, who + name + " overlaps rows");
    if (B > 0 && ntru_ranges_overlap(o, all, s, one)) return fail(NTRU_ERR_ARG, who + name + " overlaps s");
  }
  if (ntru_ranges_overlap(quot, all, rem, all)) return fail(NTRU_ERR_ARG, who + "quot overlaps rem");
  if (!eng) return fail(NTRU_ERR_ARG, "engine is NULL");
  return NTRU_OK;
}

// Whether k_mul_shared_m takes (N, mod): a power-of-two mod within make_mgeom's range, and the stages and key arrays in LDS.
bool mul_shared_matrix(const ntru_engine *eng, int N, int mod, MGeom *mg, size_t *lds) {
  if (!is_pow2(mod) || !make_mgeom(eng, N, mod, N, mg)) return false;
  *lds = (size_t)64 * mg->pitchA + (size_t)32 * mg->tpitch;      // two stages of 32 rows, two key arrays of 4 copies
  return *lds <= 160 * 1024;
}

// Enqueues the product for B >= 1 rows.
int launch_mul_shared(ntru_engine *eng, int N, int mod, const uint16_t *d_s, const uint16_t *d_rows, int64_t B, uint16_t *d_quot,
                      uint16_t *d_rem) {
  HIP_TRY(hipSetDevice(eng->device));
  MGeom mg;
  size_t lds;
  if (mul_shared_matrix(eng, N, mod, &mg, &lds)) {
    note_kernel(eng, "k_mul_shared_m");
    return launch_resident(eng, k_mul_shared_m, (long)((B + 31) / 32), BLOCK_THREADS, lds, mg, (u32)mod, (const u16 *)d_s, (const u16 *)d_rows,
                           (long)B, (u16 *)d_quot, (u16 *)d_rem);
  }
  // s replicated once for the longest pass, then the per-item kernels pass by pass; a quotient nobody wants goes to scratch
  const int64_t pass = std::min(B, MS_FALLBACK_PASS);
  Carve c;
  const size_t rep_at = c.take((size_t)pass * N * 2), quot_at = d_quot ? 0 : c.take((size_t)pass * N * 2);
  ScratchHold hold(eng, c.total);
  if (hold.rc) return hold.rc;
  uint16_t *rep = (uint16_t *)(hold.p + rep_at), *qtmp = (uint16_t *)(hold.p + quot_at);
  const long el = (long)(pass * N);
  hipLaunchKernelGGL(k_mul_shared_replicate, elementwise_grid(eng, el), dim3(256), 0, eng->stream, (const u16 *)d_s, N, el, (u16 *)rep);
  HIP_TRY(hipGetLastError());
  if (int rc = for_each_pass(B, pass, [&](int64_t o, int64_t n) {
        uint16_t *q = d_quot ? d_quot + o * N : qtmp;
        const int rc = ntru_launch_polymul_matrix(eng, N, mod, d_rows + o * N, rep, n, q, d_rem + o * N);
        return rc != NTRU_NOT_TAKEN ? rc : ntru_launch_polymul_valu(eng, N, mod, d_rows + o * N, rep, n, q, d_rem + o * N);
      }))
    return rc;
  char inner[sizeof eng->last_kernel];                   // last_kernel: the product's kernel inside the replicated path
  snprintf(inner, sizeof inner, "%s", eng->last_kernel);
  snprintf(eng->last_kernel, sizeof eng->last_kernel, "mul_shared_replicated(%.36s)", inner);
  return NTRU_OK;
}

}  // namespace

extern "C" int ntru_mul_shared_batch_dev(ntru_engine_t *eng, int N, int mod, const uint16_t *d_s, const uint16_t *d_rows, int64_t B,
                                         uint16_t *d_quot, uint16_t *d_rem) {
  if (int rc = check_mul_shared(eng, N, mod, d_s, d_rows, B, d_quot, d_rem)) return rc;
  if (B == 0) return NTRU_OK;
  return launch_mul_shared(eng, N, mod, d_s, d_rows, B, d_quot, d_rem);
}

// The rows flow through the chunked pipeline; s goes up with every chunk as a shared input, as h does for ntru_encrypt_batch.
extern "C" int ntru_mul_shared_batch(ntru_engine_t *eng, int N, int mod, const uint16_t *s, const uint16_t *rows, int64_t B,
                                     uint16_t *quot, uint16_t *rem) {
  if (int rc = check_mul_shared(eng, N, mod, s, rows, B, quot, rem)) return rc;
  if (B == 0) return NTRU_OK;
  const size_t row = (size_t)N * 2;
  Pipeline P(eng);
  const int is = P.in(s, row, true), ir = P.in(rows, row), iq = P.out(quot, row), im = P.out(rem, row);
  return P.run(B, ntru_chunk_items(B), [&](int64_t, int64_t n, void **d) {
    return launch_mul_shared(eng, N, mod, (const uint16_t *)d[is], (const uint16_t *)d[ir], n, (uint16_t *)d[iq], (uint16_t *)d[im]);
  });
}
