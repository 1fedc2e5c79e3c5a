// matrix_decrypt.hip -- MI355X (gfx950), family 4: decryptBits (index.js:111-140) for a batch under ONE shared key: a = f * e mod q,
// split, centred lift (index.js:117 verbatim), c = fp * b mod p, split -- both products as batch x Toeplitz matrix products on the int8
// matrix cores, chained in one kernel (the lifted message never leaves the CU).  matrix_common.h holds the tile geometry and the
// strip loop; tools/mfma_model.py is the executable specification.
#include "matrix_common.h"

// decryptBits on the matrix cores.  Product 1: a = f * e, e = lo7 + 128 hi (both digits non-negative, q <= 8192), planes
// [e_lo | 2 e_hi] x [f ; 64 f]; centred lift (index.js:117 verbatim); product 2: c = fp * lifted, one plane.  The lifted
// message goes from the accumulator layout (column per lane) to the operand layout (row per lane) through a 2-bit packed
// LDS image [8 row groups][columns] (4 rows per byte).
// GROUPS = 1: one workgroup = four waves = one row block at a time, two workgroups per CU (k_decrypt_m); one pass expands the
// image into the byte stage that product 2 reads.
// GROUPS = 2 (k_decrypt_m8): ONE workgroup of eight waves per CU = two groups of four, each with its own row blocks, stages and
// packed image, sharing the key arrays, the lift table and the mod-p tables.  Every matrix loop and every epilogue is a PHASE between two
// workgroup barriers, and group 1 runs one phase behind group 0: while one group's waves are in their matrix loops, the
// other group's waves (their partners on the SIMDs) are in an epilogue / staging phase, by construction instead of by
// luck.  Product 2 reads its batch operand from the packed image itself (M_DEC2P: the 2-bit field is shifted out in the loop), so
// there is no expansion phase.  Phases per row block: stage, then (loop, epilogue) per strip and product:
//     S  L E  L E  L E  L E      (9 at N = 821; S L E L E where a product is one round of strips)
// An odd period whose phases alternate between a loop and something else: with group 1 one phase behind, every slot pairs a loop
// of one group with an epilogue or the staging of the other, except the one slot (S, E) per period in which neither is in a loop.
// (Staging the NEXT row block during product 2 removes that slot too and measured slower: EXPERIMENTS.md, "Lock-step decrypt:
// product 2 from the packed image".)
// PACK (k_decrypt_mp): packOutput(p - 1, N, value) (index.js:572-596: 2 bits per value, 126 values per 252-bit field element, four
// little-endian 64-bit limbs per element) comes out of the same kernel: product 2's epilogue drops its values into a 2-bit packed
// LDS image [8 row groups][columns] (4 rows per byte -- the layout product 1 uses for the lifted message: one ds_write_b8 per four
// accumulator registers), and at the top of the next trip every thread turns 16 columns of one row into one dword of the packed
// row (the row block's packed rows are contiguous: consecutive threads store consecutive dwords).  `value` itself is optional
// then: the pipeline's pack mode writes 32 ceil(N / 126) bytes per item instead of N + 32 ceil(N / 126).
// (First version: DPP gather + ds_or_b32 into an image of the packed rows: bit-exact, 3.65 ms per 2^20 against 1.83 ms for the
// plain value-only kernel -- 1248 LDS atomics per row block with 4 active lanes each.)
template <int GROUPS, bool PACK = false>
static __device__ __forceinline__ void decrypt_m_body(MGeom g, u32 q, u32 p, u32 lift_add, const int8_t *__restrict__ f,
                                                      const uint8_t *__restrict__ fp,
                                                      const u16 *__restrict__ e, long B,
                                                      uint8_t *__restrict__ value, u16 *__restrict__ quot1,
                                                      u16 *__restrict__ rem1, uint8_t *__restrict__ quot2,
                                                      unsigned long long *__restrict__ packed = nullptr, int pack_os = 0) {
  extern __shared__ __attribute__((aligned(16))) unsigned char lds[];
  const int group = GROUPS == 2 ? __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 8)) : 0;
  // LDS layout: per group [e_hi stage][e_lo stage][packed image], then the shared key arrays and the lift table.  The mod-p
  // tables of product 2 are at LDS address 0, so that their lookups need no base add: GROUPS = 1 overlays them on the e_hi
  // stage and rebuilds them per row block; GROUPS = 2 builds them once, in a region of their own in front of the groups'.
  static_assert(!PACK || GROUPS == 1, "fused packOutput is built on the plain four-wave kernel");
  // mod-p tables of product 2: (-x) mod p at LDS address x, so that the quotient lookup's address IS the `high` accumulator;
  // x mod p at M3V + x, the base folded into the low + high add
  const int M3V = __builtin_amdgcn_readfirstlane(((int)((p - 1) * (p - 1)) * g.N + 4) & ~3);
  const int m3_bytes = GROUPS == 2 ? (M3V + (int)((p - 1) * (p - 1)) * g.N + 1 + 15) & ~15 : 0;
  const int gbytes = 64 * g.pitchA + 256 * g.NT;
  // (one wave-uniform offset: as two adds, this base costs the lock-step kernel six more SGPR spills)
  unsigned char *stHi = lds + (GROUPS == 2 ? __builtin_amdgcn_readfirstlane(m3_bytes + group * gbytes) : 0);
  unsigned char *stLo = stHi + 32 * g.pitchA;
  unsigned char *blp = stLo + 32 * g.pitchA;             // [8 row groups][32 NT columns]: 4 rows x 2 bits per byte
  // GROUPS = 2 keeps a third key array, TF64 = the 64 f plane of product 1 (the four-wave kernels derive it from f in the loop)
  u32 *TF = (u32 *)(lds + m3_bytes + GROUPS * gbytes), *TP = TF + 4 * g.tpitch, *TF64 = TP + 4 * g.tpitch;
  unsigned char *lift_lut = (unsigned char *)(TP + 4 * g.tpitch * GROUPS);   // [q]: centred lift followed by mod p: index.js:117 with lift_add in place of its 1
  // PACK: 2-bit image of product 2's values, [8 row groups][pcols] bytes, pcols = 126 pack_os + 16 >= 32 NT (zero beyond N).  It lives
  // in the e_hi stage behind the mod-p tables (dead between product 1's last loop and the next trip's staging: no LDS of its own --
  // 7 KB more would cost the second workgroup of the CU); it is turned into packed dwords at the top of the next trip, and a barrier
  // separates that from the staging writes.
  const int pcols = 126 * pack_os + 16, pimg_bytes = (8 * pcols + 15) & ~15;
  unsigned char *pimg = stHi + ((((int)((p - 1) * (p - 1)) * g.N + 4) & ~3) + (int)((p - 1) * (p - 1)) * g.N + 1 + 15 & ~15);
  auto pack_flush = [&](long rbx) {                      // the image of row block rbx -> packed[32 rbx ..]; thread = one dword of one row
    const long b0x = rbx << 5;
    const int rows_left = (int)(B - b0x < 32 ? B - b0x : 32);
    u32 *dst = (u32 *)packed + b0x * 8 * pack_os;
    const int per_row = 8 * pack_os;
    for (int x = (int)threadIdx.x; x < rows_left * per_row; x += BLOCK_THREADS) {
      const int R = x / per_row, dw = x - R * per_row, o = dw >> 3, k = dw & 7;
      const unsigned char *src = pimg + (2 * (R >> 3) + ((R >> 2) & 1)) * pcols + 126 * o + 16 * k;
      u32 d[4];                                              // sixteen columns; the address is only 2-byte aligned
#pragma unroll
      for (int c = 0; c < 4; c++) __builtin_memcpy(&d[c], src + 4 * c, 4);
      const u32 out = pack2x16(d, 2 * (R & 3));              // row R's values are bits 2 (R & 3) .. of its row group's bytes
      dst[x] = k == 7 ? out & 0x0FFFFFFFu : out;             // 126 = 7 x 16 + 14: the eighth dword of an element holds 14 values
    }
  };
  auto pack_wipe = [&]() {                               // the staging of product 1 has been here since: columns >= N must read zero again
    for (int x = (int)threadIdx.x; x < pimg_bytes / 16; x += BLOCK_THREADS) *(uint4 *)(pimg + 16 * x) = make_uint4(0u, 0u, 0u, 0u);
  };
  unsigned char *m3_lut = lds;
  auto build_m3 = [&](int tid, int nthr, int n) {
    for (int x = tid; x <= (int)((p - 1) * (p - 1)) * n; x += nthr) {
      const u32 rm = mod_small((u32)x, p);
      m3_lut[x] = (unsigned char)(rm ? p - rm : 0u);
      m3_lut[M3V + x] = (unsigned char)rm;
    }
  };
  const int tid0 = threadIdx.x & (BLOCK_THREADS - 1), lane0 = tid0 & 63, wave = __builtin_amdgcn_readfirstlane(tid0 >> 6);
  build_toeplitz_array(TF, g, [&](int i) { return (int)f[i]; }, (int)threadIdx.x, GROUPS * BLOCK_THREADS);
  build_toeplitz_array(TP, g, [&](int i) { return (int)fp[i]; }, (int)threadIdx.x, GROUPS * BLOCK_THREADS);
  if (GROUPS == 2)   // 64 f: the two low bits of every digit of f in bits 6-7 (f in {-1,0,1}: 0xC0, 0, 0x40)
    build_toeplitz_array(TF64, g, [&](int i) { return (int)(((u32)f[i] << 6) & 0xC0u); }, (int)threadIdx.x, GROUPS * BLOCK_THREADS);
  for (u32 x = threadIdx.x; x < q; x += GROUPS * BLOCK_THREADS) lift_lut[x] = (unsigned char)lift_value(x, q, p, lift_add);
  if (GROUPS == 2) build_m3((int)threadIdx.x, GROUPS * BLOCK_THREADS, g.N);
  auto phase = [&]() { if (GROUPS == 2) __syncthreads(); };   // a boundary of the lock-step schedule
  if (GROUPS == 2 && group == 1) __syncthreads();                   // group 1 runs one phase behind group 0
  const bool want_q1 = quot1 != nullptr, want_r1 = rem1 != nullptr, want_q2 = quot2 != nullptr;
  const long nrb = (B + 31) >> 5;
  const int nch = 2 * g.NT;
  const u32 qm2 = (q - 1) * 0x00010001u;
  int sidx = 0, stamp_iter = -1;
  const long stride = (long)gridDim.x * GROUPS, iters = (nrb + stride - 1) / stride;
  const int rounds = (((g.NT + 3) >> 2) + WAVES_PER_BLOCK - 1) / WAVES_PER_BLOCK;
  for (long it = 0; it < iters; it++) {
    // a group without a row block left (the last trip of an odd count) still walks through every phase: its row block is
    // placed at the end of the batch, where every load reads zero and every store is dropped by the buffer descriptors
    long rb = (long)blockIdx.x * GROUPS + group + it * stride;
    rb = rb < nrb ? rb : nrb;
    stamp_iter++;
    STAMP(0);
    int lane = lane0, N = g.N, LD = g.ld;                // see k_encrypt_m
    asm volatile("" : "+v"(lane), "+s"(N), "+s"(LD));
    const u32 *tbf = frag_lane_base(TF, g, lane), *tbp = frag_lane_base(TP, g, lane);
    const u32 *tbf64 = GROUPS == 2 ? frag_lane_base(TF64, g, lane) : tbf;

    const unsigned char *st0 = stLo + (lane & 31) * g.pitchA + 16 * (lane >> 5);
    const unsigned char *st1 = stHi + (lane & 31) * g.pitchA + 16 * (lane >> 5);
    u32 mlow[4];
    diag_low_mask(lane, mlow);
    const long b0 = rb << 5 < B ? rb << 5 : B, left = (B - b0) * LD;
    const AlignedSrc src_e = aligned_src(e + b0 * LD, 2 * left);
    // lane = 16 coefficients.  (Requesting these loads before the barrier, as k_encrypt_m does, measured 3 % slower with two
    // workgroups per CU and 5 % slower in the lock-step schedule.)
    constexpr int RPW = 32 / WAVES_PER_BLOCK;
    RawChunks<2> raw[RPW];
    int sh[RPW];
    auto request_rows = [&]() {
#pragma unroll
      for (int j = 0; j < RPW; j++) {
        const int pos0 = src_e.a0 + 2 * (wave + WAVES_PER_BLOCK * j) * LD;
        sh[j] = __builtin_amdgcn_readfirstlane(pos0 & 15);
        raw[j] = load_raw<2>(src_e, pos0 + 32 * lane, sh[j]);
      }
    };
    __syncthreads();
    STAMP(1);
    request_rows();
    if (PACK && it > 0) {                                // every wave has left the previous trip's epilogues; this trip's rows are in flight
      pack_flush((long)blockIdx.x * GROUPS + group + (it - 1) * stride);
      __syncthreads();                                   // ... before the staging below overwrites the image
    }
    {
      const int c16 = lane;
      u32 cmask[8];                                      // columns >= N of the last chunk(s) are zero; coefficients mod q
#pragma unroll
      for (int c = 0; c < 8; c++) {
        const int left2 = N - (16 * c16 + 2 * c);
        cmask[c] = qm2 & (left2 >= 2 ? 0xFFFFFFFFu : (left2 == 1 ? 0x0000FFFFu : 0u));
      }
#pragma unroll
      for (int j = 0; j < RPW; j++) {
        const int row = wave + WAVES_PER_BLOCK * j;
        v4i v[2];                                        // 16 coefficients as u16 pairs
        shift_raw<2>(raw[j], sh[j], v);
        u32 x[8];
#pragma unroll
        for (int c = 0; c < 4; c++) { x[c] = (u32)v[0][c]; x[4 + c] = (u32)v[1][c]; }
        u32 lo[4], hi[4];
#pragma unroll
        for (int c = 0; c < 4; c++) {
          const u32 xa = x[2 * c] & cmask[2 * c], xb = x[2 * c + 1] & cmask[2 * c + 1];
          lo[c] = __builtin_amdgcn_perm(xb & 0x007F007Fu, xa & 0x007F007Fu, 0x06040200u);
          hi[c] = __builtin_amdgcn_perm((xb >> 6) & 0x00FE00FEu, (xa >> 6) & 0x00FE00FEu, 0x06040200u);
        }
        if (c16 < nch) {
          *(uint4 *)(stLo + row * g.pitchA + 16 * c16) = make_uint4(lo[0], lo[1], lo[2], lo[3]);
          *(uint4 *)(stHi + row * g.pitchA + 16 * c16) = make_uint4(hi[0], hi[1], hi[2], hi[3]);
        }
      }
    }
    STAMP(2);
    __syncthreads();
    STAMP(3);
    const int lane_off = (lane >> 5) * 4 * LD + (lane & 31);
    // ---- product 1: a = f * e mod q; witness stores; lifted message -> packed image
    sidx = 0;
    constexpr int P1 = GROUPS == 2 ? M_DEC1T : M_DEC1;
    for_each_strip<4>(g.NT, GROUPS == 2 ? wave ^ (2 * group) ^ (2 * blockIdx.x >= gridDim.x ? 2 : 0) : wave, [&](int kb0, int nt) {
      auto epi = [&](auto &lo, auto &hi) {
        constexpr int NTS = sizeof(lo) / sizeof(lo[0]);
        phase();                                         // matrix loop | epilogue
        // descriptors are made here, from a re-materialised row-block base, so that they live in scalar registers only
        // while they are used (held across the matrix loops they are spilled to VGPRs and every store becomes a
        // waterfall loop)
        long bb = b0;
        asm volatile("" : "+s"(bb));
        const long lf = (B - bb) * LD;
        const __amdgpu_buffer_rsrc_t rs_r1 = rows_rsrc(want_r1 ? rem1 + bb * LD : nullptr, want_r1 ? 2 * lf : 0);
        const __amdgpu_buffer_rsrc_t rs_q1 = rows_rsrc(want_q1 ? quot1 + bb * LD : nullptr, want_q1 ? 2 * lf : 0);
        int voff[NTS];                                   // see k_encrypt_m
#pragma unroll
        for (int t = 0; t < NTS; t++) voff[t] = 32 * (kb0 + t) + (lane & 31) < N ? 2 * lane_off : (int)0x80000000;
        auto out = [&](auto wr, auto wq) {
#pragma unroll
          for (int j = 0; j < 4; j++) {                  // 4 rows x the strip's tiles at a time: remainders (and their
            u32 xs[NTS][4], lv[NTS][4];                  // stores), then their table lookups in flight together, then packing
#pragma unroll
            for (int ii = 0; ii < 4; ii++) {
              const int i = 4 * j + ii, ro = ii + 8 * j;
#pragma unroll
              for (int t = 0; t < NTS; t++) {
                const u32 x = (u32)(lo[t][i] + hi[t][i]) & (q - 1);
                xs[t][ii] = x;
                const int so = 2 * (ro * LD + 32 * (kb0 + t));
                {
                  if (decltype(wr)::value) __builtin_amdgcn_raw_buffer_store_b16((u16)x, rs_r1, voff[t], so, ST_AUX);
                  if (decltype(wq)::value) __builtin_amdgcn_raw_buffer_store_b16((u16)((u32)(0 - hi[t][i]) & (q - 1)), rs_q1, voff[t], so, ST_AUX);
                }
              }
            }
#pragma unroll
            for (int t = 0; t < NTS; t++)
#pragma unroll
              for (int ii = 0; ii < 4; ii++) lv[t][ii] = lift_lut[xs[t][ii]];
#pragma unroll
            for (int t = 0; t < NTS; t++) {
              const int col = 32 * (kb0 + t) + (lane & 31);
              const u32 pk = lv[t][0] | (lv[t][1] << 2) | (lv[t][2] << 4) | (lv[t][3] << 6);
              blp[((lane >> 5) + 2 * j) * 32 * g.NT + col] = (unsigned char)(col < N ? pk : 0u);   // [row group 2j+hh][column]
            }
          }
        };
        if (want_r1 && want_q1) out(std::true_type{}, std::true_type{});
        else if (want_r1) out(std::true_type{}, std::false_type{});
        else if (want_q1) out(std::false_type{}, std::true_type{});
        else out(std::false_type{}, std::false_type{});
      };
      switch (nt) {
        case 0: phase(); break;                          // (the strip list hands out empty strips only to keep the phases in step)
        case 1: toeplitz_strip<P1, 1>(st0, st1, tbf, tbf64, g, kb0, mlow, epi, stamp_iter, 4 + 2 * sidx); break;
        case 2: toeplitz_strip<P1, 2>(st0, st1, tbf, tbf64, g, kb0, mlow, epi, stamp_iter, 4 + 2 * sidx); break;
        case 3: toeplitz_strip<P1, 3>(st0, st1, tbf, tbf64, g, kb0, mlow, epi, stamp_iter, 4 + 2 * sidx); break;
        default: toeplitz_strip<P1, 4>(st0, st1, tbf, tbf64, g, kb0, mlow, epi, stamp_iter, 4 + 2 * sidx); break;
      }
      sidx++;
      if (sidx < rounds) phase();                        // epilogue | next matrix loop (after the last strip: the barrier below)
    }, GROUPS == 2);
    __syncthreads();                                 // every wave is done with the e stages; packed image complete
    STAMP(8);
    if (PACK) pack_wipe();
    if (GROUPS == 1) build_m3(tid0, BLOCK_THREADS, N);     // the e stages are dead: the tables go over the e_hi stage
    if (GROUPS == 1) {   // packed image -> byte stage: all of a wave's reads in flight before the first write (as a read-write loop this
        // pass was one LDS round trip per dword: 7 k cycles per row block in the phase stamps)
      constexpr int RPW = 32 / WAVES_PER_BLOCK;
      u32 pv[RPW][4];
#pragma unroll
      for (int j = 0; j < RPW; j++) {
        const int row = wave + WAVES_PER_BLOCK * j, rgb = 2 * (row >> 3) + ((row >> 2) & 1);
        const u32 *src = (const u32 *)(blp + rgb * 32 * g.NT);
#pragma unroll
        for (int it = 0; it < 4; it++) pv[j][it] = src[(lane + 64 * it) < 8 * g.NT ? lane + 64 * it : 0];
      }
#pragma unroll
      for (int j = 0; j < RPW; j++) {
        const int row = wave + WAVES_PER_BLOCK * j, sh = 2 * (row & 3);
#pragma unroll
        for (int it = 0; it < 4; it++)
          if (lane + 64 * it < 8 * g.NT) *(u32 *)(stLo + row * g.pitchA + 4 * (lane + 64 * it)) = (pv[j][it] >> sh) & 0x03030303u;
      }
    }
    STAMP(9);
    if (GROUPS == 1) __syncthreads();
    STAMP(10);
    // ---- product 2: c = fp * lifted mod p
    // GROUPS = 2 reads the batch operand straight from the packed image: lane (row, half) reads the 16 columns of its row group
    // (one 16-byte aligned address in the four lanes of a row group: an LDS broadcast) and shifts its own 2-bit field out.
    constexpr int P2 = GROUPS == 2 ? M_DEC2P : M_DEC2;
    const unsigned char *a2 = GROUPS == 2 ? blp + ((lane & 31) >> 2) * 32 * g.NT + 16 * (lane >> 5) : st0;
    const int ash = 2 * (lane & 3);
    sidx = 0;
    for_each_strip<4>(g.NT, GROUPS == 2 ? wave ^ (2 * group) ^ (2 * blockIdx.x >= gridDim.x ? 2 : 0) : wave, [&](int kb0, int nt) {
      auto epi = [&](auto &lo, auto &hi) {
        constexpr int NTS = sizeof(lo) / sizeof(lo[0]);
        phase();                                         // matrix loop | epilogue
        long bb = b0;                                    // see product 1
        asm volatile("" : "+s"(bb));
        const long lf = (B - bb) * LD;
        const __amdgpu_buffer_rsrc_t rs_v = rows_rsrc(value ? value + bb * LD : nullptr, value ? lf : 0);
        const __amdgpu_buffer_rsrc_t rs_q2 = rows_rsrc(want_q2 ? quot2 + bb * LD : nullptr, want_q2 ? lf : 0);
        int voff[NTS];                                   // see k_encrypt_m
#pragma unroll
        for (int t = 0; t < NTS; t++) voff[t] = 32 * (kb0 + t) + (lane & 31) < N ? lane_off : (int)0x80000000;
        auto out = [&](auto wq) {
#pragma unroll
          for (int j = 0; j < 4; j++) {                  // lookups of 4 rows x the strip's tiles in flight before their stores
            u32 va[NTS][4], vb[NTS][4];
#pragma unroll
            for (int t = 0; t < NTS; t++)
#pragma unroll
              for (int ii = 0; ii < 4; ii++) {
                va[t][ii] = m3_lut[(u32)(lo[t][4 * j + ii] + hi[t][4 * j + ii] + M3V)];
                vb[t][ii] = decltype(wq)::value ? (u32)m3_lut[(u32)hi[t][4 * j + ii]] : 0u;
              }
            if (PACK) {
#pragma unroll
              for (int t = 0; t < NTS; t++) {
                const int col = 32 * (kb0 + t) + (lane & 31);
                const u32 pk = va[t][0] | (va[t][1] << 2) | (va[t][2] << 4) | (va[t][3] << 6);
                if (col < N) pimg[((lane >> 5) + 2 * j) * pcols + col] = (unsigned char)pk;   // [row group 2j+hh][column]; columns >= N stay zero
              }
            }
#pragma unroll
            for (int ii = 0; ii < 4; ii++) {
              if (PACK && value == nullptr) break;         // pack mode without the plain values
#pragma unroll
              for (int t = 0; t < NTS; t++) {
                const int so = (ii + 8 * j) * LD + 32 * (kb0 + t);
                {
                  __builtin_amdgcn_raw_buffer_store_b8((uint8_t)va[t][ii], rs_v, voff[t], so, ST_AUX);
                  if (decltype(wq)::value) __builtin_amdgcn_raw_buffer_store_b8((uint8_t)vb[t][ii], rs_q2, voff[t], so, ST_AUX);
                }
              }
            }
          }
        };
        if (want_q2) out(std::true_type{}); else out(std::false_type{});
      };
      switch (nt) {
        case 0: phase(); break;                          // no strip this round: keep the phases in step
        case 1: toeplitz_strip<P2, 1>(a2, a2, tbp, tbp, g, kb0, mlow, epi, stamp_iter, 11 + 2 * sidx, 0x7fffffff, NoPause(), NoDiag(), ash); break;
        case 2: toeplitz_strip<P2, 2>(a2, a2, tbp, tbp, g, kb0, mlow, epi, stamp_iter, 11 + 2 * sidx, 0x7fffffff, NoPause(), NoDiag(), ash); break;
        case 3: toeplitz_strip<P2, 3>(a2, a2, tbp, tbp, g, kb0, mlow, epi, stamp_iter, 11 + 2 * sidx, 0x7fffffff, NoPause(), NoDiag(), ash); break;
        default: toeplitz_strip<P2, 4>(a2, a2, tbp, tbp, g, kb0, mlow, epi, stamp_iter, 11 + 2 * sidx, 0x7fffffff, NoPause(), NoDiag(), ash); break;
      }
      sidx++;
      if (sidx < rounds) phase();                        // epilogue | next matrix loop
    }, GROUPS == 2);
  }
  if (GROUPS == 2 && group == 0) __syncthreads();     // group 1's last phase
  if (PACK && iters > 0) {
    __syncthreads();                                    // the last trip's epilogues
    const long last = (long)blockIdx.x + (iters - 1) * stride;
    if (last < nrb) pack_flush(last);
  }
}

__global__ __launch_bounds__(BLOCK_THREADS, 2) void k_decrypt_m(MGeom g, u32 q, u32 p, u32 lift_add, const int8_t *__restrict__ f,
                                                             const uint8_t *__restrict__ fp,
                                                             const u16 *__restrict__ e, long B,
                                                             uint8_t *__restrict__ value, u16 *__restrict__ quot1,
                                                             u16 *__restrict__ rem1, uint8_t *__restrict__ quot2) {
  decrypt_m_body<1>(g, q, p, lift_add, f, fp, e, B, value, quot1, rem1, quot2);
}

__global__ __launch_bounds__(2 * BLOCK_THREADS, 1) void k_decrypt_m8(MGeom g, u32 q, u32 p, u32 lift_add, const int8_t *__restrict__ f,
                                                                  const uint8_t *__restrict__ fp,
                                                                  const u16 *__restrict__ e, long B,
                                                                  uint8_t *__restrict__ value, u16 *__restrict__ quot1,
                                                                  u16 *__restrict__ rem1, uint8_t *__restrict__ quot2) {
  decrypt_m_body<2>(g, q, p, lift_add, f, fp, e, B, value, quot1, rem1, quot2);
}

// decryptBits + packOutput(p - 1, N, value) in one kernel (decrypt_m_body<.., PACK>); `value` may be NULL.
__global__ __launch_bounds__(BLOCK_THREADS, 2) void k_decrypt_mp(MGeom g, u32 q, u32 p, u32 lift_add, const int8_t *__restrict__ f,
                                                              const uint8_t *__restrict__ fp,
                                                              const u16 *__restrict__ e, long B,
                                                              uint8_t *__restrict__ value, unsigned long long *__restrict__ packed, int pack_os) {
  decrypt_m_body<1, true>(g, q, p, lift_add, f, fp, e, B, value, nullptr, nullptr, nullptr, packed, pack_os);
}

NTRU_STAMPS_READER(ntru_debug_read_stamps_dec)

// ---- host side ----------------------------------------------------------------------------------------------------------
// decryptBits + packOutput fused (k_decrypt_mp): p == 3, the matrix path's range, a 16-byte aligned packed array.
int ntru_launch_decrypt_pack_matrix(ntru_engine *eng, int N, int q, int p, const int8_t *d_f, const uint8_t *d_fp, const uint16_t *d_e,
                                    int64_t B, uint8_t *d_value, uint64_t *d_packed, int out_size) {
  MGeom mg;
  if (p != 3 || ((uintptr_t)d_packed & 15) != 0 || !make_mgeom(eng, N, q, N, &mg)) return NTRU_NOT_TAKEN;
  const size_t lds = (size_t)32 * mg.tpitch + (size_t)64 * mg.pitchA + (size_t)256 * mg.NT + (((size_t)q + 15) & ~(size_t)15);
  // the 2-bit image of the values lives in the e_hi stage behind the mod-p tables
  const size_t m3_end = ((((size_t)4 * N + 4) & ~(size_t)3) + (size_t)4 * N + 1 + 15) & ~(size_t)15, img = ((size_t)8 * (126 * out_size + 16) + 15) & ~(size_t)15;
  if (lds > 160 * 1024 || m3_end + img > (size_t)32 * mg.pitchA || 126 * out_size + 16 < 32 * mg.NT) return NTRU_NOT_TAKEN;
  note_kernel(eng, "k_decrypt_mp");
  return launch_resident(eng, k_decrypt_mp, (long)((B + 31) / 32), BLOCK_THREADS, lds, mg, (u32)q, (u32)p, ntru_lift_addend(eng, q, p), d_f, d_fp, d_e, (long)B, d_value,
                         (unsigned long long *)d_packed, out_size);
}

// Kernel paths: 4 -> k_decrypt_m (two free-running workgroups per CU); 5 -> k_decrypt_m8 (one workgroup of two lock-step groups)
// wherever its LDS fits; 0 = auto -> k_decrypt_m8 where a product takes two rounds of strips (N > 512) and every witness array is
// asked for: 2.52 against 2.63 ms per 2^20 at N = 821 (profiles/archive/r02_ab_lockstep_phase_masks.txt), 2.16 against 2.24 ms at N = 701;
// at N = 509 (one round) it is 6 % slower, and so it is without the witness arrays (shorter epilogues: 2.23 against 2.02 ms).
int ntru_launch_decrypt_matrix(ntru_engine *eng, int N, int q, int p, int ld, const int8_t *d_f, const uint8_t *d_fp, const uint16_t *d_e,
                               int64_t B, uint8_t *d_value, uint16_t *d_quot1, uint16_t *d_rem1, uint8_t *d_quot2) {
  MGeom mg;
  if (p != 3 || !make_mgeom(eng, N, q, ld, &mg)) return NTRU_NOT_TAKEN;
  const size_t lds = (size_t)32 * mg.tpitch + (size_t)64 * mg.pitchA + (size_t)256 * mg.NT + (((size_t)q + 15) & ~(size_t)15);
  const long nrb = (long)((B + 31) / 32);
  if (eng->path == 5 || (eng->path == 0 && mg.NT > 16 && d_quot1 && d_rem1 && d_quot2)) {
    // two groups' stages and images, the mod-p tables of product 2, three key arrays (f, fp, 64 f), the lift table
    const size_t m3 = ((((size_t)4 * N + 4) & ~(size_t)3) + (size_t)4 * N + 1 + 15) & ~(size_t)15;
    const size_t lds8 = 2 * ((size_t)64 * mg.pitchA + (size_t)256 * mg.NT) + m3 + (size_t)48 * mg.tpitch + (((size_t)q + 15) & ~(size_t)15);
    if (lds8 <= 160 * 1024) {
      note_kernel(eng, "k_decrypt_m8");
      return launch_resident(eng, k_decrypt_m8, (nrb + 1) / 2, 2 * BLOCK_THREADS, lds8, mg, (u32)q, (u32)p, ntru_lift_addend(eng, q, p), d_f, d_fp, d_e, (long)B,
                             d_value, d_quot1, d_rem1, d_quot2);
    }
  }
  if (lds > 160 * 1024) return NTRU_NOT_TAKEN;
  note_kernel(eng, "k_decrypt_m");
  return launch_resident(eng, k_decrypt_m, nrb, BLOCK_THREADS, lds, mg, (u32)q, (u32)p, ntru_lift_addend(eng, q, p), d_f, d_fp, d_e, (long)B, d_value, d_quot1,
                         d_rem1, d_quot2);
}
