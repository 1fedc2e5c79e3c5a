// matrix_encrypt.hip -- MI355X (gfx950), family 4: encryptBits (index.js:87-110) for a batch under ONE shared key as batch x Toeplitz
// matrix products on the int8 matrix cores (v_mfma_i32_32x32x32_i8, int32 accumulation: exact), the closed-form split by 1 - x^N
// (index.js:358-401) and the plaintext add (index.js:235-244) fused into the epilogue.  matrix_common.h holds the
// tile geometry and the strip loop; tools/mfma_model.py is the executable specification.
#include "matrix_common.h"

// encryptBits on the matrix cores: e = (r * h + m) split by 1 - x^N; r in {0..3} bytes, h < q <= 8192.
// h is taken in the representative hs = d0 + 128 d1, d0 in [-64,63], 4 d1 in [-128,124]; planes [r | 32 r] x [d0 ; 4 d1].
// MAXT: widest strip.  8 (one workgroup per CU, 512 registers per wave, one strip per wave and row block) was measured at
// 2.28 ms per 2^20 against 1.51-1.58 ms for 4: with one wave per SIMD nothing overlaps the matrix loops
// (EXPERIMENTS.md, round 2); only 4 is instantiated.
// DMA (k_encrypt_md): the batch operands reach LDS by direct global -> LDS loads (buffer_load_dwordx4 ... lds, no
// registers).  r of the NEXT row block is requested into the r stage once every wave has left its last matrix
// loop -- in front of the last epilogue's stores instead of behind them (phase stamps: the rows requested at the top of a trip
// come back 8-9 k cycles later) -- and brought into operand form (shift to byte 0, columns >= N zeroed) in place by the wave that
// owns the row; m is requested straight into the m image at the top of a trip and only waited for before the first epilogue.
// Two more barriers per row block, all of them LDS-only.
template <int MAXT, bool DMA>
static __device__ __forceinline__ void encrypt_m_body(MGeom g, u32 q, const u16 *__restrict__ h,
                                                      const uint8_t *__restrict__ r,
                                                      const uint8_t *__restrict__ m, long B,
                                                      u16 *__restrict__ e, u16 *__restrict__ quotE) {
  extern __shared__ __attribute__((aligned(16))) unsigned char lds[];
  // DMA: a barrier that orders LDS traffic only.  With direct-to-LDS loads in flight the compiler puts s_waitcnt vmcnt(0) in front of
  // every __syncthreads() -- which also waits for every outstanding STORE, the very queue the early loads are meant to get ahead of.
  auto wg_barrier = [&]() {
    if (DMA) asm volatile("s_waitcnt lgkmcnt(0)\n\ts_barrier" ::: "memory");
    else __syncthreads();
  };
  u32 *T0 = (u32 *)lds, *T1 = T0 + 4 * g.tpitch;         // key arrays, then the r stage and the m image
  unsigned char *stA = (unsigned char *)(T1 + 4 * g.tpitch);
  unsigned char *mimg = stA + 32 * g.pitchA;             // rows b0..b0+31 of m exactly as in memory (pitch g.ld)
  const int tid0 = threadIdx.x & (BLOCK_THREADS - 1), lane0 = tid0 & 63, wave = __builtin_amdgcn_readfirstlane(tid0 >> 6);
  const int hthr = (int)(q >> 1) - 65;
  auto hs_of = [&](int i) { int hv = (int)(h[i] & (q - 1)); return hv > hthr ? hv - (int)q : hv; };
  // Digits of h: value = d0 + 128 d1 against the planes [r | 32 r] x [d0 ; 4 d1].  q <= 4096: NON-NEGATIVE digits (d0 = h & 127,
  // 4 d1 <= 124 fits an int8) -- a matrix instruction on operands without sign-extension bits costs less energy, and at the power cap
  // that is time: 1.450 against 1.503 ms per 2^20 at N = 821 (1.59 against 1.65 J above idle, tools/power_kernel.py, same device).
  // q = 8192: d1 reaches 63, so h is taken in the representative whose digits fit (d0 in [-64, 63], 4 d1 in [-128, 124]).
  if (q <= 4096) {
    build_toeplitz_array(T0, g, [&](int i) { return (int)(h[i] & (q - 1)) & 127; }, (int)threadIdx.x, BLOCK_THREADS);
    build_toeplitz_array(T1, g, [&](int i) { return ((int)(h[i] & (q - 1)) >> 7) * 4; }, (int)threadIdx.x, BLOCK_THREADS);
  } else {
    build_toeplitz_array(T0, g, [&](int i) { const int hs = hs_of(i); return ((hs + 64) & 127) - 64; }, (int)threadIdx.x, BLOCK_THREADS);
    build_toeplitz_array(T1, g, [&](int i) { const int hs = hs_of(i); const int d0 = ((hs + 64) & 127) - 64; return ((hs - d0) >> 7) * 4; }, (int)threadIdx.x, BLOCK_THREADS);
  }
  const bool want_q = quotE != nullptr;
  const long nrb = (B + 31) >> 5;
  int sidx = 0, stamp_iter = -1;
  const long stride = (long)gridDim.x, iters = (nrb + stride - 1) / stride;
  const int rounds = (((g.NT + MAXT - 1) / MAXT) + WAVES_PER_BLOCK - 1) / WAVES_PER_BLOCK;
  // DMA: pieces start at absolutely dword-aligned addresses (descriptor based at the dword at or below the row block, size in
  // whole dwords: the range check is per dword, and a dword that holds the last byte of the batch must not count as out of
  // range), so a row lands 0-3 bytes into its slot and the image 0-3 bytes into the m image.
  auto dma_r = [&](long rbx, int lane) {                    // rows wave, wave + 4, ... into the r stage, one instruction per row
    const long b0x = rbx << 5 < B ? rbx << 5 : B;
    const unsigned long long a = (unsigned long long)(r + b0x * g.ld);
    const int a0 = (int)(a & 3);
    const __amdgpu_buffer_rsrc_t rs = rows_rsrc((const void *)(a & ~3ULL), ((B - b0x) * g.ld + a0 + 3) & ~3L);
#pragma unroll
    for (int j = 0; j < 32 / WAVES_PER_BLOCK; j++) {
      const int row = wave + WAVES_PER_BLOCK * j, ro = a0 + row * g.ld;
      if (lane < (((ro & 3) + g.N + 15) >> 4))
        __builtin_amdgcn_raw_ptr_buffer_load_lds(rs, (__attribute__((address_space(3))) void *)(stA + row * g.pitchA), 16,
                                                 (ro & ~3) + 16 * lane, 0, 0, 0);
    }
  };
  auto dma_m = [&](long rbx, int tid) {                     // the 32 rows of m as one run of 16-byte pieces into the m image
    const long b0x = rbx << 5 < B ? rbx << 5 : B;
    const unsigned long long a = (unsigned long long)(m + b0x * g.ld);
    const int a0 = (int)(a & 3);
    const __amdgpu_buffer_rsrc_t rs = rows_rsrc((const void *)(a & ~3ULL), ((B - b0x) * g.ld + a0 + 3) & ~3L);
    const int npc = (a0 + 32 * g.ld + 15) >> 4;
#pragma unroll
    for (int j = 0; j < 8; j++)                             // 8 x 256 pieces >= 32 x 1024 / 16
      if (tid + j * BLOCK_THREADS < npc)
        __builtin_amdgcn_raw_ptr_buffer_load_lds(rs, (__attribute__((address_space(3))) void *)(mimg + 16 * (wave * 64 + j * BLOCK_THREADS)), 16,
                                                 16 * (tid + j * BLOCK_THREADS), 0, 0, 0);
  };
  if (DMA) {
    dma_r((long)blockIdx.x < nrb ? (long)blockIdx.x : nrb, lane0);
    __builtin_amdgcn_s_waitcnt(0);                         // nothing else is in flight yet
  }
  for (long it = 0; it < iters; it++) {
    long rb = (long)blockIdx.x + it * stride;   // past the end: a row block of zeros whose stores are dropped
    rb = rb < nrb ? rb : nrb;
    long rb_next = (long)blockIdx.x + (it + 1) * stride;
    rb_next = rb_next < nrb ? rb_next : nrb;
    stamp_iter++;
    STAMP(0);
    // Re-materialise the lane index and N per row block: otherwise every per-lane address / predicate of the staging
    // and of the epilogues is hoisted out of this loop and spilled around the matrix loops.
    int lane = lane0, N = g.N, LD = g.ld, tid = tid0;
    asm volatile("" : "+v"(lane), "+s"(N), "+s"(LD), "+v"(tid));
    const u32 *tb0 = frag_lane_base(T0, g, lane), *tb1 = frag_lane_base(T1, g, lane);
    const unsigned char *st0 = stA + (lane & 31) * g.pitchA + 16 * (lane >> 5);
    u32 mlow[4];
    diag_low_mask(lane, mlow);
    const long b0 = rb << 5 < B ? rb << 5 : B, left = (B - b0) * LD;   // elements from this row block to the end of the batch
    const AlignedSrc src_r = aligned_src(r + b0 * LD, left), src_m = aligned_src(m + b0 * LD, left);
    // All loads of the row block (r rows and the m image) are requested BEFORE the barrier: they land in registers, so
    // they need not wait for the previous row block's readers, and the two HBM round trips become one that overlaps the
    // barrier wait (phase stamps: 4.5 k + 4.5 k cycles back to back before).  N <= 1024: lane = 16-byte chunk of a row.
    constexpr int RPW = 32 / WAVES_PER_BLOCK;
    const int shm = __builtin_amdgcn_readfirstlane(src_m.a0);
    RawChunks<1> in_r[RPW], in_m[8];
    if (!DMA) {
#pragma unroll
      for (int j = 0; j < RPW; j++) {
        const int pos0 = src_r.a0 + (wave + WAVES_PER_BLOCK * j) * LD;
        in_r[j] = load_raw<1>(src_r, pos0 + 16 * lane, 0);
      }
#pragma unroll
      for (int j = 0; j < 8; j++) {
        const int i = tid * 16 + j * BLOCK_THREADS * 16;
        in_m[j] = load_raw<1>(src_m, src_m.a0 + i, 0);   // past the row block: next rows or zeros, not written
      }
    }
    wg_barrier();                                    // the previous row block's readers are done (first pass: key arrays built)
    STAMP(1);
    const int a0m = DMA ? __builtin_amdgcn_readfirstlane((int)((unsigned long long)(m + b0 * LD) & 3)) : 0;   // DMA: the m image starts a0m bytes in
    if (DMA) {                                       // every wave's r rows have landed (each waited for its own in its last epilogue)
      dma_m(rb, tid);
      const int a0r = (int)((unsigned long long)(r + b0 * LD) & 3);
      const v4i mk = col_mask16(16 * lane, N);
      int s4[RPW];
#pragma unroll
      for (int j = 0; j < RPW; j++) {                // all reads of the wave's rows before the first write back
        const int row = wave + WAVES_PER_BLOCK * j;
        const unsigned char *slot = stA + row * g.pitchA + 16 * (lane < 2 * g.NT ? lane : 0);
        in_r[j].c[0] = *(const v4i *)slot;
        in_r[j].tail = *(const u32 *)(slot + 16);
        s4[j] = __builtin_amdgcn_readfirstlane((a0r + row * LD) & 3);
      }
#pragma unroll
      for (int j = 0; j < RPW; j++) {
        const int row = wave + WAVES_PER_BLOCK * j;
        v4i v[1];
        shift_raw<1>(in_r[j], s4[j], v);
        if (lane < 2 * g.NT) *(v4i *)(stA + row * g.pitchA + 16 * lane) = v[0] & mk;
      }
    } else {
      const v4i mk = col_mask16(16 * lane, N);
#pragma unroll
      for (int j = 0; j < RPW; j++) {
        const int row = wave + WAVES_PER_BLOCK * j;
        v4i v[1];
        shift_raw<1>(in_r[j], src_r.a0 + row * LD, v);
        if (lane < 2 * g.NT) *(v4i *)(stA + row * g.pitchA + 16 * lane) = v[0] & mk;
      }
      STAMP(16);
#pragma unroll
      for (int j = 0; j < 8; j++) {
        const int i = tid * 16 + j * BLOCK_THREADS * 16;
        v4i v[1];
        shift_raw<1>(in_m[j], shm, v);
        if (i < 32 * LD) *(v4i *)(mimg + i) = v[0];
      }
    }
    STAMP(2);
    wg_barrier();
    STAMP(3);
    sidx = 0;
    // DMA: what a wave does at the start of an epilogue, strip or no strip (every wave walks through every round): wait for its m
    // pieces before the first one, barriers before the first (m image complete) and the last (r stage free of readers), then the
    // request for the next row block's r rows -- in front of this epilogue's stores.
    auto epi_sync = [&]() {
      if (!DMA) return;
      if (sidx == 0) __builtin_amdgcn_s_waitcnt((7 << 4) | (15 << 8));          // vmcnt(0): this wave's m pieces (the loops issue no vector memory operation)
      if (sidx == 0 || sidx == rounds - 1) wg_barrier();
      if (sidx == rounds - 1 && it + 1 < iters) dma_r(rb_next, lane);
    };
    const bool dma_now = DMA && it + 1 < iters;          // (in the last round) r rows of the next row block are in flight behind this epilogue's stores
    for_each_strip<MAXT>(g.NT, DMA ? wave ^ (2 * (int)blockIdx.x >= (int)gridDim.x ? 2 : 0) : wave, [&](int kb0, int nt) {
      // Result register i of a tile is row (i & 3) + 8 (i >> 2) + 4 (lane >> 5), column lane & 31: a per-lane offset
      // plus a wave-uniform (scalar) offset per register; rows past the batch end are dropped by the descriptor.
      // (Packing 4 columns per lane with in-quad transposes and 64-bit stores was measured 8 % slower: the rows are only
      // 2-byte aligned.)
      const int lane_off = (lane >> 5) * 4 * LD + (lane & 31);
      auto epi = [&](auto &lo, auto &hi) {               // arrays of the strip's tiles
        constexpr int NTS = sizeof(lo) / sizeof(lo[0]);
        epi_sync();
        long bb = b0;                                    // descriptors made where they are used: see k_decrypt_m
        asm volatile("" : "+s"(bb));
        const long lf = (B - bb) * LD;
        const __amdgpu_buffer_rsrc_t rs_e = rows_rsrc(e + bb * LD, 2 * lf);
        const __amdgpu_buffer_rsrc_t rs_q = rows_rsrc(want_q ? quotE + bb * LD : e + bb * LD, 2 * lf);
        const unsigned char *m_l = mimg + a0m + 32 * kb0 + lane_off;
        // columns >= N (last tile only) get an offset beyond any descriptor: the hardware drops those lanes, no
        // exec-mask region per store
        int voff[NTS];
#pragma unroll
        for (int t = 0; t < NTS; t++) voff[t] = 32 * (kb0 + t) + (lane & 31) < N ? 2 * lane_off : (int)0x80000000;
        // Stores: a tile register holds row R in lanes 0-31 and row R + 4 in lanes 32-63 (32 columns each), so a store of it
        // writes two 64-byte pieces of two rows.  v_permlane32_swap exchanges the upper half of tile t's register with the
        // lower half of tile t+1's: one register then is ONE row across both tiles, 128 contiguous bytes per store (a whole
        // cache line on rows pitched to 64 elements).  What the store path pays for is the number of lines touched, not
        // the instruction count: 8-byte stores of four rows per lane group were 14 % SLOWER (profiles/archive/r02_ablation_*).
        const int pv0 = 32 * kb0 + lane;                 // column of this lane in a tile pair starting at tile kb0
        auto out = [&](auto wq) {
#pragma unroll
          for (int j = 0; j < 4; j++) {                  // 4 rows per half-wave at a time, across the strip's tiles
            u32 mv[NTS][4];
#pragma unroll
            for (int t = 0; t < NTS; t++)
#pragma unroll
              for (int ii = 0; ii < 4; ii++) mv[t][ii] = m_l[(8 * j + ii) * LD + 32 * t];
            u32 ev[NTS][4], qv[NTS][4];
#pragma unroll
            for (int t = 0; t < NTS; t++)
#pragma unroll
              for (int ii = 0; ii < 4; ii++) {
                ev[t][ii] = (u32)(lo[t][4 * j + ii] + hi[t][4 * j + ii] + (int)mv[t][ii]) & (q - 1);
                qv[t][ii] = (u32)(0 - hi[t][4 * j + ii]) & (q - 1);
              }
#pragma unroll
            for (int t = 0; t + 1 < NTS; t += 2) {       // tile pairs: one row of 64 columns per store
              const int pvoff = pv0 + 32 * t < N ? 2 * lane : (int)0x80000000;
#pragma unroll
              for (int ii = 0; ii < 4; ii++) {
                const auto se = __builtin_amdgcn_permlane32_swap(ev[t][ii], ev[t + 1][ii], false, false);
                const int so = 2 * ((8 * j + ii) * LD + 32 * (kb0 + t));
                {
                  __builtin_amdgcn_raw_buffer_store_b16((u16)se[0], rs_e, pvoff, so, ST_AUX);
                  __builtin_amdgcn_raw_buffer_store_b16((u16)se[1], rs_e, pvoff, so + 8 * LD, ST_AUX);
                  if (decltype(wq)::value) {
                    const auto sq = __builtin_amdgcn_permlane32_swap(qv[t][ii], qv[t + 1][ii], false, false);
                    __builtin_amdgcn_raw_buffer_store_b16((u16)sq[0], rs_q, pvoff, so, ST_AUX);
                    __builtin_amdgcn_raw_buffer_store_b16((u16)sq[1], rs_q, pvoff, so + 8 * LD, ST_AUX);
                  }
                }
              }
            }
            if (NTS & 1) {                               // the odd tile out: two rows of 32 columns per store
              constexpr int t = NTS - 1;
              const int so = 2 * (8 * j * LD + 32 * (kb0 + t));
              {
#pragma unroll
                for (int ii = 0; ii < 4; ii++) {
                  __builtin_amdgcn_raw_buffer_store_b16((u16)ev[t][ii], rs_e, voff[t], so + 2 * ii * LD, ST_AUX);
                  if (decltype(wq)::value) __builtin_amdgcn_raw_buffer_store_b16((u16)qv[t][ii], rs_q, voff[t], so + 2 * ii * LD, ST_AUX);
                }
              }
            }
          }
          // DMA: the row loads are older than the S stores issued since and vector memory operations complete in order: at most
          // min(S, 63) outstanding = the rows have landed (and the S - 63 oldest stores with them).  At the END of the epilogue:
          // the loads have had its whole length (phase stamps: waiting after the second group of rows cost ~3 k cycles).
          constexpr int S = 16 * NTS * (decltype(wq)::value ? 2 : 1), K = S < 63 ? S : 63;
          if (DMA && dma_now && sidx == rounds - 1) __builtin_amdgcn_s_waitcnt((K & 15) | (7 << 4) | (15 << 8) | ((K >> 4) << 14));
        };
        if (want_q) out(std::true_type{}); else out(std::false_type{});
      };
      switch (nt) {
        case 0:                                          // no strip this round: keep the barriers (and this wave's row request) in step
          epi_sync();
          if (DMA && sidx == rounds - 1) __builtin_amdgcn_s_waitcnt((7 << 4) | (15 << 8));   // vmcnt(0): nothing of its own is stored after them
          break;
        case 1: toeplitz_strip<M_ENC, 1>(st0, st0, tb0, tb1, g, kb0, mlow, epi, stamp_iter, 4 + 2 * sidx); break;
        case 2: toeplitz_strip<M_ENC, 2>(st0, st0, tb0, tb1, g, kb0, mlow, epi, stamp_iter, 4 + 2 * sidx); break;
        case 3: toeplitz_strip<M_ENC, 3>(st0, st0, tb0, tb1, g, kb0, mlow, epi, stamp_iter, 4 + 2 * sidx); break;
        case 4: toeplitz_strip<M_ENC, 4>(st0, st0, tb0, tb1, g, kb0, mlow, epi, stamp_iter, 4 + 2 * sidx); break;
        default: break;                                  // MAXT = 4
      }
      sidx++;
    }, DMA);
  }
}

__global__ __launch_bounds__(BLOCK_THREADS, 2) void k_encrypt_m(MGeom g, u32 q, const u16 *__restrict__ h,
                                                             const uint8_t *__restrict__ r,
                                                             const uint8_t *__restrict__ m, long B,
                                                             u16 *__restrict__ e, u16 *__restrict__ quotE) {
  encrypt_m_body<4, false>(g, q, h, r, m, B, e, quotE);
}

__global__ __launch_bounds__(BLOCK_THREADS, 2) void k_encrypt_md(MGeom g, u32 q, const u16 *__restrict__ h,
                                                              const uint8_t *__restrict__ r,
                                                              const uint8_t *__restrict__ m, long B,
                                                              u16 *__restrict__ e, u16 *__restrict__ quotE) {
  encrypt_m_body<4, true>(g, q, h, r, m, B, e, quotE);
}

NTRU_STAMPS_READER(ntru_debug_read_stamps_enc)

// ---- host side ----------------------------------------------------------------------------------------------------------
// Kernel paths (ntru_engine_set_kernel_path): 0 = auto and 5 -> k_encrypt_md where a row fits one direct-to-LDS instruction, else
// k_encrypt_m; 4 -> k_encrypt_m.
int ntru_launch_encrypt_matrix(ntru_engine *eng, int N, int q, int ld, const uint16_t *d_h, const uint8_t *d_r, const uint8_t *d_m,
                               int64_t B, uint16_t *d_e, uint16_t *d_quotE) {
  MGeom mg;
  if (!make_mgeom(eng, N, q, ld, &mg)) return NTRU_NOT_TAKEN;
  const size_t lds = (size_t)32 * mg.tpitch + (size_t)32 * mg.pitchA + (((size_t)32 * ld + 15) & ~(size_t)15) + 16;
  const long nrb = (long)((B + 31) / 32);
  if (lds > 160 * 1024) return NTRU_NOT_TAKEN;
  // The default: the operands reach LDS by direct-to-LDS loads, r of the next row block ahead of the last epilogue's stores:
  // 1.49-1.51 ms against 1.57-1.62 ms per 2^20 at N = 821 on the same device (profiles/archive/r02_ab_direct_to_lds_rows.txt).
  // One direct-to-LDS instruction moves 64 x 16 bytes from the dword at or below a row, and eight of them per thread the m
  // image: a row of (its byte phase) + N > 1024 bytes, or an image of (phase) + 32 ld > 32768 bytes, would lose its last 1-3
  // bytes.  Those shapes (N >= 1022, or ld = 1024, with rows that are not dword-aligned) take k_encrypt_m, whose register
  // staging fetches the extra dword.
  const bool rows_dword_aligned = (ld & 3) == 0 && ((uintptr_t)d_r & 3) == 0, img_dword_aligned = (ld & 3) == 0 && ((uintptr_t)d_m & 3) == 0;
  const bool dma_fits = (N + 3 <= 1024 || (rows_dword_aligned && N <= 1024)) && (32 * ld + 3 <= 32768 || (img_dword_aligned && 32 * ld <= 32768));
  const bool md = eng->path != 4 && dma_fits;
  snprintf(eng->last_kernel, sizeof eng->last_kernel, md ? "k_encrypt_md" : "k_encrypt_m");
  return launch_resident(eng, md ? k_encrypt_md : k_encrypt_m, nrb, BLOCK_THREADS, lds, mg, (u32)q, d_h, d_r, d_m, (long)B, d_e, d_quotE);
}
