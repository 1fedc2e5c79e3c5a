// matrix_encrypt_body.h -- the one body of the shared-key encrypt kernels on the matrix cores, shared by matrix_encrypt.hip
// (k_encrypt_m, k_encrypt_md: the epilogue adds a byte row of m, staged as an LDS image) and matrix_reencrypt.hip (k_reencrypt_m,
// k_reencrypt_md: the epilogue adds a gathered 16-bit ciphertext row).  The addend source is the template parameter Add.
#ifndef NTRU_MATRIX_ENCRYPT_BODY_H
#define NTRU_MATRIX_ENCRYPT_BODY_H

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
// Add: where the epilogue's addend comes from.  AddByteImage: the byte rows m, staged as the LDS image described above.
// AddGatherRows16 (m is unused and NULL): output row i takes the 16-bit row src[i] (i itself without src) of e_in, any uint16_t
// value, reduced mod q by the epilogue's mask.  No 32 x ld x 2-byte image of it is staged (that would cost the second workgroup
// per CU).  Instead the element offset of each of the row block's 32 source rows is put into a 256-byte LDS table at the top of the
// trip -- -1 for a row past the batch and for an index outside [0, B_in): such a row is not read at all and adds zero -- and every
// wave stages the columns of its own strip only, ahead of the strip's matrix loop (stage_addend below; 8.5 KB per wave).  Reading
// the addend from global memory in the epilogue instead was measured at 3.68 ms against 1.87 ms per 2^20 rows at N = 821
// (EXPERIMENTS.md "Re-randomising and shuffling": the loads queue behind the epilogue's own stores).  The loads are dword-granular, as
// dma_r's: of a row that IS read, the dword that holds its first and the dword that holds its last element are read whole, so up
// to 2 bytes next to an e_in that is not dword-aligned share an access with it; nothing further away is touched.  An element is
// staged before the wave that staged it stores to it, so e_out may be e_in when src is NULL (in place).  Offsets are 64-bit:
// B_in x N x 2 bytes can pass 4 GB.
// AddCheckLinks (mix_audit.hip: k_linkcheck_m, k_linkcheck_md; e and quotE are NULL): AddGatherRows16 with a compare in the place of the
// stores.  Row l claims e_out[dst[l]] == r[l] * h + e_in[src[l]]: the epilogue forms the sum as the re-encrypt kernels do and XORs it
// with the expected columns, read from global memory where they are used -- this epilogue stores nothing, so the loads do not queue
// behind stores as the addend's did, and a second stage per wave would cost the second workgroup per CU for 1 % at best
// (EXPERIMENTS.md "Auditing a mix" has both timings, and what the direct read costs in latency).  The differences of a
// strip are OR-ed per row by wave ballots into a 32-entry LDS flag table; the row's owner in the r stage tests its bytes and counts
// into a second table; after the last strip one barrier, and lanes 0-31 store the row block's 32 flag bytes at once.  A link with an
// index outside its array reads no row (both offsets -1).  Out-of-domain bytes of r: load_a forms the 32 r plane by shifting the
// dwords of ONE row's fragment, so a carry lands in bytes of the same row of the A operand, and a row of the product depends on that
// row of A alone: the other links of the row block are not disturbed, and the bad row's own product is ignored (NTRU_LINK_BAD_R).
struct AddByteImage { static constexpr bool ROWS16 = false, CHECK = false; };
constexpr int ADD_ROW_PITCH = 272;                        // bytes per staged row segment: 4 tiles x 32 columns x 2 bytes + its dword phase, in 16-byte pieces
constexpr int CHECK_TABLE_BYTES = 512;                   // AddCheckLinks, behind the addend stages: 32 expected-row offsets, 32 flag words, 32 r verdicts
struct AddCheckLinks {
  static constexpr bool ROWS16 = true, CHECK = true;
  const u16 *e_in;
  long B_in;
  const long *src;
  const u16 *e_out;
  long B_out;
  const long *dst;
  int other, n1, n2;                                      // the domain of r: bytes in {0, 1, other}; counts, each -1 = not tested
  uint8_t *flags;
  unsigned long long *n_bad;                              // NULL, or zeroed by the launcher: one atomic per workgroup adds to it
  // element offsets of a link's two rows into in_ofs / out_ofs, both -1 unless both indices are inside their arrays; true: a link of
  // the batch with an index outside
  __device__ __forceinline__ bool link_offsets(long row, long B, int LD, long &in_ofs, long &out_ofs) const {
    in_ofs = out_ofs = -1;
    if (row >= B) return false;
    const long s = src ? src[row] : row, d = dst ? dst[row] : row;
    if ((unsigned long)s >= (unsigned long)B_in || (unsigned long)d >= (unsigned long)B_out) return true;
    in_ofs = s * LD;
    out_ofs = d * LD;
    return false;
  }
  // NTRU_LINK_BAD_R or 0 from a row's totals: bytes outside the domain, ones, bytes equal to `other` (other == 1: the same bytes)
  __device__ __forceinline__ u32 r_verdict(bool outside, int ones, int others) const {
    if (outside) return 2u;
    if (other == 1) return n1 >= 0 && n2 >= 0 && ones != n1 + n2 ? 2u : 0u;
    return (n1 >= 0 && ones != n1) || (n2 >= 0 && others != n2) ? 2u : 0u;
  }
};
struct AddGatherRows16 {
  static constexpr bool ROWS16 = true, CHECK = false;
  const u16 *e_in;
  long B_in;
  const long *src;
  __device__ __forceinline__ long row_offset(long row, long B, int LD) const {
    if (row >= B) return -1;
    const long s = src ? src[row] : row;
    return (unsigned long)s < (unsigned long)B_in ? s * LD : -1;
  }
};

template <int MAXT, bool DMA, class Add = AddByteImage>
static __device__ __forceinline__ void encrypt_m_body(MGeom g, u32 q, const u16 *__restrict__ h,
                                                      const uint8_t *__restrict__ r,
                                                      const uint8_t *__restrict__ m, long B,
                                                      u16 *__restrict__ e, u16 *__restrict__ quotE, Add add = Add()) {
  constexpr bool ROWS16 = Add::ROWS16, CHECK = Add::CHECK;
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
  long *rowtab = (long *)mimg;                           // ROWS16: in its place, the element offsets of the 32 source rows
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
  u32 n_bad_mine = 0;                                    // CHECK: links of this workgroup's row blocks with a flag set (lanes 0-31 of wave 0)
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
  // ROWS16: the addend columns of a wave's own strip, all 32 rows, by direct-to-LDS loads into the wave's own 32 x ADD_ROW_PITCH bytes
  // behind the row table -- requested ahead of the strip's matrix loop and waited for at the top of its epilogue, so the round trip
  // has the loop to hide behind; only this wave reads them back: no workgroup barrier.  One instruction per row, 17 lanes x 16 bytes
  // from the dword at or below the row's first column of the strip (as dma_r); the descriptor ends with the dword that holds the
  // row's last element, and has no bytes at all for a row without an addend.
  unsigned char *stg = mimg + 256 + wave * (32 * ADD_ROW_PITCH);
  // CHECK: behind the four stages, the element offsets of the 32 expected rows, the flag table the epilogues OR into, the verdicts
  // on the rows of r
  long *rowtab2 = (long *)(mimg + 256 + WAVES_PER_BLOCK * (32 * ADD_ROW_PITCH));
  u32 *flagtab = (u32 *)(rowtab2 + 32), *rtab = flagtab + 32;
  auto stage_addend = [&](int kb0, int lane) {
    if constexpr (ROWS16) {
      const long mine = rowtab[lane & 31];
      const u32 olo = (u32)mine, ohi = (u32)((unsigned long)mine >> 32);
      const int left = 2 * (g.N - 32 * kb0);
#pragma unroll
      for (int row = 0; row < 32; row++) {
        const long ro = (long)(((unsigned long)__builtin_amdgcn_readlane(ohi, row) << 32) | __builtin_amdgcn_readlane(olo, row));
        const unsigned long long a = (unsigned long long)(add.e_in + (ro < 0 ? 0 : ro) + 32 * kb0);
        const int a0 = (int)(a & 3);
        const __amdgpu_buffer_rsrc_t rs = rows_rsrc((const void *)(a & ~3ULL), ro < 0 ? 0 : (a0 + left + 3) & ~3);
        if (lane < ADD_ROW_PITCH / 16)
          __builtin_amdgcn_raw_ptr_buffer_load_lds(rs, (__attribute__((address_space(3))) void *)(stg + row * ADD_ROW_PITCH), 16, 16 * lane, 0, 0, 0);
      }
    }
  };
  // CHECK: the row of r a wave has just brought into operand form (16 bytes per lane, columns >= N zero): its bytes outside
  // {0, 1, other} and its counts, summed over the wave; lane 0 files the verdict.  Bytes are classed four at a time: zero_bytes(x)
  // has bit 7 of a byte set exactly where that byte of x is zero.
  auto judge_r = [&](int row, v4i w, int lane) {
    if constexpr (CHECK) {
      auto zero_bytes = [](u32 x) { return ~(((x & 0x7F7F7F7Fu) + 0x7F7F7F7Fu) | x) & 0x80808080u; };
      const u32 oth = 0x01010101u * (u32)add.other;
      int zeros = 0, ones = 0, others = 0;
#pragma unroll
      for (int k = 0; k < 4; k++) {
        zeros += __builtin_popcount(zero_bytes((u32)w[k]));
        ones += __builtin_popcount(zero_bytes((u32)w[k] ^ 0x01010101u));
        others += __builtin_popcount(zero_bytes((u32)w[k] ^ oth));
      }
      const bool outside = zeros + ones + (add.other == 1 ? 0 : others) != 16;
      u32 pair = (u32)ones | ((u32)others << 16);            // each total <= 1024
#pragma unroll
      for (int s = 32; s > 0; s >>= 1) pair += (u32)__shfl_xor((int)pair, s, 64);
      const bool any_outside = __ballot(outside) != 0;
      if (lane == 0) rtab[row] = add.r_verdict(any_outside, (int)(pair & 0xFFFFu), (int)(pair >> 16));
    }
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
      if constexpr (!ROWS16) {
#pragma unroll
        for (int j = 0; j < 8; j++) {
          const int i = tid * 16 + j * BLOCK_THREADS * 16;
          in_m[j] = load_raw<1>(src_m, src_m.a0 + i, 0);   // past the row block: next rows or zeros, not written
        }
      }
    }
    long row_ofs = -1;                               // ROWS16: thread t < 32 looks up source row t of the row block
    long row_ofs2 = -1;                              // CHECK: and the expected row; idx_flag: NTRU_LINK_BAD_INDEX of that link
    u32 idx_flag = 0;
    if constexpr (CHECK) {
      if (tid < 32) idx_flag = add.link_offsets(b0 + tid, B, LD, row_ofs, row_ofs2) ? 1u : 0u;
    } else if constexpr (ROWS16) {
      if (tid < 32) row_ofs = add.row_offset(b0 + tid, B, LD);
    }
    wg_barrier();                                    // the previous row block's readers are done (first pass: key arrays built)
    STAMP(1);
    const int a0m = DMA ? __builtin_amdgcn_readfirstlane((int)((unsigned long long)(m + b0 * LD) & 3)) : 0;   // DMA: the m image starts a0m bytes in
    if constexpr (ROWS16) if (tid < 32) rowtab[tid] = row_ofs;
    if constexpr (CHECK) if (tid < 32) { rowtab2[tid] = row_ofs2; flagtab[tid] = 0; }
    if (DMA) {                                       // every wave's r rows have landed (each waited for its own in its last epilogue)
      if constexpr (!ROWS16) dma_m(rb, tid);
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
        judge_r(row, v[0] & mk, lane);
      }
    } else {
      const v4i mk = col_mask16(16 * lane, N);
#pragma unroll
      for (int j = 0; j < RPW; j++) {
        const int row = wave + WAVES_PER_BLOCK * j;
        v4i v[1];
        shift_raw<1>(in_r[j], src_r.a0 + row * LD, v);
        if (lane < 2 * g.NT) *(v4i *)(stA + row * g.pitchA + 16 * lane) = v[0] & mk;
        judge_r(row, v[0] & mk, lane);
      }
      STAMP(16);
      if constexpr (!ROWS16) {
#pragma unroll
        for (int j = 0; j < 8; j++) {
          const int i = tid * 16 + j * BLOCK_THREADS * 16;
          v4i v[1];
          shift_raw<1>(in_m[j], shm, v);
          if (i < 32 * LD) *(v4i *)(mimg + i) = v[0];
        }
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
      // (ROWS16: there is no m image to wait for)
      if (!ROWS16 && sidx == 0) __builtin_amdgcn_s_waitcnt((7 << 4) | (15 << 8));          // vmcnt(0): this wave's m pieces (the loops issue no vector memory operation)
      if ((!ROWS16 && sidx == 0) || sidx == rounds - 1) wg_barrier();
      if (sidx == rounds - 1 && it + 1 < iters) dma_r(rb_next, lane);
    };
    const bool dma_now = DMA && it + 1 < iters;          // (in the last round) r rows of the next row block are in flight behind this epilogue's stores
    for_each_strip<MAXT>(g.NT, DMA ? wave ^ (2 * (int)blockIdx.x >= (int)gridDim.x ? 2 : 0) : wave, [&](int kb0, int nt) {
      // Result register i of a tile is row (i & 3) + 8 (i >> 2) + 4 (lane >> 5), column lane & 31: a per-lane offset
      // plus a wave-uniform (scalar) offset per register; rows past the batch end are dropped by the descriptor.
      // (Packing 4 columns per lane with in-quad transposes and 64-bit stores was measured 8 % slower: the rows are only
      // 2-byte aligned.)
      const int lane_off = (lane >> 5) * 4 * LD + (lane & 31);
      if (nt > 0) stage_addend(kb0, lane);
      auto epi = [&](auto &lo, auto &hi) {               // arrays of the strip's tiles
        constexpr int NTS = sizeof(lo) / sizeof(lo[0]);
        if constexpr (ROWS16) __builtin_amdgcn_s_waitcnt((7 << 4) | (15 << 8));   // vmcnt(0): the strip's addend has landed (and the stores before it)
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
          u32 bad_rows = 0;                              // CHECK: bit R = row R of the row block differs somewhere in this strip (wave-uniform)
#pragma unroll
          for (int j = 0; j < 4; j++) {                  // 4 rows per half-wave at a time, across the strip's tiles
            u32 mv[NTS][4];
#pragma unroll
            for (int t = 0; t < NTS; t++)
#pragma unroll
              for (int ii = 0; ii < 4; ii++) {
                if constexpr (ROWS16) {
                  const long ro = rowtab[8 * j + ii + 4 * (lane >> 5)];
                  const int col = 32 * (kb0 + t) + (lane & 31);
                  // no exec-mask region per load: a lane without an addend reads h[0] (always there) and drops it
                  // (decided before the read, so that the read stays unconditional: no exec-mask region per element)
                  const bool ok = ro >= 0 && col < N;
                  // the staged segment starts at the dword at or below the row's first column of the strip: 0 or 2 bytes in
                  const int ph = (int)((((unsigned long long)add.e_in >> 1) + (unsigned long long)ro + 32 * kb0) & 1) * 2;
                  const u32 v = *(const u16 *)(stg + (8 * j + ii + 4 * (lane >> 5)) * ADD_ROW_PITCH + ph + 64 * t + 2 * (lane & 31));
                  mv[t][ii] = ok ? v : 0u;
                } else {
                  mv[t][ii] = m_l[(8 * j + ii) * LD + 32 * t];
                }
              }
            u32 ev[NTS][4], qv[NTS][4];
#pragma unroll
            for (int t = 0; t < NTS; t++)
#pragma unroll
              for (int ii = 0; ii < 4; ii++) {
                ev[t][ii] = (u32)(lo[t][4 * j + ii] + hi[t][4 * j + ii] + (int)mv[t][ii]) & (q - 1);
                qv[t][ii] = (u32)(0 - hi[t][4 * j + ii]) & (q - 1);
              }
            if constexpr (CHECK) {
              // the expected columns against the sum; a lane without a link or a column keeps its zero.  One bit per row of
              // the row block: a half-wave holds 32 columns of one row, so a ballot's halves are rows 8 j + ii and 8 j + ii + 4
#pragma unroll
              for (int ii = 0; ii < 4; ii++) {
                const int rw = 8 * j + ii + 4 * (lane >> 5);
                const long ro = rowtab2[rw];
                u32 dd = 0;
#pragma unroll
                for (int t = 0; t < NTS; t++) {
                  const int col = 32 * (kb0 + t) + (lane & 31);
                  const bool ok = ro >= 0 && col < N;
                  // (unconditional, as the staged read above: a lane without a link or a column reads h[0], which is always there)
                  const u32 xv = *(ok ? add.e_out + ro + col : h);
                  dd |= ok ? (ev[t][ii] ^ xv) & (q - 1) : 0u;
                }
                const unsigned long long differ = __ballot(dd != 0);
                bad_rows |= ((u32)differ ? 1u : 0u) << (8 * j + ii) | ((u32)(differ >> 32) ? 1u : 0u) << (8 * j + ii + 4);
              }
            } else {
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
          }
          // DMA: the row loads are older than the S stores issued since and vector memory operations complete in order: at most
          // min(S, 63) outstanding = the rows have landed (and the S - 63 oldest stores with them).  At the END of the epilogue:
          // the loads have had its whole length (phase stamps: waiting after the second group of rows cost ~3 k cycles).
          // CHECK: no stores follow the row loads, so the wait is for all of them; the strip's verdicts go into the flag table
          if constexpr (CHECK)
            if (bad_rows != 0 && lane < 32 && ((bad_rows >> lane) & 1u))
              __hip_atomic_fetch_or(&flagtab[lane], 4u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
          constexpr int S = CHECK ? 0 : 16 * NTS * (decltype(wq)::value ? 2 : 1), K = S < 63 ? S : 63;
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
    if constexpr (CHECK) {
      wg_barrier();                                  // every wave's strips have filed their verdicts
      if (tid < 32) {
        // a bad index or a bad r stands alone: that link's product and rows mean nothing
        const u32 fl = idx_flag | rtab[tid] ? idx_flag | rtab[tid] : flagtab[tid];
        const bool mine = b0 + tid < B;
        if (mine) add.flags[b0 + tid] = (uint8_t)fl;     // 32 bytes side by side: one store per row block
        n_bad_mine += (u32)__builtin_popcountll(__ballot(mine && fl != 0));
      }
    }
  }
  if constexpr (CHECK)                               // one atomic per workgroup
    if (threadIdx.x == 0 && add.n_bad && n_bad_mine) atomicAdd(add.n_bad, (unsigned long long)n_bad_mine);
}

#endif
