// matrix_noise.hip -- the decryption noise of ciphertext rows under ONE private key: product 1 of decryptBits (index.js:111-140),
// a = f * e mod (x^N - 1, q), centred as both lift modes centre it (c_k = a_k > q/2 ? a_k - q : a_k) and reduced to two numbers per
// row: peak = max_k |c_k| (uint16_t) and energy = sum_k c_k^2 (uint64_t).  a is byte for byte the rem1 of ntru_decrypt_batch; nothing
// here depends on p, fp or the lift mode.  The kernels, the *_dev entry points and the host-pointer forms, for dense and packed rows.
//
// k_noise_m (q <= 8192, N <= 1024, kernel paths 0 with N >= 64, 4 and 5: wherever the shared-key decrypt runs on the matrix cores):
// k_decrypt_m's product 1 -- e = e_lo + 128 e_hi staged as [e_lo | 2 e_hi], planes [f ; 64 f], toeplitz_strip<M_DEC1> of
// matrix_common.h -- with an epilogue that stores no rows.  Per accumulator register (one row, one column per lane and tile) it
// forms x = (low + high) & (q - 1), zero for the junk columns >= N, and c = min(x, q - x) = |centred x|; it folds max c and
// sum c^2 over the strip's tiles (at most 4 (q/2)^2 <= 2^26 per lane), then over the 32 lanes of each half-wave (<= 2^31: a u32).
// The lane fold is a halving exchange on ds_swizzle (no LDS memory, no atomics -- see matrix_decrypt.hip on k_decrypt_mp's first
// version): the lanes of a pair split the registers between them, so 16 registers x 32 lanes take 8 + 4 + 2 + 1 + 1 exchanges per
// quantity instead of 16 x 5.  One (max, sum) pair per row and strip goes to an LDS array [8 strips][32 rows]; behind the barrier
// that ends the row block's strips 32 threads fold the strips that exist and store 2 + 8 bytes per row through descriptors sized by
// the rows left.  tools/mfma_model.py (noise_*) is the executable specification of the epilogue.
//
// Everything else -- q > 8192, N > 1024, N < 64 on path 0, kernel paths 1-3 -- runs ntru_launch_decrypt_valu (p = 3 against a zero
// fp) for its rem1 into the engine-owned scratch, in passes of at most 65536 rows, and reduces the pass with k_noise_rows (one
// wavefront per row): correct, not fast.  The packed forms unpack a pass into scratch first (k_unpack_rows), on either route.
#include "matrix_common.h"

namespace {

constexpr int NOISE_MAX_STRIPS = 8;          // for_each_strip<4>: NT <= 32 tiles are at most two rounds of four strips
constexpr int64_t NOISE_PASS = 65536;        // rows per pass of everything that goes through scratch
static_assert(NOISE_MAX_STRIPS * 4 >= 1024 / 32 && NOISE_MAX_STRIPS % WAVES_PER_BLOCK == 0, "a slot per strip of the widest row");

// The value of lane (lane ^ X) of the same half-wave.
template <int X>
__device__ __forceinline__ u32 noise_xchg(u32 v) { return (u32)__builtin_amdgcn_ds_swizzle((int)v, (X << 10) | 0x1F); }

// One halving step over the lane pairs (l, l ^ 2H): the lane with that bit clear keeps registers 0 .. H-1 and gives H .. 2H-1 away, its
// partner the other way round; both end with H registers folded over the pair, so register bit log2(H) has become lane bit log2(2H).
template <int H>
__device__ __forceinline__ void noise_halve(u32 (&mx)[16], u32 (&sq)[16], int lane) {
  const bool up = (lane & (2 * H)) != 0;
#pragma unroll
  for (int k = 0; k < H; k++) {
    const u32 keep_m = up ? mx[k + H] : mx[k], give_m = up ? mx[k] : mx[k + H];
    const u32 keep_s = up ? sq[k + H] : sq[k], give_s = up ? sq[k] : sq[k + H];
    const u32 got_m = noise_xchg<2 * H>(give_m), got_s = noise_xchg<2 * H>(give_s);
    mx[k] = keep_m > got_m ? keep_m : got_m;
    sq[k] = keep_s + got_s;
  }
}

__global__ __launch_bounds__(BLOCK_THREADS, 2) void k_noise_m(MGeom g, u32 q, const int8_t *__restrict__ f, const u16 *__restrict__ e, long B,
                                                             u16 *__restrict__ peak, unsigned long long *__restrict__ energy) {
  extern __shared__ __attribute__((aligned(16))) unsigned char lds[];
  // LDS: [2 e_hi stage][e_lo stage][key array of f][max per strip and row][sum per strip and row]
  unsigned char *stHi = lds, *stLo = stHi + 32 * g.pitchA;
  u32 *TF = (u32 *)(stLo + 32 * g.pitchA), *smax = TF + 4 * g.tpitch, *ssum = smax + 32 * NOISE_MAX_STRIPS;
  const int lane0 = threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
  build_toeplitz_array(TF, g, [&](int i) { return (int)f[i]; }, (int)threadIdx.x, BLOCK_THREADS);
  const long nrb = (B + 31) >> 5;
  const int nch = 2 * g.NT;
  const u32 qm2 = (q - 1) * 0x00010001u;
  // for_each_strip's cut: strip j = 4 rho + (the wave as it swaps them) exists for j < min(NT, 4 rounds); slot j is strip j's
  const int rounds = (((g.NT + 3) >> 2) + WAVES_PER_BLOCK - 1) / WAVES_PER_BLOCK;
  const int nstrips = g.NT < rounds * WAVES_PER_BLOCK ? g.NT : rounds * WAVES_PER_BLOCK;
  const int swave = wave ^ (2 * blockIdx.x >= gridDim.x ? 2 : 0);
  for (long rb = blockIdx.x; rb < nrb; rb += gridDim.x) {
    // what follows from the lane is made again in every trip (see k_encrypt_m)
    int lane = lane0, N = g.N, LD = g.ld;
    asm volatile("" : "+v"(lane), "+s"(N), "+s"(LD));
    const u32 *tbf = frag_lane_base(TF, g, lane);
    const unsigned char *st0 = stLo + (lane & 31) * g.pitchA + 16 * (lane >> 5);
    const unsigned char *st1 = stHi + (lane & 31) * g.pitchA + 16 * (lane >> 5);
    u32 mlow[4];
    diag_low_mask(lane, mlow);
    const long b0 = rb << 5, left = (B - b0) * LD;
    const AlignedSrc src = aligned_src(e + b0 * LD, 2 * left);
    // staging as in decrypt_m_body: a wave takes one row at a time, lane = 16 coefficients read as aligned 16-byte chunks and shifted
    // in registers; rows behind B read as zero.  No barrier in front: the one that ended the row block before (below) is behind every
    // read of the stages, and its fold has left the slots before this trip's strips write them (they come after the next barrier).
    constexpr int RPW = 32 / WAVES_PER_BLOCK;
    RawChunks<2> raw[RPW];
    int sh[RPW];
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
    __syncthreads();                                     // stages (and, the first time, the key array) complete
    int sidx = 0;                                        // this wave's round of strips: starts again with every row block
    for_each_strip<4>(g.NT, wave, [&](int kb0, int nt) {
      auto epi = [&](auto &lo, auto &hi) {
        constexpr int NTS = sizeof(lo) / sizeof(lo[0]);
        u32 qm[NTS];                                     // a junk column (>= N) counts as x = 0: it reaches neither the maximum nor the sum
#pragma unroll
        for (int t = 0; t < NTS; t++) qm[t] = 32 * (kb0 + t) + (lane & 31) < N ? q - 1 : 0u;
        u32 mx[16], sq[16];                              // register i: row (i & 3) + 8 (i >> 2) (+ 4 in the upper half-wave)
#pragma unroll
        for (int i = 0; i < 16; i++) {
          mx[i] = 0;
          sq[i] = 0;
#pragma unroll
          for (int t = 0; t < NTS; t++) {
            const u32 x = (u32)(lo[t][i] + hi[t][i]) & qm[t], y = q - x;
            const u32 c = x < y ? x : y;                 // x > q/2 ? q - x : x, and x = q/2 stays q/2
            mx[i] = mx[i] > c ? mx[i] : c;
            sq[i] += __umul24(c, c);
          }
        }
        noise_halve<8>(mx, sq, lane);
        noise_halve<4>(mx, sq, lane);
        noise_halve<2>(mx, sq, lane);
        noise_halve<1>(mx, sq, lane);
        const u32 om = noise_xchg<1>(mx[0]), os = noise_xchg<1>(sq[0]);
        const u32 m = mx[0] > om ? mx[0] : om, s = sq[0] + os;
        const int i = (lane & 31) >> 1, row = (i & 3) + 8 * (i >> 2) + 4 * (lane >> 5), slot = 32 * (WAVES_PER_BLOCK * sidx + swave) + row;
        if ((lane & 1) == 0) {
          smax[slot] = m;
          ssum[slot] = s;
        }
      };
      switch (nt) {
        case 1: toeplitz_strip<M_DEC1, 1>(st0, st1, tbf, tbf, g, kb0, mlow, epi); break;
        case 2: toeplitz_strip<M_DEC1, 2>(st0, st1, tbf, tbf, g, kb0, mlow, epi); break;
        case 3: toeplitz_strip<M_DEC1, 3>(st0, st1, tbf, tbf, g, kb0, mlow, epi); break;
        default: toeplitz_strip<M_DEC1, 4>(st0, st1, tbf, tbf, g, kb0, mlow, epi); break;
      }
      sidx++;
    });
    __syncthreads();                                     // every wave is done with the stages; the slots of the strips that exist are written
    if (threadIdx.x < 32) {
      const int r = (int)threadIdx.x;
      u32 m = 0;
      unsigned long long s = 0;
      for (int j = 0; j < nstrips; j++) {                // a wave without a strip (NT < 4) has no slot in this range
        const u32 mj = smax[32 * j + r];
        m = m > mj ? m : mj;
        s += ssum[32 * j + r];
      }
      const long rows_left = B - b0;                     // rows behind B drop out at the descriptors, as everywhere else
      const __amdgpu_buffer_rsrc_t rs_p = rows_rsrc(peak ? peak + b0 : nullptr, peak ? 2 * rows_left : 0);
      const __amdgpu_buffer_rsrc_t rs_e = rows_rsrc(energy ? energy + b0 : nullptr, energy ? 8 * rows_left : 0);
      __builtin_amdgcn_raw_buffer_store_b16((u16)m, rs_p, 2 * r, 0, ST_AUX);
      __builtin_amdgcn_raw_buffer_store_b64((v2u){(u32)s, (u32)(s >> 32)}, rs_e, 8 * r, 0, ST_AUX);
    }
  }
}

// rem [B][N] (a = f * e mod q, reduced) -> peak [B], energy [B]; one wavefront per row.
__global__ __launch_bounds__(BLOCK_THREADS) void k_noise_rows(const u16 *__restrict__ rem, int N, u32 q, long B, u16 *__restrict__ peak,
                                                             unsigned long long *__restrict__ energy) {
  const int lane = threadIdx.x & 63;
  const long wv = (long)blockIdx.x * WAVES_PER_BLOCK + (threadIdx.x >> 6), nwv = (long)gridDim.x * WAVES_PER_BLOCK;
  for (long b = wv; b < B; b += nwv) {
    const u16 *row = rem + b * N;
    u32 m = 0;
    unsigned long long s = 0;                            // q = 65536: one c^2 reaches 2^30
    for (int k = lane; k < N; k += 64) {
      const u32 x = row[k] & (q - 1), y = q - x, c = x < y ? x : y;
      m = m > c ? m : c;
      s += (unsigned long long)c * c;
    }
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) {
      const u32 om = (u32)__shfl_xor((int)m, d, 64);
      m = m > om ? m : om;
      s += __shfl_xor(s, d, 64);
    }
    if (lane == 0) {
      if (peak) peak[b] = (u16)m;
      if (energy) energy[b] = s;
    }
  }
}

// The argument checks of the four forms, before the engine is looked at; `rows` is the dense or the packed array, row_bytes its row.
int check_noise(const std::string &who, const ntru_engine *eng, int N, int q, const int8_t *f, const void *rows, const char *rows_name,
                int64_t B, const uint16_t *peak, const uint64_t *energy, size_t *row_bytes, bool packed) {
  if (B < 0) return fail(NTRU_ERR_ARG, who + "negative batch size");
  if (N < 2 || N > NTRU_MAX_N || q < 2 || q > 65536 || !is_pow2(q))
    return fail(NTRU_ERR_UNSUPPORTED, who + "unsupported (N, q): need 2 <= N <= " + std::to_string(NTRU_MAX_N) + " and q a power of two with 2 <= q <= 65536");
  *row_bytes = (size_t)N * 2;
  if (packed) {
    int bits, per, al, os;
    if (int rc = ntru_pack_params(q - 1, N, &bits, &per, &al, &os)) return rc;
    *row_bytes = (size_t)os * 32;
  }
  if (B > 0 && (!f || !rows)) return fail(NTRU_ERR_ARG, who + "NULL buffer (" + (!f ? "f" : rows_name) + ")");
  if (!peak && !energy) return fail(NTRU_ERR_ARG, who + "peak and energy are both NULL: nothing to compute");
  if (((uintptr_t)energy & 7) != 0) return fail(NTRU_ERR_ARG, who + "energy must be 8-byte aligned");
  const size_t in = (size_t)B * *row_bytes, pk = (size_t)B * 2, en = (size_t)B * 8;
  if (ntru_ranges_overlap(peak, pk, rows, in)) return fail(NTRU_ERR_ARG, who + "peak overlaps " + rows_name);
  if (ntru_ranges_overlap(peak, pk, f, (size_t)N)) return fail(NTRU_ERR_ARG, who + "peak overlaps f");
  if (ntru_ranges_overlap(energy, en, rows, in)) return fail(NTRU_ERR_ARG, who + "energy overlaps " + rows_name);
  if (ntru_ranges_overlap(energy, en, f, (size_t)N)) return fail(NTRU_ERR_ARG, who + "energy overlaps f");
  if (ntru_ranges_overlap(peak, pk, energy, en)) return fail(NTRU_ERR_ARG, who + "peak overlaps energy");
  if (!eng) return fail(NTRU_ERR_ARG, "engine is NULL");
  return NTRU_OK;
}

// Whether k_noise_m takes (N, q): make_mgeom's range for dense rows, and the stages, the key array and the slots in LDS.
bool noise_matrix(const ntru_engine *eng, int N, int q, MGeom *mg, size_t *lds) {
  if (!make_mgeom(eng, N, q, N, mg)) return false;
  *lds = (size_t)64 * mg->pitchA + (size_t)16 * mg->tpitch + (size_t)8 * 32 * NOISE_MAX_STRIPS;
  return *lds <= 160 * 1024;
}

// Enqueues the reduction for B >= 1 rows, dense (d_e) or packed (d_packed, d_e NULL).
int launch_noise(ntru_engine *eng, int N, int q, const int8_t *d_f, const uint16_t *d_e, const uint64_t *d_packed, size_t packed_row,
                 int64_t B, uint16_t *d_peak, uint64_t *d_energy) {
  HIP_TRY(hipSetDevice(eng->device));
  MGeom mg;
  size_t lds = 0;
  const bool matrix = noise_matrix(eng, N, q, &mg, &lds);
  auto run_matrix = [&](const uint16_t *rows, int64_t n, uint16_t *pk, uint64_t *en) {
    note_kernel(eng, "k_noise_m");
    return launch_resident(eng, k_noise_m, (long)((n + 31) / 32), BLOCK_THREADS, lds, mg, (u32)q, d_f, (const u16 *)rows, (long)n, (u16 *)pk,
                           (unsigned long long *)en);
  };
  if (matrix && d_e) return run_matrix(d_e, B, d_peak, d_energy);
  // everything else goes through scratch pass by pass: the unpacked rows, and on the slow route rem1, value and a zero fp
  const int64_t pass = std::min(B, NOISE_PASS);
  Carve c;
  const size_t unp_at = d_e ? 0 : c.take((size_t)pass * N * 2);
  const size_t rem_at = matrix ? 0 : c.take((size_t)pass * N * 2), val_at = matrix ? 0 : c.take((size_t)pass * N), fp_at = matrix ? 0 : c.take((size_t)N);
  ScratchHold hold(eng, c.total);
  if (hold.rc) return hold.rc;
  uint16_t *rows = (uint16_t *)(hold.p + unp_at), *rem = (uint16_t *)(hold.p + rem_at);
  uint8_t *val = (uint8_t *)(hold.p + val_at), *fp = (uint8_t *)(hold.p + fp_at);
  if (!matrix) HIP_TRY(hipMemsetAsync(fp, 0, (size_t)N, eng->stream));
  if (int rc = for_each_pass(B, pass, [&](int64_t o, int64_t n) -> int {
        const uint16_t *src = d_e ? d_e + o * N : rows;
        if (!d_e)
          if (int rc = ntru_launch_unpack_rows(eng, N, q, (const uint64_t *)((const char *)d_packed + (size_t)o * packed_row), n, rows)) return rc;
        if (matrix) return run_matrix(src, n, rows_at(d_peak, o), rows_at(d_energy, o));
        if (int rc = ntru_launch_decrypt_valu(eng, N, q, 3, d_f, fp, src, n, val, nullptr, rem, nullptr)) return rc;
        hipLaunchKernelGGL(k_noise_rows, elementwise_grid(eng, (long)n * 64), dim3(BLOCK_THREADS), 0, eng->stream, (const u16 *)rem, N, (u32)q, (long)n,
                           (u16 *)rows_at(d_peak, o), (unsigned long long *)rows_at(d_energy, o));
        HIP_TRY(hipGetLastError());
        return NTRU_OK;
      }))
    return rc;
  if (!matrix) {                                         // last_kernel: the product's kernel inside the slow route
    char inner[sizeof eng->last_kernel];
    snprintf(inner, sizeof inner, "%s", eng->last_kernel);
    snprintf(eng->last_kernel, sizeof eng->last_kernel, "noise_rows(%.48s)", inner);
  }
  return NTRU_OK;
}

}  // namespace

extern "C" int ntru_noise_batch_dev(ntru_engine_t *eng, int N, int q, const int8_t *d_f, const uint16_t *d_e, int64_t B, uint16_t *d_peak,
                                    uint64_t *d_energy) {
  size_t row;
  if (int rc = check_noise("ntru_noise_batch: ", eng, N, q, d_f, d_e, "e", B, d_peak, d_energy, &row, false)) return rc;
  if (B == 0) return NTRU_OK;
  return launch_noise(eng, N, q, d_f, d_e, nullptr, 0, B, d_peak, d_energy);
}

extern "C" int ntru_noise_packed_batch_dev(ntru_engine_t *eng, int N, int q, const int8_t *d_f, const uint64_t *d_packed, int64_t B,
                                           uint16_t *d_peak, uint64_t *d_energy) {
  size_t row;
  if (int rc = check_noise("ntru_noise_packed_batch: ", eng, N, q, d_f, d_packed, "packed", B, d_peak, d_energy, &row, true)) return rc;
  if (B == 0) return NTRU_OK;
  return launch_noise(eng, N, q, d_f, nullptr, d_packed, row, B, d_peak, d_energy);
}

// The rows flow through the chunked pipeline; f goes up with every chunk as a shared input; 2 and 8 bytes per row come down.
static int noise_host(ntru_engine *eng, int N, int q, const int8_t *f, const void *rows, size_t row, bool packed, int64_t B, uint16_t *peak,
                      uint64_t *energy) {
  Pipeline P(eng);
  const int jf = P.in(f, (size_t)N, true), ir = P.in(rows, row), ip = P.out(peak, 2), ie = P.out(energy, 8);
  return P.run(B, ntru_chunk_items(B), [&](int64_t, int64_t n, void **d) {
    return launch_noise(eng, N, q, (const int8_t *)d[jf], packed ? nullptr : (const uint16_t *)d[ir], packed ? (const uint64_t *)d[ir] : nullptr,
                        row, n, (uint16_t *)d[ip], (uint64_t *)d[ie]);
  });
}

extern "C" int ntru_noise_batch(ntru_engine_t *eng, int N, int q, const int8_t *f, const uint16_t *e, int64_t B, uint16_t *peak,
                                uint64_t *energy) {
  size_t row;
  if (int rc = check_noise("ntru_noise_batch: ", eng, N, q, f, e, "e", B, peak, energy, &row, false)) return rc;
  if (B == 0) return NTRU_OK;
  return noise_host(eng, N, q, f, e, row, false, B, peak, energy);
}

extern "C" int ntru_noise_packed_batch(ntru_engine_t *eng, int N, int q, const int8_t *f, const uint64_t *packed, int64_t B, uint16_t *peak,
                                       uint64_t *energy) {
  size_t row;
  if (int rc = check_noise("ntru_noise_packed_batch: ", eng, N, q, f, packed, "packed", B, peak, energy, &row, true)) return rc;
  if (B == 0) return NTRU_OK;
  return noise_host(eng, N, q, f, packed, row, true, B, peak, energy);
}
