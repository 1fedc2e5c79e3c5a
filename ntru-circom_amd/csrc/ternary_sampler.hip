// ternary_sampler.hip -- MI355X (gfx950): the on-device ternary sampler, generateCustomArray (index.js:461-488) for one item per LANE:
// k_sample_ternary, its two launchers (consecutive stream positions; the positions of a device list) and ntru_sample_ternary_dev.
//
// Same procedure as the reference: [1]*n1 ++ [other]*n2 ++ [0]*..., then for i = N-1 .. 1: j = u32 % (i+1), swap.
// The u32 of step t of item b is word t of the ChaCha20 keystream (RFC 8439 block function) under the caller's key with
// nonce (b_lo, b_hi, "NTRU"), so any host can replay it with a stock ChaCha20.  The Fisher-Yates chain is inherently
// sequential per item, so items are spread over lanes.  A lane's row lives in LDS as 2-bit symbols (0, 1, 2 = `other`),
// 16 per dword, laid out [word][lane]: whatever word a lane touches, it is in the lane's own bank.  13 KB per wave at
// N = 821 -> 12 waves per CU, and the launcher asks for as much LDS as makes the resident count a MULTIPLE OF FOUR: the
// kernel is bound by vector issue, every workgroup is one wave, and 9 waves on 4 SIMDs (what the round-2 layout with its
// per-wave reciprocal table got) left three SIMDs idle a third of the time (profiles/archive/r03_ablation_sampler.txt).
// A workgroup is WAVES = 4 independent waves (no barrier, private LDS regions) wherever four rows regions fit the LDS: as TWELVE
// single-wave workgroups per CU the same kernel took 3.4 ms per 2^20 items at N = 821, as three four-wave workgroups 2.2 ms
// (profiles/archive/r03_ab_sampler.txt; the inversion kernel, eight single-wave workgroups per CU, does not care: more than eight workgroups
// per CU do not seem to be resident together, whatever the occupancy query says).
// The block function, reciprocal table, start row and shuffle walk are in sampler_common.h.
#include "sampler_common.h"

// Which stream position row k of a launch of B rows draws (Items, handed to the kernel by value).
struct ConsecutiveItems {                    // first_item + k; lanes past B draw the positions that follow and store nothing
  unsigned long long first_item;
  __device__ unsigned long long position(long k, long) const { return first_item + (unsigned long long)k; }
};
struct ListedItems {                         // pos_base + idx[k], idx a device list of B items; lanes past B draw a copy of the last one
  unsigned long long pos_base;
  const u32 *idx;
  __device__ unsigned long long position(long k, long B) const { return pos_base + idx[k < B ? k : B - 1]; }
};

// DR: double rounds of the block function: 10 = ChaCha20 (RFC 8439, the default), 6 = ChaCha12, 4 = ChaCha8 (ntru_engine_set_sampler_rounds:
// the kernel is bound by the vector issue of these rounds; generateCustomArray's contract is the shuffle and its `u32 % (i + 1)` draws,
// not the generator behind them, and a host replays whichever variant it asked for).
template <bool BIGN, int WAVES, int DR, class Items>     // BIGN: N + 1 >= 2048, reciprocals from an LDS table behind the rows
__global__ __launch_bounds__(WAVES * 64) void k_sample_ternary(int N, int n1, int n2, u32 other, ChaChaKey key, Items items, long B,
                                                               uint8_t *__restrict__ out, int NW) {
  extern __shared__ __attribute__((aligned(16))) unsigned char lds[];
  const int lane = threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
  const size_t per_wave = (size_t)NW * 64 + (BIGN ? (size_t)((N + 2) & ~1) : 0);     // dwords
  u32 *rows = (u32 *)lds + wave * per_wave;              // [NW][64] dwords of 16 symbols
  u32 *recip_l = rows + (size_t)NW * 64;                 // BIGN: [N + 1]
  if (BIGN) {
    for (int d = lane; d <= N; d += 64) recip_l[d] = d >= 2 ? (u32)(0x100000000ULL / (unsigned)d) : 0u;
    wave_lds_fence();
  }
  u32 *col = rows + lane;                                // word w of this lane's row: col[64 w]
  const bool out_aligned = (((unsigned long long)out) & 15) == 0 && N >= 16;
  for (long base = ((long)blockIdx.x * WAVES + wave) * 64; base < B; base += (long)gridDim.x * WAVES * 64) {
    for (int w = 0; w < NW; w++) col[64 * w] = sampler_start_word(w, n1, n2);
    const unsigned long long item = items.position(base + lane, B);
    sampler_shuffle_row<BIGN, DR>(col, N, key, (u32)item, (u32)(item >> 32), SAMPLER_NONCE2, recip_l);
    wave_lds_fence();
    if (out_aligned && base + 64 <= B) {
      // rows -> row-major byte output.  The 64 rows of the block are ONE contiguous run of 64 N bytes that starts on a 64-byte
      // boundary: lane L writes the 16-byte pieces of bytes [S L, S L + S), S = 16 NW >= N, i.e. the end of row ~L and the start of
      // row ~L + 1 (distinct rows per lane: distinct LDS banks), every store aligned; 64 N is a multiple of 16, so a piece is
      // inside the run or outside it.
      const u32 S = 16u * (u32)NW, a0 = S * (u32)lane, run = 64u * (u32)N;
      u32 r = a0 / (u32)N, c = a0 - r * (u32)N;
      uint4 *dst = (uint4 *)(out + (size_t)base * N) + (size_t)NW * lane;
      for (int it = 0; it < NW; it++) {
        if (a0 + 16u * (u32)it < run) {
          const u32 *rp = rows + r;
          const int w = (int)(c >> 4), w1i = w + 1 < NW ? w + 1 : w;
          u32 bits = __builtin_amdgcn_alignbit(rp[64 * w1i], rp[64 * w], 2 * (c & 15));
          const int nf = N - (int)c;                     // symbols of row r from c on (>= 1)
          if (nf < 16) bits = (bits & ((1u << (2 * nf)) - 1u)) | (rows[r + 1] << (2 * nf));   // the piece continues in row r + 1
          u32 o[4];
#pragma unroll
          for (int q = 0; q < 4; q++) {
            u32 t = unpack2x4(bits >> (8 * q));
            if (other != 2u) t += ((t >> 1) & 0x01010101u) * (other - 2u);
            o[q] = t;
          }
          dst[it] = make_uint4(o[0], o[1], o[2], o[3]);
        }
        c += 16;
        if (c >= (u32)N) { c -= (u32)N; r++; }
      }
    } else {
      // any alignment, partial last block: the wave walks one row at a time, one byte per lane
      for (int rr = 0; rr < 64; rr++) {
        if (base + rr >= B) break;
        uint8_t *dst = out + (size_t)(base + rr) * N;
        const u32 *src = rows + rr;
        for (int k = lane; k < N; k += 64) {
          const u32 sym = (src[64 * (k >> 4)] >> (2 * (k & 15))) & 3u;
          dst[k] = (uint8_t)(sym == 2u ? other : sym);
        }
      }
    }
    wave_lds_fence();
  }
}

// LDS bytes of a workgroup: per wave the rows, NW = ceil(N / 16) dwords of 16 symbols for each of 64 lanes, and behind them, BIGN,
// the N + 1 reciprocals (an even number of dwords).
static size_t sampler_lds_bytes(bool bign, int waves, int N) {
  return waves * ((size_t)64 * ((N + 15) / 16) * 4 + (bign ? (size_t)((N + 2) & ~1) * 4 : 0));
}

template <bool BIGN, int WAVES, int DR, class Items>
static int launch_sampler(ntru_engine *eng, int N, int n1, int n2, int other, const uint32_t *key, Items items, int64_t B,
                          uint8_t *d_out) {
  const size_t lds = sampler_lds_bytes(BIGN, WAVES, N);
  if (lds > 160 * 1024) return fail(NTRU_ERR_UNSUPPORTED, "N too large for the sampler's LDS rows");
  ChaChaKey ck;
  memcpy(ck.k, key, 32);
  note_kernel(eng, "k_sample_ternary");
  return launch_resident(eng, k_sample_ternary<BIGN, WAVES, DR, Items>, (B + WAVES * 64 - 1) / (WAVES * 64), WAVES * 64, lds, N, n1, n2,
                         (u32)other, ck, items, (long)B, d_out, (N + 15) / 16);
}

// The caller (keygen_batch.hip) has checked N <= NTRU_MAX_N, so N + 1 < 2048: reciprocals from the constant table.  Key material is
// always drawn with ChaCha20, whatever ntru_engine_set_sampler_rounds says.
int ntru_launch_sample_listed(ntru_engine *eng, int N, int n1, int n2, int other, const uint32_t *key, uint64_t pos_base,
                              const uint32_t *d_idx, int n, uint8_t *d_out) {
  return launch_sampler<false, 4, 10>(eng, N, n1, n2, other, key, ListedItems{pos_base, d_idx}, n, d_out);
}

extern "C" int ntru_sample_ternary_dev(ntru_engine_t *eng, int N, int n1, int n2, int other, const uint32_t *key,
                                       uint64_t first_item, int64_t B, uint8_t *d_out) {
  if (!eng) return fail(NTRU_ERR_ARG, "engine is NULL");
  if (B < 0 || N < 1 || n1 < 0 || n2 < 0) return fail(NTRU_ERR_ARG, "negative size");
  if (n1 + n2 > N) return fail(NTRU_ERR_ARG, "The total of 1s and -1s cannot exceed the array length.");   // index.js:463
  if (other < 0 || other > 255) return fail(NTRU_ERR_ARG, "`other` must fit a byte");
  if (!key) return fail(NTRU_ERR_ARG, "ntru_sample_ternary: key is NULL");
  if (B == 0) return NTRU_OK;
  if (!d_out) return fail(NTRU_ERR_ARG, "ntru_sample_ternary: NULL buffer");
  HIP_TRY(hipSetDevice(eng->device));
  const ConsecutiveItems items{first_item};
  auto go = [&](auto dr) -> int {
    constexpr int DR = decltype(dr)::value;
    return N + 1 < 2048 ? launch_sampler<false, 4, DR>(eng, N, n1, n2, other, key, items, B, d_out)     // <= 32 KB of rows per wave
                        : launch_sampler<true, 1, DR>(eng, N, n1, n2, other, key, items, B, d_out);
  };
  switch (eng->sampler_rounds) {
    case 8: return go(std::integral_constant<int, 4>{});
    case 12: return go(std::integral_constant<int, 6>{});
    default: return go(std::integral_constant<int, 10>{});
  }
}
