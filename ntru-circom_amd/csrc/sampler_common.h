// sampler_common.h -- the device side of the ternary sampler (generateCustomArray, index.js:461-488) that k_sample_ternary
// (ternary_sampler.hip) is made of, one item per LANE: the reciprocal table of `u32 % (i + 1)`, the start row and the Fisher-Yates
// walk over a row of 2-bit symbols in LDS -- and the ChaCha block function, which k_perm_keys (permutation.hip) draws its sort keys
// from as well.
#ifndef NTRU_SAMPLER_COMMON_H
#define NTRU_SAMPLER_COMMON_H

#include "kernels_common.h"

struct ChaChaKey { u32 k[8]; };

// floor(2^32 / d) for 2 <= d < 2048, through the scalar cache (rows of N + 1 >= 2048 take an LDS table instead).
struct RecipTable {
  u32 v[2048];
  constexpr RecipTable() : v() { for (unsigned d = 2; d < 2048; d++) v[d] = (u32)(0x100000000ULL / d); }
};
static __constant__ const RecipTable g_recip = RecipTable();

#define CHACHA_QR(a, b, c, d)                                                          \
  a += b; d ^= a; d = __builtin_rotateleft32(d, 16); c += d; b ^= c; b = __builtin_rotateleft32(b, 12); \
  a += b; d ^= a; d = __builtin_rotateleft32(d, 8);  c += d; b ^= c; b = __builtin_rotateleft32(b, 7);

// The ChaCha block function of RFC 8439 with DR double rounds (10 = ChaCha20): ks = the 16 keystream words of block `ctr` under `key`
// and nonce (n0, n1, n2).
template <int DR>
static __device__ __forceinline__ void chacha_block(const ChaChaKey &key, u32 ctr, u32 n0, u32 n1, u32 n2, u32 (&ks)[16]) {
  u32 x0 = 0x61707865u, x1 = 0x3320646eu, x2 = 0x79622d32u, x3 = 0x6b206574u;
  u32 x4 = key.k[0], x5 = key.k[1], x6 = key.k[2], x7 = key.k[3], x8 = key.k[4], x9 = key.k[5], x10 = key.k[6],
      x11 = key.k[7], x12 = ctr, x13 = n0, x14 = n1, x15 = n2;
#pragma unroll
  for (int r = 0; r < DR; r++) {
    CHACHA_QR(x0, x4, x8, x12) CHACHA_QR(x1, x5, x9, x13) CHACHA_QR(x2, x6, x10, x14) CHACHA_QR(x3, x7, x11, x15)
    CHACHA_QR(x0, x5, x10, x15) CHACHA_QR(x1, x6, x11, x12) CHACHA_QR(x2, x7, x8, x13) CHACHA_QR(x3, x4, x9, x14)
  }
  ks[0] = x0 + 0x61707865u; ks[1] = x1 + 0x3320646eu; ks[2] = x2 + 0x79622d32u; ks[3] = x3 + 0x6b206574u;
  ks[4] = x4 + key.k[0]; ks[5] = x5 + key.k[1]; ks[6] = x6 + key.k[2]; ks[7] = x7 + key.k[3];
  ks[8] = x8 + key.k[4]; ks[9] = x9 + key.k[5]; ks[10] = x10 + key.k[6]; ks[11] = x11 + key.k[7];
  ks[12] = x12 + ctr; ks[13] = x13 + n0; ks[14] = x14 + n1; ks[15] = x15 + n2;
}
#undef CHACHA_QR

constexpr u32 SAMPLER_NONCE2 = 0x4e545255u;             // "NTRU": the third nonce word of every item

// word w (symbols 16 w .. 16 w + 15) of the start row [1]*n1 ++ [2]*n2 ++ [0]*...
static __device__ __forceinline__ u32 sampler_start_word(int w, int n1, int n2) {
  auto below = [](int k) { return k <= 0 ? 0u : (k >= 16 ? 0xFFFFFFFFu : (1u << (2 * k)) - 1u); };   // symbols 0 .. k-1 of a word
  const u32 m1 = below(n1 - 16 * w), m2 = below(n1 + n2 - 16 * w);
  return (0x55555555u & m1) | (0xAAAAAAAAu & m2 & ~m1);
}

// One row per lane, already holding the start row: for i = N-1 .. 1: j = u32 % (i+1), swap, the u32 of step t being word t of the
// keystream of DR double rounds (10 = ChaCha20) under `key` with nonce (n0, nn1, nn2) = (item_lo, item_hi, "NTRU").  col = the lane's
// column of the rows region ([NW][64] dwords of 16 symbols: word w at col[64 w]); reciprocals floor(2^32 / d) from g_recip, or from
// recip_l[d] when BIGN.  i is the same in every lane (a uniform loop): the word that holds position i stays in a register until i
// leaves it, u32 % (i+1) is a multiply by the reciprocal, one 24-bit multiply-subtract (the remainder is below 2d < 2^24, so the
// product is only needed modulo 2^24) and one correction -- instead of a 35-instruction division.
template <bool BIGN, int DR>
static __device__ __forceinline__ void sampler_shuffle_row(u32 *col, int N, const ChaChaKey &key, u32 n0, u32 nn1, u32 nn2,
                                                           const u32 *recip_l) {
  auto recip_of = [&](int d) -> u32 { return d < 2 ? 0u : (BIGN ? recip_l[d] : g_recip.v[d]); };
  int i = N - 1;
  u32 a = col[64 * (i >> 4)];                          // the word that holds position i
  for (u32 ctr = 0; i >= 1; ctr++) {                  // i is the same in every lane: uniform loop
    u32 rc[16];
    if (!BIGN) {                                       // requested now, needed after the rounds
#pragma unroll
      for (int w = 0; w < 16; w++) rc[w] = recip_of(i + 1 - w);
    }
    u32 ks[16];
    chacha_block<DR>(key, ctr, n0, nn1, nn2, ks);
#pragma unroll
    for (int w = 0; w < 16; w++) {
      if (i >= 1) {
        const u32 d = (u32)(i + 1);
        const u32 hi = __umulhi(ks[w], BIGN ? recip_of((int)d) : rc[w]);
        u32 j;                                                         // ks - hi d is in [0, 2d): its low 24 bits are all of it
        asm("v_mad_i32_i24 %0, %1, %2, %3" : "=v"(j) : "v"(hi), "s"(0 - (int)d), "v"(ks[w]));
        j &= 0xFFFFFFu;
        j = min(j, j - d);
        const int wi = i >> 4, si = 2 * (i & 15), wj = (int)(j >> 4), sj = 2 * (int)(j & 15);
        const u32 bl = col[64 * wj];
        const bool same = wj == wi;
        const u32 b = same ? a : bl;
        const u32 x = ((a >> si) ^ (b >> sj)) & 3u;                    // swap two 2-bit fields by their difference
        a ^= x << si;
        const u32 nb = (same ? a : b) ^ (x << sj);
        col[64 * wj] = nb;
        a = same ? nb : a;
        i--;
        if ((i & 15) == 15) {                                          // uniform: position i has moved into the word below
          col[64 * wi] = a;
          a = col[64 * (i >> 4)];
        }
      }
    }
  }
  col[0] = a;                                          // i == 0: the register copy of word 0 (N == 1: unchanged)
}

#endif
