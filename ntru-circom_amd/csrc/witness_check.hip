// witness_check.hip -- batched witness checking against the reference's Verify* circuits (circuits/ntru.circom with circomlib
// 2.0.5 LessThan / LessEqThan / IsEqual / IsZero / Num2Bits): VerifyEncrypt, VerifyDecrypt and VerifyInverse, their kernels, the
// *_dev entry points (host-pointer forms: ntru_host.hip).
//
// Every witness entry is an integer in [0, 65536), so no signal leaves [0, 2^43) and the field arithmetic of the templates is
// integer arithmetic.  Each template then reduces to ("Witness checks"):
//   Modulus(M, n)(x)    satisfied iff x < T(M, n) = 2^n + floor((2^n - 1) / (M - 1))   (ltQ: x - floor(x / M) < 2^n)
//                                 and M - 2^n <= y < 2^n for y = x mod M              (ltP, gteZeroY)
//   VerifyDividePolynomials(M, n, 2N - 1, N + 1)(a, 1 + (M - 1) x^N, Q, R):
//                       P_k = [k <= N] (Q_k + R_k) + [k >= N] (M - 1) Q_{k-N}, k = 0..2N, each through Modulus(M, n);
//                       reduced P_k == a_k for k < 2N - 1 (IsEqual), == 0 for k = 2N - 1, 2N (IsZero)
//   a_k = Modulus(M, n)(sum_i A_i W_{k-i} [+ m_k for k < N in VerifyEncrypt]), the LINEAR product.
// VerifyDecrypt's second stage runs the same rule on (fp, b) with b_i = Modulus(p, np)(remainder1[i] + gt_i) and
// gt_i = LessThan(nq)(q / 2, remainder1[i]).
//
// One item per wavefront.  The product needs the exact integer sum (the range rule reads it), so the operands are staged in LDS
// as byte planes and every pair of planes is accumulated exactly in u32 with v_dot4_u32_u8 (one plane sum <= 1920 * 255^2 < 2^27),
// the pairs combined in u64 at the end.  A plane that is zero for the item (the high byte of r in {0,1,2}, of fp, of b) is
// skipped wave-uniformly.  Lane l owns the four consecutive outputs k = K0 + 4 l .. K0 + 4 l + 3 of a pass of 256 outputs; the
// broadcast operand A is read as aligned dwords A[4t .. 4t+3] (every lane the same address), the windowed operand W lies
// reversed behind PAD zero bytes, so that the four windows of a lane are one aligned dword and three byte shifts of the next.
#include <hip/hip_runtime.h>

#include <cstdint>
#include <cstdio>
#include <string>

#include "kernels_common.h"

typedef unsigned long long u64;
typedef unsigned char u8;

namespace {

constexpr int WC_WAVES = 4;
constexpr int WC_THREADS = WC_WAVES * 64;

// Modulus(M, n) of one stage: x < T, ylo <= x mod M <= yhi.  mask = M - 1 when M is a power of two, else 0.
struct Stage {
  u64 T;
  u32 M, mask, ylo, yhi;
};

// LDS geometry of one wavefront's operands (bytes): A planes [alen] each, W planes [vlen] each, W reversed behind pad zeros.
struct Geom {
  int N, alen, pad, vlen;
};

Geom geom_of(int N) {
  Geom g;
  g.N = N;
  g.alen = (N + 3) & ~3;
  g.pad = ((N + 260 + 3) & ~3) - N;      // >= 258 (the lowest window of a pass), pad + N a multiple of 4
  g.vlen = g.pad + N + 260;              // the highest dword pair a pass reads ends below pad + N + 260
  return g;
}

__device__ __forceinline__ u32 mod_m(u64 x, const Stage &s) {
  if (s.mask) return (u32)x & s.mask;
  // the top 32 bits, then two 16-bit Horner steps (each operand below 2^32: r < M <= 65535 here)
  u32 r = (u32)(x >> 32) % s.M;
  r = ((r << 16) | ((u32)x >> 16)) % s.M;
  return ((r << 16) | ((u32)x & 0xffffu)) % s.M;
}

// Modulus(M, n)(x): returns y = x mod M, ORs NTRU_CHECK_RANGE into fl when a range check of the template fails
__device__ __forceinline__ u32 modulus(u64 x, const Stage &s, u32 &fl) {
  const u32 y = mod_m(x, s);
  if (x >= s.T || y < s.ylo || y > s.yhi) fl |= NTRU_CHECK_RANGE;
  return y;
}

__device__ __forceinline__ u32 wave_or(u32 v) {
  u32 r = 0;
  for (int b = 0; b < 6; b++)
    if (__ballot((v >> b) & 1u)) r |= 1u << b;
  return r;
}

// A forward into two byte planes: P0[i] / P1[i] = low / high byte of A_i, zero for N <= i < alen.  Returns 2 when some A_i of the
// item has a nonzero high byte, else 0.
template <class Get>
__device__ __forceinline__ u32 stage_fwd(u32 *P0, u32 *P1, const Geom &g, int lane, Get get) {
  u32 any = 0;
  for (int d = lane; d < g.alen / 4; d += 64) {
    u32 lo = 0, hi = 0;
    for (int b = 0; b < 4; b++) {
      const int i = 4 * d + b;
      const u32 v = i < g.N ? get(i) : 0u;
      lo |= (v & 0xffu) << (8 * b);
      hi |= (v >> 8) << (8 * b);
    }
    P0[d] = lo; P1[d] = hi;
    any |= hi;
  }
  return __ballot(any != 0) ? 2u : 0u;
}

// W reversed: V0[pad + j] / V1[pad + j] = low / high byte of W_{N-1-j} for 0 <= j < N, zero elsewhere in [0, vlen).  Returns 2 when
// some W_i has a nonzero high byte.
template <class Get>
__device__ __forceinline__ u32 stage_rev(u32 *V0, u32 *V1, const Geom &g, int lane, Get get) {
  u32 any = 0;
  for (int d = lane; d < g.vlen / 4; d += 64) {
    u32 lo = 0, hi = 0;
    for (int b = 0; b < 4; b++) {
      const int j = 4 * d + b - g.pad;
      const u32 v = (j >= 0 && j < g.N) ? get(g.N - 1 - j) : 0u;
      lo |= (v & 0xffu) << (8 * b);
      hi |= (v >> 8) << (8 * b);
    }
    V0[d] = lo; V1[d] = hi;
    any |= hi;
  }
  return __ballot(any != 0) ? 2u : 0u;
}

// acc[j][pair] += sum over t in [tlo, thi] of the plane-pair dot products of output kbase + j; d = dword of the j = 3 window at tlo.
// pair 0: A low x W low, 1: A low x W high, 2: A high x W low, 3: A high x W high.
template <bool AH, bool WH>
__device__ __forceinline__ void product4(const u32 *A0, const u32 *A1, const u32 *V0, const u32 *V1, int d, int tlo, int thi,
                                         u32 (&acc)[4][4]) {
  u32 p0 = V0[d], q0 = WH ? V1[d] : 0u;
  for (int t = tlo; t <= thi; t++) {
    d++;
    const u32 p1 = V0[d], q1 = WH ? V1[d] : 0u;
    const u32 a0 = A0[t], a1 = AH ? A1[t] : 0u;
    const u32 w[4] = {__builtin_amdgcn_alignbyte(p1, p0, 3), __builtin_amdgcn_alignbyte(p1, p0, 2),
                      __builtin_amdgcn_alignbyte(p1, p0, 1), p0};
#pragma unroll
    for (int j = 0; j < 4; j++) {
      acc[j][0] = __builtin_amdgcn_udot4(a0, w[j], acc[j][0], false);
      if (AH) acc[j][2] = __builtin_amdgcn_udot4(a1, w[j], acc[j][2], false);
    }
    if (WH) {
      const u32 u[4] = {__builtin_amdgcn_alignbyte(q1, q0, 3), __builtin_amdgcn_alignbyte(q1, q0, 2),
                        __builtin_amdgcn_alignbyte(q1, q0, 1), q0};
#pragma unroll
      for (int j = 0; j < 4; j++) {
        acc[j][1] = __builtin_amdgcn_udot4(a0, u[j], acc[j][1], false);
        if (AH) acc[j][3] = __builtin_amdgcn_udot4(a1, u[j], acc[j][3], false);
      }
    }
    p0 = p1; q0 = q1;
  }
}

// One VerifyInverse-shaped stage on operands already in LDS (planes: bit 1 = A has a high plane, bit 2 = W has one): the product
// (+ m for VerifyEncrypt), its Modulus, the division rule against Q, R (rows of N + 1).  Returns this lane's NTRU_CHECK_* bits.
__device__ __forceinline__ u32 check_stage(const u32 *A0, const u32 *A1, const u32 *V0, const u32 *V1, const Geom &g, int lane,
                                           u32 planes, const Stage &s, const u16 *m, const u16 *Q, const u16 *R) {
  const int N = g.N;
  u32 fl = 0;
  for (int K0 = 0; K0 <= 2 * N; K0 += 256) {
    const int kbase = K0 + 4 * lane;
    const int tlo = K0 - N + 1 > 0 ? (K0 - N + 1) / 4 : 0;
    const int thi = min((N + 3) / 4 - 1, (K0 + 255) / 4);
    u32 acc[4][4] = {};
    if (tlo <= thi) {
      const int d = (g.pad + N - 4 - kbase) / 4 + tlo;
      if (planes & 2u) {
        if (planes & 4u) product4<true, true>(A0, A1, V0, V1, d, tlo, thi, acc);
        else product4<true, false>(A0, A1, V0, V1, d, tlo, thi, acc);
      } else {
        if (planes & 4u) product4<false, true>(A0, A1, V0, V1, d, tlo, thi, acc);
        else product4<false, false>(A0, A1, V0, V1, d, tlo, thi, acc);
      }
    }
#pragma unroll
    for (int j = 0; j < 4; j++) {
      const int k = kbase + j;
      if (k > 2 * N) break;
      u32 a = 0;
      if (k <= 2 * N - 2) {
        u64 x = (u64)acc[j][0] + ((u64)acc[j][1] << 8) + ((u64)acc[j][2] << 8) + ((u64)acc[j][3] << 16);
        if (m && k < N) x += m[k];
        a = modulus(x, s, fl);
      }
      u64 P = 0;
      if (k <= N) P += (u64)Q[k] + R[k];
      if (k >= N) P += (u64)(s.M - 1) * Q[k - N];
      const u32 y = modulus(P, s, fl);
      if (k <= 2 * N - 2) { if (y != a) fl |= NTRU_CHECK_EQ; }
      else if (y != 0) fl |= NTRU_CHECK_TAIL;
    }
  }
  return fl;
}

__device__ __forceinline__ u32 *wave_lds(const Geom &g) {
  extern __shared__ u32 wc_smem[];
  const int wave = threadIdx.x >> 6;
  return wc_smem + (size_t)wave * (2 * g.alen + 2 * g.vlen) / 4;
}

// VerifyEncrypt(q, nq, N): A = h, W = r, + m; quotientE, remainderE
__global__ void __launch_bounds__(WC_THREADS) k_check_encrypt(Geom g, Stage s, const u16 *r, const u16 *m, const u16 *h,
                                                               const u16 *quotE, const u16 *remE, long B, u8 *flags) {
  const int lane = threadIdx.x & 63;
  u32 *A0 = wave_lds(g), *A1 = A0 + g.alen / 4, *V0 = A1 + g.alen / 4, *V1 = V0 + g.vlen / 4;
  const int N = g.N;
  for (long item = (long)blockIdx.x * WC_WAVES + (threadIdx.x >> 6); item < B; item += (long)gridDim.x * WC_WAVES) {
    const size_t rn = (size_t)item * N, rq = (size_t)item * (N + 1);
    u32 planes = stage_fwd(A0, A1, g, lane, [&](int i) { return (u32)h[rn + i]; });
    planes |= stage_rev(V0, V1, g, lane, [&](int i) { return (u32)r[rn + i]; }) << 1;
    wave_lds_fence();
    const u32 fl = check_stage(A0, A1, V0, V1, g, lane, planes, s, m + rn, quotE + rq, remE + rq);
    const u32 all = wave_or(fl);
    if (lane == 0) flags[item] = (u8)all;
    wave_lds_fence();                  // this item's LDS reads before the next item's staging
  }
}

// VerifyInverse(M, n, N): A = fq, W = f; quotientI, remainderI
__global__ void __launch_bounds__(WC_THREADS) k_check_inverse(Geom g, Stage s, const u16 *f, const u16 *fq, const u16 *quot,
                                                               const u16 *rem, long B, u8 *flags) {
  const int lane = threadIdx.x & 63;
  u32 *A0 = wave_lds(g), *A1 = A0 + g.alen / 4, *V0 = A1 + g.alen / 4, *V1 = V0 + g.vlen / 4;
  const int N = g.N;
  for (long item = (long)blockIdx.x * WC_WAVES + (threadIdx.x >> 6); item < B; item += (long)gridDim.x * WC_WAVES) {
    const size_t rn = (size_t)item * N, rq = (size_t)item * (N + 1);
    u32 planes = stage_fwd(A0, A1, g, lane, [&](int i) { return (u32)fq[rn + i]; });
    planes |= stage_rev(V0, V1, g, lane, [&](int i) { return (u32)f[rn + i]; }) << 1;
    wave_lds_fence();
    const u32 fl = check_stage(A0, A1, V0, V1, g, lane, planes, s, nullptr, quot + rq, rem + rq);
    const u32 all = wave_or(fl);
    if (lane == 0) flags[item] = (u8)all;
    wave_lds_fence();
  }
}

// LessThan(nq)(q / 2, x) of VerifyDecrypt: valid iff lo < x <= hi; gt = x > half
struct Gt {
  int lo, hi;
  u32 half;
};

// VerifyDecrypt(q, nq, p, np, N): stage 1 A = e, W = f against quotient1 / remainder1 (mod q); stage 2 A = fp, W = b against
// quotient2 / remainder2 (mod p), b_i = Modulus(p, np)(remainder1[i] + gt_i).  Stage 2's bits are shifted left by 3.
__global__ void __launch_bounds__(WC_THREADS) k_check_decrypt(Geom g, Stage s1, Stage s2, Gt gt, const u16 *f, const u16 *fp,
                                                               const u16 *e, const u16 *quot1, const u16 *rem1, const u16 *quot2,
                                                               const u16 *rem2, long B, u8 *flags) {
  const int lane = threadIdx.x & 63;
  u32 *A0 = wave_lds(g), *A1 = A0 + g.alen / 4, *V0 = A1 + g.alen / 4, *V1 = V0 + g.vlen / 4;
  const int N = g.N;
  for (long item = (long)blockIdx.x * WC_WAVES + (threadIdx.x >> 6); item < B; item += (long)gridDim.x * WC_WAVES) {
    const size_t rn = (size_t)item * N, rq = (size_t)item * (N + 1);
    u32 planes = stage_fwd(A0, A1, g, lane, [&](int i) { return (u32)e[rn + i]; });
    planes |= stage_rev(V0, V1, g, lane, [&](int i) { return (u32)f[rn + i]; }) << 1;
    wave_lds_fence();
    u32 fl = check_stage(A0, A1, V0, V1, g, lane, planes, s1, nullptr, quot1 + rq, rem1 + rq);
    wave_lds_fence();
    u32 fl2 = 0;
    const u16 *R1 = rem1 + rq;
    planes = stage_fwd(A0, A1, g, lane, [&](int i) { return (u32)fp[rn + i]; });
    planes |= stage_rev(V0, V1, g, lane, [&](int i) {
      const int x = R1[i];
      if (x <= gt.lo || x > gt.hi) fl2 |= NTRU_CHECK_RANGE;
      return modulus((u64)x + ((u32)x > gt.half ? 1u : 0u), s2, fl2);
    }) << 1;
    wave_lds_fence();
    fl2 |= check_stage(A0, A1, V0, V1, g, lane, planes, s2, nullptr, quot2 + rq, rem2 + rq);
    const u32 all = wave_or(fl | (fl2 << 3));
    if (lane == 0) flags[item] = (u8)all;
    wave_lds_fence();
  }
}

// ---- host side --------------------------------------------------------------------------------------------------------------------

int check_N(int N) {
  if (N < 2 || N > NTRU_MAX_N) return fail(NTRU_ERR_ARG, "witness check: need 2 <= N <= " + std::to_string(NTRU_MAX_N) + ", got N = " + std::to_string(N));
  return NTRU_OK;
}

int check_mod(const char *name, int M, int n) {
  if (M < 2 || M > 65536)
    return fail(NTRU_ERR_ARG, std::string("witness check: need 2 <= ") + name + " <= 65536, got " + std::to_string(M));
  if (n < 1 || n > 252)
    return fail(NTRU_ERR_ARG, std::string("witness check: the bit count of ") + name + " must be in [1, 252] (circomlib's LessThan), got " +
                                  std::to_string(n));
  return NTRU_OK;
}

int check_batch(ntru_engine *eng, int64_t B) {
  if (B < 0) return fail(NTRU_ERR_ARG, "witness check: negative batch size");
  if (!eng) return fail(NTRU_ERR_ARG, "engine is NULL");
  return NTRU_OK;
}

// Modulus(M, n) of a stage: T and the y bounds (no signal reaches 2^44, so larger n never bind)
Stage stage_of(int M, int n) {
  Stage s;
  s.M = (u32)M;
  s.mask = is_pow2(M) ? (u32)M - 1 : 0u;
  if (n >= 45) s.T = ~0ull;
  else {
    const u64 p = 1ull << n;
    s.T = p + (p - 1) / (u64)(M - 1);
  }
  s.ylo = (n < 17 && (u64)M > (1ull << n)) ? (u32)(M - (1 << n)) : 0u;
  s.yhi = n < 16 ? (u32)((1 << n) - 1) : 65535u;
  return s;
}

template <class Kern, class... Args>
int launch_check(ntru_engine *eng, Kern kern, const char *name, const Geom &g, int64_t B, Args... args) {
  HIP_TRY(hipSetDevice(eng->device));
  const size_t lds = (size_t)WC_WAVES * (2 * g.alen + 2 * g.vlen);
  if (int rc = launch_resident(eng, kern, (long)((B + WC_WAVES - 1) / WC_WAVES), WC_THREADS, lds, g, args...)) return rc;
  note_kernel(eng, name);
  return NTRU_OK;
}

}  // namespace

extern "C" int ntru_check_encrypt_batch_dev(ntru_engine_t *eng, int N, int q, int nq, const uint16_t *d_r, const uint16_t *d_m,
                                            const uint16_t *d_h, const uint16_t *d_quotE, const uint16_t *d_remE, int64_t B,
                                            uint8_t *d_flags) {
  if (int rc = check_N(N)) return rc;
  if (int rc = check_mod("q", q, nq)) return rc;
  if (int rc = check_batch(eng, B)) return rc;
  if (B == 0) return NTRU_OK;
  if (!d_r || !d_m || !d_h || !d_quotE || !d_remE || !d_flags) return fail(NTRU_ERR_ARG, "ntru_check_encrypt_batch: NULL buffer");
  return launch_check(eng, k_check_encrypt, "k_check_encrypt", geom_of(N), B, stage_of(q, nq), d_r, d_m, d_h, d_quotE, d_remE, (long)B,
                      d_flags);
}

extern "C" int ntru_check_inverse_batch_dev(ntru_engine_t *eng, int N, int M, int n, const uint16_t *d_f, const uint16_t *d_fq,
                                            const uint16_t *d_quotI, const uint16_t *d_remI, int64_t B, uint8_t *d_flags) {
  if (int rc = check_N(N)) return rc;
  if (int rc = check_mod("M", M, n)) return rc;
  if (int rc = check_batch(eng, B)) return rc;
  if (B == 0) return NTRU_OK;
  if (!d_f || !d_fq || !d_quotI || !d_remI || !d_flags) return fail(NTRU_ERR_ARG, "ntru_check_inverse_batch: NULL buffer");
  return launch_check(eng, k_check_inverse, "k_check_inverse", geom_of(N), B, stage_of(M, n), d_f, d_fq, d_quotI, d_remI, (long)B,
                      d_flags);
}

extern "C" int ntru_check_decrypt_batch_dev(ntru_engine_t *eng, int N, int q, int nq, int p, int np, const uint16_t *d_f,
                                            const uint16_t *d_fp, const uint16_t *d_e, const uint16_t *d_quot1, const uint16_t *d_rem1,
                                            const uint16_t *d_quot2, const uint16_t *d_rem2, int64_t B, uint8_t *d_flags) {
  if (int rc = check_N(N)) return rc;
  if (int rc = check_mod("q", q, nq)) return rc;
  if (q & 1) return fail(NTRU_ERR_ARG, "witness check: VerifyDecrypt needs an even q (q/2 is a field division), got " + std::to_string(q));
  if (int rc = check_mod("p", p, np)) return rc;
  if (int rc = check_batch(eng, B)) return rc;
  if (B == 0) return NTRU_OK;
  if (!d_f || !d_fp || !d_e || !d_quot1 || !d_rem1 || !d_quot2 || !d_rem2 || !d_flags)
    return fail(NTRU_ERR_ARG, "ntru_check_decrypt_batch: NULL buffer");
  Gt gt;
  gt.half = (u32)(q / 2);
  const long span = nq >= 20 ? (1l << 20) : (1l << nq);        // remainder1 < 65536: a wider span never binds
  gt.lo = (int)std::max<long>(-1, (long)(q / 2) - span);
  gt.hi = (int)std::min<long>(1l << 20, (long)(q / 2) + span);
  return launch_check(eng, k_check_decrypt, "k_check_decrypt", geom_of(N), B, stage_of(q, nq), stage_of(p, np), gt, d_f, d_fp, d_e,
                      d_quot1, d_rem1, d_quot2, d_rem2, (long)B, d_flags);
}
