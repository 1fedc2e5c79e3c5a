// matrix_peritem_scheme.hip -- encryptBits / decryptBits (index.js:87-140) with a SEPARATE key pair for every item: the kernels, the
// composed fallback outside their range, and the *_dev entry points (host-pointer forms: ntru_host.hip).
//
// The reference's unit is one NTRU instance per key, so "one ciphertext per recipient" and "one decryption per key holder" are the
// batches its users have.  Both kernels follow k_verify_keys_m (matrix_peritem.hip): one item per wavefront, the chunk rows of the
// batch operand in registers (lane (r, hh) holds chunk 2 r + hh), the reversed Toeplitz array of the key-side operand in the wave's
// LDS, and pi_product_reg, which keeps low and high half apart -- remainder = low + high, quotient = -high.
//   k_encrypt_pi_m   rows = the digit planes of h (two; one centred plane for q <= 256), Toeplitz array of r (bytes 0/1/2 as int8):
//                    k_verify_keys_m's product 1 alone, with e = (low + high + m) mod q and quotE = -high mod q (m has degree < N:
//                    it never reaches the quotient).
//   k_decrypt_pi_m   both reversed arrays (f ternary, fp) at item start; product 1 = the digit planes of e against f gives quot1 /
//                    rem1; its epilogue lifts rem1 to a in {0, 1, 2} (index.js:117; the engine's lift addend for its 1) and writes a as a natural-order byte
//                    image into the wave's LDS, from which each lane reads its own 16-byte chunk back -- the row layout, the route
//                    of the Newton round's e; product 2 = one plane, a against fp, reduced mod 3: value = rem2 and quot2.
// Range: 128 <= N <= 1024 (64 with kernel path 4), q <= 8192, p == 3 for decrypt (peritem_applies).  Outside it the entry points
// compose existing launches (ntru_polymul_split_dev with per-item operands, plus the small elementwise kernels below): correct, not fast.
#include <algorithm>

#include "peritem_common.h"

// ---- encryptBits, one key per item ------------------------------------------------------------------------------------------
// ONE: q <= 256, a single (centred) digit plane of h.  quotE may be NULL (its stores go to an empty descriptor and are dropped).
template <bool ONE>
__global__ __launch_bounds__(64 * PI_WAVES) __attribute__((amdgpu_waves_per_eu(ONE ? 4 : 3, 4))) void k_encrypt_pi_m(
    PGeom g, u32 q, const u16 *__restrict__ h, const uint8_t *__restrict__ r, const uint8_t *__restrict__ m, long B,
    u16 *__restrict__ e, u16 *__restrict__ quotE) {
  extern __shared__ __attribute__((aligned(16))) unsigned char lds[];
  constexpr int NPL = ONE ? 1 : 2;
  const int lane = threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  unsigned char *nat = lds + (size_t)wave * pi_wave_bytes(g, 1);
  u32 *T = (u32 *)(nat + pi_nat_bytes(g));
  const int N = g.N;
  const bool want_q = quotE != nullptr;
  const long item_step = (long)gridDim.x * PI_WAVES;         // the NEXT item's rows are requested early: see k_product_tern_m
  PiRow<2> rh;
  PiRow<1> rr;
  auto request = [&](long it) {
    const int ch = pi_chunk_of(opaque(lane));
    rh.request(h, it, N, ch); rr.request(r, it, N, ch);
  };
  if ((long)blockIdx.x * PI_WAVES + wave < B) request((long)blockIdx.x * PI_WAVES + wave);
  for (long item = (long)blockIdx.x * PI_WAVES + wave; item < B; item += item_step) {
    const long row = item * N;
    v4i F[NPL];
    {
      const int ch = pi_chunk_of(opaque(lane));
      u32 xh[8];
      rh.pairs(h + row, xh);
      const v4i vr = rr.bytes(r + row);
      if (item + item_step < B) request(item + item_step);
      pi_build_array_ch(nat, T, g, lane, ch, vr & col_mask16(16 * ch, N));
      v4i o0, o1;
      pi_digits(xh, q, 1u, 16 * ch, N, o0, o1);
      F[0] = o0;
      if (!ONE) F[NPL - 1] = o1;
    }
    // m in the accumulator layout (register i of this lane: index pi_ko(i) + kl), in flight during the product;
    // bytes at and beyond N read as zero
    const int kl = pi_index_of(opaque(lane));
    const __amdgpu_buffer_rsrc_t rs_m = rows_rsrc(m + row, (long)N);
    u32 mv[16];
#pragma unroll
    for (int i = 0; i < 16; i++) mv[i] = __builtin_amdgcn_raw_buffer_load_b8(rs_m, kl, pi_ko(i), 0);
    v16i L[NPL], H[NPL];
    pi_product_reg<NPL>(F, T, g, lane, L, H);
    {
      const __amdgpu_buffer_rsrc_t rs_e = rows_rsrc(e + row, 2L * N);
      const __amdgpu_buffer_rsrc_t rs_q = rows_rsrc(want_q ? quotE + row : nullptr, want_q ? 2L * N : 0L);
      pi_for_split<NPL>(L, H, [&](int i, int ko, u32 lo, u32 hi) {
        __builtin_amdgcn_raw_buffer_store_b16((u16)((lo + hi + mv[i]) & (q - 1)), rs_e, 2 * kl, 2 * ko, 0);
        if (want_q) __builtin_amdgcn_raw_buffer_store_b16((u16)((0u - hi) & (q - 1)), rs_q, 2 * kl, 2 * ko, 0);
      });
    }
    wave_lds_fence();
  }
}

// ---- decryptBits, one key per item ------------------------------------------------------------------------------------------
// p == 3.  ONE: q <= 256, a single (centred) digit plane of e.  quot1 / rem1 / quot2 may be NULL (empty descriptors).
template <bool ONE>
__global__ __launch_bounds__(64 * PI_WAVES) __attribute__((amdgpu_waves_per_eu(3, 4))) void k_decrypt_pi_m(
    PGeom g, u32 q, u32 lift_add, const int8_t *__restrict__ f, const uint8_t *__restrict__ fp, const u16 *__restrict__ e, long B,
    uint8_t *__restrict__ value, u16 *__restrict__ quot1, u16 *__restrict__ rem1, uint8_t *__restrict__ quot2) {
  extern __shared__ __attribute__((aligned(16))) unsigned char lds[];
  constexpr int NPL = ONE ? 1 : 2;
  const int lane = threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  unsigned char *nat = lds + (size_t)wave * pi_wave_bytes(g, 2);
  u32 *Tf = (u32 *)(nat + pi_nat_bytes(g)), *Tp = Tf + 4 * g.tpitch;
  const int N = g.N;
  const bool want_q1 = quot1 != nullptr, want_r1 = rem1 != nullptr, want_q2 = quot2 != nullptr;
  const long item_step = (long)gridDim.x * PI_WAVES;
  PiRow<2> re;
  PiRow<1> rf, rp;
  auto request = [&](long it) {
    const int ch = pi_chunk_of(opaque(lane));
    re.request(e, it, N, ch); rf.request(f, it, N, ch); rp.request(fp, it, N, ch);
  };
  if ((long)blockIdx.x * PI_WAVES + wave < B) request((long)blockIdx.x * PI_WAVES + wave);
  for (long item = (long)blockIdx.x * PI_WAVES + wave; item < B; item += item_step) {
    const long row = item * N;
    v4i F[NPL];
    {
      const int ch = pi_chunk_of(opaque(lane));
      const v4i cmask = col_mask16(16 * ch, N);
      u32 xe[8];
      re.pairs(e + row, xe);
      const v4i vf = rf.bytes(f + row), vp = rp.bytes(fp + row);
      if (item + item_step < B) request(item + item_step);
      pi_build_array_ch(nat, Tf, g, lane, ch, pi_ternary(vf, cmask));
      pi_build_array_ch(nat, Tp, g, lane, ch, pi_mod3_bytes(vp & cmask));   // (its last fence: nat is free for the image of a)
      v4i o0, o1;
      pi_digits(xe, q, 1u, 16 * ch, N, o0, o1);
      F[0] = o0;
      if (!ONE) F[NPL - 1] = o1;
    }
    // ---- product 1: f (x) e modulo q, then the lift into a natural-order byte image (index <= 1151 whatever N is: pi_nat_bytes)
    const int kl = pi_index_of(opaque(lane));
    v4i A[1];
    {
      v16i L[NPL], H[NPL];
      pi_product_reg<NPL>(F, Tf, g, lane, L, H);
      const __amdgpu_buffer_rsrc_t rs_q = rows_rsrc(want_q1 ? quot1 + row : nullptr, want_q1 ? 2L * N : 0L);
      const __amdgpu_buffer_rsrc_t rs_r = rows_rsrc(want_r1 ? rem1 + row : nullptr, want_r1 ? 2L * N : 0L);
      pi_for_split<NPL>(L, H, [&](int, int ko, u32 lo, u32 hi) {
        const u32 rv = (lo + hi) & (q - 1);
        if (want_r1) __builtin_amdgcn_raw_buffer_store_b16((u16)rv, rs_r, 2 * kl, 2 * ko, 0);
        if (want_q1) __builtin_amdgcn_raw_buffer_store_b16((u16)((0u - hi) & (q - 1)), rs_q, 2 * kl, 2 * ko, 0);
        nat[ko + kl] = (unsigned char)(2 * rv > q ? (rv + lift_add) % 3u : rv % 3u);     // index.js:117 (lift_add for its 1), strict >
      });
      wave_lds_fence();
      const int ch = pi_chunk_of(opaque(lane));
      A[0] = *(const v4i *)(nat + 16 * ch) & col_mask16(16 * ch, N);        // (bytes at and beyond N: junk tiles, cut)
    }
    // ---- product 2: a (x) fp modulo 3
    v16i L2[1], H2[1];
    pi_product_reg<1>(A, Tp, g, lane, L2, H2);
    {
      const __amdgpu_buffer_rsrc_t rs_v = rows_rsrc(value + row, (long)N);
      const __amdgpu_buffer_rsrc_t rs_q = rows_rsrc(want_q2 ? quot2 + row : nullptr, want_q2 ? (long)N : 0L);
#pragma unroll
      for (int i = 0; i < 16; i++) {
        const int ko = pi_ko(i);
        // 0 <= L, H <= 4 N (a, fp < 3): no sign to take care of
        __builtin_amdgcn_raw_buffer_store_b8((uint8_t)((u32)(L2[0][i] + H2[0][i]) % 3u), rs_v, kl, ko, 0);
        if (want_q2) __builtin_amdgcn_raw_buffer_store_b8((uint8_t)((3u - (u32)H2[0][i] % 3u) % 3u), rs_q, kl, ko, 0);
      }
    }
    wave_lds_fence();                                      // the image is read before the next item's arrays are staged over it
  }
}

// ---- the composed path (outside the kernels' range): elementwise steps around ntru_polymul_split_dev ------------------------------
__global__ void k_pi_widen(const uint8_t *__restrict__ in, long n, u16 *__restrict__ out) {
  for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (long)gridDim.x * blockDim.x) out[i] = in[i];
}
__global__ void k_pi_narrow(const u16 *__restrict__ in, long n, uint8_t *__restrict__ out) {
  for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (long)gridDim.x * blockDim.x) out[i] = (uint8_t)in[i];
}
// f in {-1, 0, 1} as a residue mod q (index.js:112: -1 -> q - 1)
__global__ void k_pi_signed_modq(const int8_t *__restrict__ in, long n, u32 q, u16 *__restrict__ out) {
  for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (long)gridDim.x * blockDim.x) out[i] = (u16)((u32)(int)in[i] & (q - 1));
}
// e += m mod q (index.js:90-92: any byte of m)
__global__ void k_pi_add_bytes(u16 *__restrict__ e, const uint8_t *__restrict__ m, long n, u32 q) {
  for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (long)gridDim.x * blockDim.x) e[i] = (u16)(((u32)e[i] + m[i]) & (q - 1));
}
// the centred lift of index.js:117, lift_add in place of its 1
__global__ void k_pi_lift(const u16 *__restrict__ rem, long n, u32 q, u32 p, u32 lift_add, u16 *__restrict__ out) {
  for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (long)gridDim.x * blockDim.x) {
    const u32 x = rem[i];
    out[i] = (u16)lift_value(x, q, p, lift_add);
  }
}

namespace {

// Items per pass of the composed path: its temporaries (`per_item` bytes each) stay within 256 MB of engine-owned scratch.
int64_t composed_items(int64_t B, size_t per_item) {
  const int64_t c = std::max<int64_t>(1024, (int64_t)(((size_t)256 << 20) / per_item));
  return std::min(B, c);
}

template <class Kern, class... Args>
int launch_elementwise(ntru_engine *eng, Kern kern, long n, Args... args) {
  hipLaunchKernelGGL(kern, elementwise_grid(eng, n), dim3(256), 0, eng->stream, args...);
  HIP_TRY(hipGetLastError());
  return NTRU_OK;
}

// last_kernel of a composed call: the product's kernel inside it
void note_composed(ntru_engine *eng) {
  char inner[sizeof eng->last_kernel];
  snprintf(inner, sizeof inner, "%s", eng->last_kernel);
  snprintf(eng->last_kernel, sizeof eng->last_kernel, "peritem_composed(%.40s)", inner);
}

int encrypt_composed(ntru_engine *eng, int N, int q, const uint16_t *d_h, const uint8_t *d_r, const uint8_t *d_m, int64_t B,
                     uint16_t *d_e, uint16_t *d_quotE) {
  const size_t row = 2 * (size_t)N, per_item = (d_quotE ? 1 : 2) * row;
  const int64_t C = composed_items(B, per_item);
  ScratchHold hold(eng, (size_t)C * per_item + 256);
  if (hold.rc) return hold.rc;
  uint16_t *const r16 = (uint16_t *)hold.p, *const qt = r16 + (size_t)C * N;
  for (int64_t o = 0; o < B; o += C) {
    const int64_t n = std::min(C, B - o);
    const long el = (long)(n * N), off = (long)(o * N);
    if (int rc = launch_elementwise(eng, k_pi_widen, el, d_r + off, el, r16)) return rc;
    if (int rc = ntru_polymul_split_dev(eng, N, q, d_h + off, r16, n, d_quotE ? d_quotE + off : qt, d_e + off)) return rc;
    if (int rc = launch_elementwise(eng, k_pi_add_bytes, el, d_e + off, d_m + off, el, (u32)q)) return rc;
  }
  note_composed(eng);
  return NTRU_OK;
}

int decrypt_composed(ntru_engine *eng, int N, int q, int p, const int8_t *d_f, const uint8_t *d_fp, const uint16_t *d_e, int64_t B,
                     uint8_t *d_value, uint16_t *d_quot1, uint16_t *d_rem1, uint8_t *d_quot2) {
  // six rows of u16 per item: f mod q (then the lifted a), fp, quot1 and rem1 when not wanted, quot2 and rem2 before the narrowing
  const size_t row = 2 * (size_t)N, per_item = 6 * row;
  const int64_t C = composed_items(B, per_item);
  ScratchHold hold(eng, (size_t)C * per_item + 256);
  if (hold.rc) return hold.rc;
  uint16_t *const s = (uint16_t *)hold.p;
  const size_t cn = (size_t)C * N;
  uint16_t *const fa = s, *const fp16 = s + cn, *const q1t = s + 2 * cn, *const r1t = s + 3 * cn, *const q2 = s + 4 * cn, *const r2 = s + 5 * cn;
  for (int64_t o = 0; o < B; o += C) {
    const int64_t n = std::min(C, B - o);
    const long el = (long)(n * N), off = (long)(o * N);
    uint16_t *const q1 = d_quot1 ? d_quot1 + off : q1t, *const r1 = d_rem1 ? d_rem1 + off : r1t;
    if (int rc = launch_elementwise(eng, k_pi_signed_modq, el, d_f + off, el, (u32)q, fa)) return rc;
    if (int rc = ntru_polymul_split_dev(eng, N, q, fa, d_e + off, n, q1, r1)) return rc;
    if (int rc = launch_elementwise(eng, k_pi_lift, el, (const u16 *)r1, el, (u32)q, (u32)p, ntru_lift_addend(eng, q, p), fa)) return rc;
    if (int rc = launch_elementwise(eng, k_pi_widen, el, d_fp + off, el, fp16)) return rc;
    if (int rc = ntru_polymul_split_dev(eng, N, p, fp16, fa, n, q2, r2)) return rc;
    if (int rc = launch_elementwise(eng, k_pi_narrow, el, (const u16 *)r2, el, d_value + off)) return rc;
    if (d_quot2)
      if (int rc = launch_elementwise(eng, k_pi_narrow, el, (const u16 *)q2, el, d_quot2 + off)) return rc;
  }
  note_composed(eng);
  return NTRU_OK;
}

}  // namespace

// ---- device-pointer entry points ----------------------------------------------------------------------------------------------------
extern "C" int ntru_encrypt_peritem_batch_dev(ntru_engine_t *eng, int N, int q, const uint16_t *d_h, const uint8_t *d_r,
                                              const uint8_t *d_m, int64_t B, uint16_t *d_e, uint16_t *d_quotE) {
  if (int rc = ntru_check_common(eng, N, q, B)) return rc;
  if (B == 0) return NTRU_OK;
  if (!d_h || !d_r || !d_m || !d_e) return fail(NTRU_ERR_ARG, "ntru_encrypt_peritem_batch: NULL buffer");
  HIP_TRY(hipSetDevice(eng->device));
  if (!peritem_applies(eng, N, q)) return encrypt_composed(eng, N, q, d_h, d_r, d_m, B, d_e, d_quotE);
  const PGeom pg = make_pgeom(N);
  note_kernel(eng, "k_encrypt_pi_m");
  return launch_peritem(eng, q <= 256 ? k_encrypt_pi_m<true> : k_encrypt_pi_m<false>, B, pi_wave_bytes(pg, 1), pg, (u32)q, d_h, d_r, d_m,
                        (long)B, d_e, d_quotE);
}

extern "C" int ntru_decrypt_peritem_batch_dev(ntru_engine_t *eng, int N, int q, int p, const int8_t *d_f, const uint8_t *d_fp,
                                              const uint16_t *d_e, int64_t B, uint8_t *d_value, uint16_t *d_quot1, uint16_t *d_rem1,
                                              uint8_t *d_quot2) {
  if (int rc = ntru_check_common(eng, N, q, B)) return rc;
  if (int rc = ntru_check_decrypt_p(N, p)) return rc;
  if (B == 0) return NTRU_OK;
  if (!d_f || !d_fp || !d_e || !d_value) return fail(NTRU_ERR_ARG, "ntru_decrypt_peritem_batch: NULL buffer");
  HIP_TRY(hipSetDevice(eng->device));
  if (p != 3 || !peritem_applies(eng, N, q)) return decrypt_composed(eng, N, q, p, d_f, d_fp, d_e, B, d_value, d_quot1, d_rem1, d_quot2);
  const PGeom pg = make_pgeom(N);
  note_kernel(eng, "k_decrypt_pi_m");
  return launch_peritem(eng, q <= 256 ? k_decrypt_pi_m<true> : k_decrypt_pi_m<false>, B, pi_wave_bytes(pg, 2), pg, (u32)q, ntru_lift_addend(eng, q, 3), d_f, d_fp, d_e,
                        (long)B, d_value, d_quot1, d_rem1, d_quot2);
}
