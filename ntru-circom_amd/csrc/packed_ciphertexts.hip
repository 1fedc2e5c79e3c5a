// packed_ciphertexts.hip -- ciphertexts in the circuits' wire format, packOutput(mod - 1, N, e) (index.js:572-596; what CombineArray
// makes public and ntru_encrypt_pack_batch_dev, ntru_pipeline_batch and ntru_keygen_batch emit), read back on the device: sums in groups
// straight from the packed rows, unpacking to dense rows, and the tally and decrypt calls on top of them.
//
// Format (ntru_pack_params(mod - 1, N, &bits, &per, &arr_len, &os)): a row is `os` field elements of four little-endian uint64_t limbs,
// coefficient i is the bits-wide field at bit (i % per) * bits of element i / per; fields may straddle limbs.  Fields with index >= N
// and the bits of an element above per * bits are ignored, as k_unpack and unpackInput's mask ignore them.
//
// k_sum_groups_packed<BITS, POW2, WEIGHTED>:  out[g][k] = (sum over the rows of group g of w[row] * field_k(row)) mod `mod`, the contract
// of k_sum_groups (ciphertext_sum.hip) on 32 os bytes per row instead of 2 N.  The rows are cut into Pb row blocks exactly as there
// (sum_groups_common.h), a group inside one block is stored from the registers, a group that crosses a boundary leaves the partial rows
// that the existing k_sum_groups_finish completes.  Inside a block:
//   * one lane owns one UNIT of a row and keeps one accumulator per field of it.  For bits >= 7 (per <= 36: every q >= 128) a unit is a
//     whole element: the lane reads its 32 bytes as two 16-byte loads and takes the per fields out of them with constant shifts.  For
//     smaller moduli an element has up to 252 fields; it is cut into slices of 32 fields, which are exactly `bits` whole dwords, and
//     a unit is one slice (the same kernel body on `bits` dword loads: no second, unpacking path, which a _dev call with device offsets
//     could not size without reading them);
//   * a row has U = os x slices units.  U <= 32: floor(64 / U) rows sit side by side in the wave, and when a group ends the lanes that
//     hold the same unit are added up across the wave (ds_bpermute tree over reduced values).  32 < U <= 64: one row per step.  U > 64:
//     tiles of 64 units, one wavefront each;
//   * four row steps are loaded before the first is summed.
// Every load lies inside the lane's own element of an existing row: nothing is read past the array.  A 16-byte load needs a 4-byte
// aligned address only (matrix_common.h), so a base that is 8 but not 16 bytes aligned takes the same instructions.
// Exactness: a raw field is < 2^bits <= 65536 and w < mod <= 65536, so w x < 2^32 from one 24-bit multiply; for a power-of-two modulus
// the u32 accumulators may wrap, otherwise they are u64 and partial rows are stored reduced.  Integer sums do not depend on the order:
// the result is the same bytes whatever the decomposition.
//
// k_unpack_rows: packed rows -> dense [B][N] uint16_t rows (the pad is dropped), one coefficient per thread.
#include <hip/hip_runtime.h>

#include <cstdint>
#include <cstdio>
#include <cstring>
#include <string>

#include "kernels_common.h"
#include "sum_groups_common.h"

namespace {

constexpr int SP_THREADS = 256;          // four independent waves
constexpr int SP_WAVES_PER_CU = 8;
constexpr int SP_BATCH = 4;              // row steps in flight
constexpr int PK_PASS = 65536;           // rows per pass of the calls that unpack into scratch

typedef u32x4 u32x4_a8 __attribute__((aligned(8)));

// How a lane sees an element of BITS-wide fields.
template <int BITS>
struct Unit {
  static constexpr int PER = 252 / BITS;
  static constexpr bool SLICED = PER > 36;
  static constexpr int SLICES = SLICED ? (PER + 31) / 32 : 1;   // a slice: 32 fields = BITS whole dwords
  static constexpr int NF = SLICED ? 32 : PER;                  // fields = accumulators of a unit
  static constexpr int NDW = SLICED ? BITS : 8;                 // dwords a unit reads
};
int slices_of(int bits) { return 252 / bits > 36 ? (252 / bits + 31) / 32 : 1; }

// The dwords of unit (element at p, slice c).  A sliced unit's last slice may reach past the element's eight dwords: those read as 0.
template <int BITS>
__device__ __forceinline__ void load_unit(const u32 *p, int c, u32 (&d)[Unit<BITS>::NDW]) {
  if constexpr (!Unit<BITS>::SLICED) {
    const u32x4 lo = *(const u32x4_a8 *)p, hi = *(const u32x4_a8 *)(p + 4);
#pragma unroll
    for (int k = 0; k < 4; k++) { d[k] = lo[k]; d[k + 4] = hi[k]; }
  } else {
#pragma unroll
    for (int k = 0; k < Unit<BITS>::NDW; k++) d[k] = c * BITS + k < 8 ? p[c * BITS + k] : 0u;
  }
}

// acc[j] += w * field j of the unit, for every field (j is a constant after unrolling: every shift and register is fixed)
template <int BITS, bool WEIGHTED, class Acc>
__device__ __forceinline__ void accumulate(Acc (&acc)[Unit<BITS>::NF], const u32 (&d)[Unit<BITS>::NDW], u32 w) {
  constexpr int NDW = Unit<BITS>::NDW;
#pragma unroll
  for (int j = 0; j < Unit<BITS>::NF; j++) {
    const int pos = j * BITS, k = pos >> 5, sh = pos & 31;
    u32 x = d[k] >> sh;
    if (sh + BITS > 32) x |= d[k + 1 < NDW ? k + 1 : k] << (32 - sh);
    x &= (1u << BITS) - 1u;
    acc[j] += (Acc)(WEIGHTED ? __umul24(x, w) : x);
  }
}

// R row steps from row r on (the rows r, r + side, ...): every load is issued before the first sum needs one.
template <int R, int BITS, bool WEIGHTED, class Acc>
__device__ __forceinline__ void row_batch(Acc (&acc)[Unit<BITS>::NF], const u32 *p, long pitch, int c, const u16 *w, int side) {
  u32 d[R][Unit<BITS>::NDW];
  u32 wt[R];
#pragma unroll
  for (int j = 0; j < R; j++) {
    load_unit<BITS>(p + j * pitch, c, d[j]);
    wt[j] = WEIGHTED ? (u32)w[j * side] : 1u;
  }
#pragma unroll
  for (int j = 0; j < R; j++) accumulate<BITS, WEIGHTED>(acc, d[j], wt[j]);
}

template <int BITS, bool POW2, bool WEIGHTED>
__global__ void __launch_bounds__(SP_THREADS) k_sum_groups_packed(int N, u32 mod, Groups gr, const u32 *__restrict__ packed,
                                                                  const u16 *__restrict__ wts, int os, int NT, long Pb,
                                                                  u32 *__restrict__ part, long *__restrict__ meta, u16 *__restrict__ out) {
  typedef typename std::conditional<POW2, u32, u64>::type Acc;
  typedef Unit<BITS> UN;
  const int lane = threadIdx.x & 63;
  const long wave = (long)blockIdx.x * (SP_THREADS / 64) + (threadIdx.x >> 6);
  const int tile = (int)(wave % NT);
  const long b = wave / NT;
  if (b >= Pb) return;
  const Cut cut = cut_of(gr, Pb);
  if (b >= cut.nb) return;
  const long r0 = cut.base + b * cut.R;
  const long r1 = r0 + cut.R < cut.end ? r0 + cut.R : cut.end;
  const bool last = r1 == cut.end;
  // this lane's unit: row `sub` of the `side` rows of a step, element `elem`, slice c
  const int U = os * UN::SLICES;
  const int side = U <= 32 ? 64 / U : 1;
  const int sub = U <= 32 ? lane / U : 0;
  const int u = U <= 32 ? lane - sub * U : tile * 64 + lane;
  const bool active = sub < side && u < U;
  const int elem = u / UN::SLICES, c = u - elem * UN::SLICES;
  const int col0 = elem * UN::PER + c * 32;                             // the unit's first coefficient
  int nv = UN::PER - c * 32 < UN::NF ? UN::PER - c * 32 : UN::NF;       // its fields that are coefficients: inside the element and the row
  nv = N - col0 < nv ? N - col0 : nv;
  const long pitch = (long)os * 8 * side;                               // dwords from one row step to the next
  // first group that meets the block: the first one that starts at or behind r0, or the one before it when that reaches into the block
  long g = 0;
  {
    long lo = 0, hi = gr.G;
    while (lo < hi) {
      const long mid = (lo + hi) >> 1;
      if (g_start(gr, mid) < r0) lo = mid + 1; else hi = mid;
    }
    g = lo;
    if (g > 0 && g_start(gr, g) > r0) g--;
  }
  long tail_g = -1;
  for (; g < gr.G; g++) {
    const long s = g_start(gr, g);
    if (s >= r1 && !last) break;
    const long e = g_start(gr, g + 1);
    const long a = s > r0 ? s : r0, z = e < r1 ? e : r1;
    Acc acc[UN::NF];
#pragma unroll
    for (int k = 0; k < UN::NF; k++) acc[k] = 0;
    if (active && nv > 0) {
      long r = a + sub;
      const u32 *p = packed + ((r - gr.wlo) * os + elem) * 8;
      const u16 *w = WEIGHTED ? wts + (r - gr.wlo) : nullptr;
      const long step = (long)SP_BATCH * side;
      for (; r + step - side < z; r += step, p += SP_BATCH * pitch, w += WEIGHTED ? step : 0)
        row_batch<SP_BATCH, BITS, WEIGHTED>(acc, p, pitch, c, w, side);
      for (; r < z; r += side, p += pitch, w += WEIGHTED ? side : 0) row_batch<1, BITS, WEIGHTED>(acc, p, pitch, c, w, side);
    }
    u32 v[UN::NF];
#pragma unroll
    for (int k = 0; k < UN::NF; k++) v[k] = POW2 ? (u32)acc[k] & (mod - 1) : mod_u64((u64)acc[k], mod);
    if (side > 1) {                                                     // (the same for the whole wave) rows side by side: add them up
      for (int dist = 1; dist < side; dist <<= 1) {
        const bool take = sub + dist < side;
#pragma unroll
        for (int k = 0; k < UN::NF; k++) {
          const u32 t = (u32)__shfl((int)v[k], lane + dist * U, 64);
          if (take) v[k] += t;
        }
      }
#pragma unroll
      for (int k = 0; k < UN::NF; k++) v[k] = POW2 ? v[k] & (mod - 1) : v[k] % mod;   // at most 21 values below mod
    }
    if (s >= r0 && e <= r1) {
      if (active && sub == 0) {
        u16 *q = out + g * N + col0;
#pragma unroll
        for (int k = 0; k < UN::NF; k++)
          if (k < nv) q[k] = (u16)v[k];
      }
    } else {
      const int slot = s < r0 ? 0 : 1;
      if (slot) tail_g = g;
      if (active && sub == 0) {
        u32 *q = part + (b * 2 + slot) * N + col0;
#pragma unroll
        for (int k = 0; k < UN::NF; k++)
          if (k < nv) q[k] = v[k];
      }
    }
  }
  if (tile == 0 && lane == 0) meta[b] = tail_g;
}

// unpackInput (index.js:598-620) of every row without its pad: out[b][i] = field (i % per) of element i / per of row b.
__global__ void __launch_bounds__(256) k_unpack_rows(int N, int bits, int per, int os, const u64 *__restrict__ in, long B,
                                                     u16 *__restrict__ out) {
  const long total = B * N;
  for (long idx = (long)blockIdx.x * blockDim.x + threadIdx.x; idx < total; idx += (long)gridDim.x * blockDim.x) {
    const long b = idx / N;
    const int i = (int)(idx - b * N), e = i / per, pos = (i - e * per) * bits, k = pos >> 6, sh = pos & 63;
    const u64 *l = in + (b * os + e) * 4;
    u64 v = l[k] >> sh;
    if (sh + bits > 64) v |= l[k + 1] << (64 - sh);                     // pos + bits <= 252: limb k + 1 exists
    out[idx] = (u16)(v & ((1u << bits) - 1u));
  }
}

struct PackShape { int bits, per, os; };
int pack_shape(int mod, int N, PackShape *ps) {
  int al;
  return ntru_pack_params(mod - 1, N, &ps->bits, &ps->per, &al, &ps->os);
}

// Enqueues the sums of the groups `w` of the packed rows at d_packed (row w.wlo first) into d_out (group 0 of w first).
int launch_sum_packed(ntru_engine *eng, int N, int mod, const void *d_packed, const uint16_t *d_weights, const SumWindow &w, uint16_t *d_out) {
  PackShape ps;
  if (int rc = pack_shape(mod, N, &ps)) return rc;
  if (ps.bits < 1 || ps.bits > 16) return fail(NTRU_ERR_ARG, "ntru_sum_groups_packed: no kernel for fields of " + std::to_string(ps.bits) + " bits");
  const int U = ps.os * slices_of(ps.bits);
  const bool pow2 = is_pow2(mod), weighted = d_weights != nullptr;
  auto enqueue = [&](dim3 grid, const Groups &gr, int NT, long Pb, u32 *part, long *meta) {
    auto go = [&](auto bits, auto p2, auto wt) {
      hipLaunchKernelGGL((k_sum_groups_packed<decltype(bits)::value, decltype(p2)::value, decltype(wt)::value>), grid, dim3(SP_THREADS), 0,
                         eng->stream, N, (u32)mod, gr, (const u32 *)d_packed, d_weights, ps.os, NT, Pb, part, meta, d_out);
    };
#define SP_CASE(BITS) \
  case BITS: sum_variant(pow2, weighted, [&](auto p2, auto wt) { go(std::integral_constant<int, BITS>{}, p2, wt); }); break;
    switch (ps.bits) {
      case 1:                                           // mod = 2: a power of two
        weighted ? go(std::integral_constant<int, 1>{}, std::true_type{}, std::true_type{})
                 : go(std::integral_constant<int, 1>{}, std::true_type{}, std::false_type{});
        break;
      SP_CASE(2) SP_CASE(3) SP_CASE(4) SP_CASE(5) SP_CASE(6) SP_CASE(7) SP_CASE(8) SP_CASE(9) SP_CASE(10) SP_CASE(11) SP_CASE(12) SP_CASE(13)
      SP_CASE(14) SP_CASE(15) SP_CASE(16)
    }
#undef SP_CASE
  };
  if (int rc = launch_sum_rows(eng, N, mod, w, U <= 64 ? 1 : (U + 63) / 64, SP_WAVES_PER_CU, SP_THREADS, d_out, enqueue)) return rc;
  snprintf(eng->last_kernel, sizeof eng->last_kernel, "k_sum_groups_packed<%d,%d,%d>", ps.bits, (int)pow2, d_weights ? 1 : 0);
  return NTRU_OK;
}

// Enqueues the unpacking of B packed rows into dense rows.
int launch_unpack_rows(ntru_engine *eng, int N, const PackShape &ps, const uint64_t *d_packed, int64_t B, uint16_t *d_rows) {
  HIP_TRY(hipSetDevice(eng->device));
  hipLaunchKernelGGL(k_unpack_rows, elementwise_grid(eng, (long)B * N), dim3(256), 0, eng->stream, N, ps.bits, ps.per, ps.os,
                     (const u64 *)d_packed, (long)B, d_rows);
  HIP_TRY(hipGetLastError());
  return NTRU_OK;
}

}  // namespace

int ntru_launch_unpack_rows(ntru_engine *eng, int N, int q, const uint64_t *d_packed, int64_t B, uint16_t *d_rows) {
  PackShape ps;
  if (int rc = pack_shape(q, N, &ps)) return rc;
  return launch_unpack_rows(eng, N, ps, d_packed, B, d_rows);
}

extern "C" int ntru_sum_groups_packed_dev(ntru_engine_t *eng, int N, int mod, const uint64_t *d_packed, const uint16_t *d_weights,
                                          const int64_t *d_offsets, int64_t K, int64_t G, uint16_t *d_out) {
  if (int rc = ntru_check_sum_args(eng, N, mod, !d_offsets, K, G, "ntru_sum_groups_packed")) return rc;
  if (G == 0) return NTRU_OK;
  if (!d_packed || !d_out) return fail(NTRU_ERR_ARG, "ntru_sum_groups_packed: NULL buffer");
  const SumWindow w = {d_offsets, d_offsets ? 0 : K, 0, G, 0, 0x7fffffffffffffffL};
  return launch_sum_packed(eng, N, mod, d_packed, d_weights, w, d_out);
}

extern "C" int ntru_sum_groups_packed(ntru_engine_t *eng, int N, int mod, const uint64_t *packed, const uint16_t *weights,
                                      const int64_t *offsets, int64_t K, int64_t G, uint16_t *out) {
  PackShape ps = {1, 1, 3};
  if (N >= 2 && mod >= 2 && mod <= 65536) if (int rc = pack_shape(mod, N, &ps)) return rc;     // (anything else: refused by the checks)
  return ntru_sum_groups_host(eng, "ntru_sum_groups_packed", N, mod, packed, (size_t)ps.os * 32, weights, offsets, K, G, out,
                              launch_sum_packed);
}

extern "C" int ntru_tally_decrypt_packed_batch_dev(ntru_engine_t *eng, int N, int q, int p, const int8_t *d_f, const uint8_t *d_fp,
                                                   const uint64_t *d_packed, const uint16_t *d_weights, const int64_t *d_offsets,
                                                   int64_t K, int64_t G, uint16_t *d_sum, uint8_t *d_value, uint16_t *d_quot1,
                                                   uint16_t *d_rem1, uint8_t *d_quot2) {
  return tally_decrypt(
      eng, "ntru_tally_decrypt_packed_batch", N, q, p, !d_offsets, K, G, d_f && d_fp && d_packed && d_sum && d_value, "d_sum",
      [&] { return ntru_sum_groups_packed_dev(eng, N, q, d_packed, d_weights, d_offsets, K, G, d_sum); },
      [&] { return ntru_decrypt_batch_dev(eng, N, q, p, d_f, d_fp, d_sum, G, d_value, d_quot1, d_rem1, d_quot2); });
}

extern "C" int ntru_tally_decrypt_packed_batch(ntru_engine_t *eng, int N, int q, int p, const int8_t *f, const uint8_t *fp,
                                               const uint64_t *packed, const uint16_t *weights, const int64_t *offsets, int64_t K,
                                               int64_t G, uint16_t *sum, uint8_t *value, uint16_t *quot1, uint16_t *rem1, uint8_t *quot2) {
  return tally_decrypt(                                  // (packed is tested by ntru_sum_groups_host, once it knows that there are rows)
      eng, "ntru_tally_decrypt_packed_batch", N, q, p, !offsets, K, G, f && fp && sum && value, "sum",
      [&] { return ntru_sum_groups_packed(eng, N, q, packed, weights, offsets, K, G, sum); },
      [&] { return ntru_decrypt_batch(eng, N, q, p, f, fp, sum, G, value, quot1, rem1, quot2); });
}

// Rows are unpacked into the engine-owned scratch buffer, in passes of at most PK_PASS rows (its size is bounded in B), and are still on
// chip when the decrypt kernel, called as it is, reads them.
extern "C" int ntru_decrypt_packed_batch_dev(ntru_engine_t *eng, int N, int q, int p, const int8_t *d_f, const uint8_t *d_fp,
                                             const uint64_t *d_packed, int64_t B, uint8_t *d_value, uint16_t *d_quot1, uint16_t *d_rem1,
                                             uint8_t *d_quot2) {
  if (int rc = ntru_decrypt_batch_dev(eng, N, q, p, nullptr, nullptr, nullptr, 0, nullptr, nullptr, nullptr, nullptr)) return rc;
  if (B < 0) return fail(NTRU_ERR_ARG, "ntru_decrypt_packed_batch: negative batch size");
  if (B == 0) return NTRU_OK;
  if (!d_f || !d_fp || !d_packed || !d_value) return fail(NTRU_ERR_ARG, "ntru_decrypt_packed_batch: NULL buffer");
  PackShape ps;
  if (int rc = pack_shape(q, N, &ps)) return rc;
  ScratchHold hold(eng, (size_t)std::min<int64_t>(B, PK_PASS) * N * 2);
  if (hold.rc) return hold.rc;
  uint16_t *d_e = (uint16_t *)hold.p;
  return for_each_pass(B, PK_PASS, [&](int64_t o, int64_t n) -> int {
    if (int rc = launch_unpack_rows(eng, N, ps, d_packed + o * ps.os * 4, n, d_e)) return rc;
    return ntru_decrypt_batch_dev(eng, N, q, p, d_f, d_fp, d_e, n, d_value + o * N, rows_at(d_quot1, o * N), rows_at(d_rem1, o * N),
                                  rows_at(d_quot2, o * N));
  });
}

extern "C" int ntru_decrypt_packed_batch(ntru_engine_t *eng, int N, int q, int p, const int8_t *f, const uint8_t *fp, const uint64_t *packed,
                                         int64_t B, uint8_t *value, uint16_t *quot1, uint16_t *rem1, uint8_t *quot2) {
  if (int rc = ntru_decrypt_batch_dev(eng, N, q, p, nullptr, nullptr, nullptr, 0, nullptr, nullptr, nullptr, nullptr)) return rc;
  if (B < 0) return fail(NTRU_ERR_ARG, "ntru_decrypt_packed_batch: negative batch size");
  if (B == 0) return NTRU_OK;
  if (!f || !fp || !packed || !value) return fail(NTRU_ERR_ARG, "ntru_decrypt_packed_batch: NULL buffer");
  PackShape ps;
  if (int rc = pack_shape(q, N, &ps)) return rc;
  Pipeline P(eng);
  const int jf = P.in(f, N, true), jfp = P.in(fp, N, true), ip = P.in(packed, (size_t)ps.os * 32);
  const int iv = P.out(value, N), iq1 = P.out(quot1, (size_t)N * 2), ir1 = P.out(rem1, (size_t)N * 2), iq2 = P.out(quot2, N);
  return P.run(B, ntru_chunk_items(B), [&](int64_t, int64_t n, void **d) {
    return ntru_decrypt_packed_batch_dev(eng, N, q, p, (const int8_t *)d[jf], (const uint8_t *)d[jfp], (const uint64_t *)d[ip], n,
                                         (uint8_t *)d[iv], (uint16_t *)d[iq1], (uint16_t *)d[ir1], (uint8_t *)d[iq2]);
  });
}
