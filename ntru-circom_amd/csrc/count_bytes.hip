// count_bytes.hip -- counting the decrypted byte messages of a batch by choice and group (the end of a ballot pipeline: after the last
// mix step every row is decrypted, the choice is read out of the message and counted; decryptStr, index.js:84-86, on decryptBits,
// index.js:111-140): decrypt once, classify every row on the device, and return only the table count[G][n_choices + 3] and, when asked
// for, one class id per row.  Kernel, *_dev entry points and the host-pointer forms (as scan_hits.hip has them).
//
//   cls(b), for bytes / flag = ntru_rows_to_bytes of decryptBits(e[b]).value under the key, is the first that applies of
//     flag != 0                                                        NTRU_COUNT_MALFORMED = n_choices + 2
//     bytes [tag_off, tag_off + tag_len) differ from the tag            NTRU_COUNT_BAD_TAG   = n_choices + 1
//     v = big-endian bytes [field_off, field_off + field_len);
//       v < first_choice or v - first_choice >= n_choices               NTRU_COUNT_OTHER     = n_choices
//     otherwise                                                         v - first_choice
//   count[g][c] = rows with group == g and cls == c; a row whose group id lies outside [0, G) is counted nowhere and has cls -1.
//
// Rows go in passes of at most 65536.  Per pass the existing calls run unchanged -- ntru_decrypt_batch_dev into scratch, then
// ntru_rows_to_bytes_dev into scratch -- and ONE kernel follows on those bytes and flags, k_count_classify, one lane per row: a
// persistent grid of at most CT_WG_PER_CU workgroups per CU, each walking the CT_ROWS-row tiles of the pass in a grid-stride loop.
// A row's bin is accumulated one of two ways, chosen by the launcher:
//   G * n_bins <= CT_LDS_BINS   a workgroup-private histogram of u32 counters in LDS (a pass has at most 65536 rows: no overflow), zeroed
//                               once, added to with LDS atomics over all the workgroup's tiles, flushed at the end with one 64-bit
//                               global atomic add per NON-ZERO bin, consecutive lanes on consecutive bins;
//   larger tables               one 64-bit global atomic add per row, straight into count.
// Integer adds commute: the bytes of count and cls are the same whatever the launch shape, the pass size, the route and the chunking.
// Nothing here needs positions, so there is no ordering between workgroups and no sort.
// The tag (at most NTRU_SCAN_MAX_TAG bytes) is read on the host when the call enqueues; tag and field reach the kernel by value.
#include <hip/hip_runtime.h>

#include <cstdint>
#include <cstdio>
#include <cstring>
#include <string>

#include "kernels_common.h"

namespace {

constexpr int CT_ROWS = 256;                   // rows = lanes per tile and workgroup
constexpr int64_t CT_PASS = 1 << 16;           // rows per pass, as the byte, packed and scan calls
constexpr int CT_WG_PER_CU = 2;                // the persistent grid: at most this many workgroups per CU
constexpr int CT_LDS_BINS = 8192;              // u32 counters of the workgroup-private histogram: 32 KB of LDS
static_assert(CT_PASS < (1ll << 32), "a u32 counter of the LDS histogram holds the rows of a pass");
static_assert(NTRU_COUNT_MAX_BINS <= (1 << 24) && NTRU_COUNT_MAX_CHOICES <= (1 << 16), "a bin index is an int");

struct CountField {
  int off, len;                                // 1 <= len <= 4 message bytes, big-endian
  u32 first, n_choices;
};

// cls of row r of the pass, its group aside.
__device__ __forceinline__ int row_class(const uint8_t *__restrict__ bytes, const uint8_t *__restrict__ flags, int r, int nbytes,
                                         const ScanTag &tag, const CountField &fld) {
  if (flags[r] != 0) return (int)fld.n_choices + 2;
  const uint8_t *m = bytes + (long)r * nbytes;
  if (!tag_matches(m, tag)) return (int)fld.n_choices + 1;
  u32 v = 0;
#pragma unroll
  for (int j = 0; j < 4; j++)
    if (j < fld.len) v = (v << 8) | m[fld.off + j];
  // v and first_choice are below 2^32 and n_choices at most 2^16: with v >= first the difference is exact in 32 bits, which is the
  // comparison of first_choice + n_choices in 64
  return v >= fld.first && v - fld.first < fld.n_choices ? (int)(v - fld.first) : (int)fld.n_choices;
}

// group [n] (or NULL: every row in group 0), cls [n] (or NULL) and the bytes and flags belong to the n rows of one pass; count is the
// whole table [G][n_bins].  LDS: bins = G * n_bins <= CT_LDS_BINS.
template <bool LDS>
__global__ void __launch_bounds__(CT_ROWS) k_count_classify(int nbytes, ScanTag tag, CountField fld, int G, const uint8_t *__restrict__ bytes,
                                                            const uint8_t *__restrict__ flags, const int *__restrict__ group, int n,
                                                            int *__restrict__ cls, unsigned long long *__restrict__ count) {
  __shared__ u32 s_hist[LDS ? CT_LDS_BINS : 1];
  const int tid = threadIdx.x, n_bins = (int)fld.n_choices + 3, bins = G * n_bins;
  if (LDS) {
    for (int i = tid; i < bins; i += CT_ROWS) s_hist[i] = 0u;
    __syncthreads();
  }
  const int tiles = (n + CT_ROWS - 1) / CT_ROWS;
  for (int t = blockIdx.x; t < tiles; t += gridDim.x) {
    const int r = t * CT_ROWS + tid;
    if (r >= n) continue;
    const int g = group ? group[r] : 0;
    const bool counted = (u32)g < (u32)G;
    const int c = counted ? row_class(bytes, flags, r, nbytes, tag, fld) : -1;
    if (cls) cls[r] = c;
    if (!counted) continue;
    const int bin = g * n_bins + c;
    if (LDS) atomicAdd(&s_hist[bin], 1u);
    else atomicAdd(&count[bin], 1ull);
  }
  if (LDS) {
    __syncthreads();
    for (int i = tid; i < bins; i += CT_ROWS) {
      const u32 v = s_hist[i];
      if (v) atomicAdd(&count[i], (unsigned long long)v);
    }
  }
}

// ---- host side --------------------------------------------------------------------------------------------------------------------

struct CountArgs {
  int N, q, p, nbytes;
  const void *f, *fp, *rows;
  int64_t B;
  int tag_off, tag_len;
  const uint8_t *tag;
  int field_off, field_len;
  uint64_t first_choice;
  int n_choices, G;
  const int32_t *group;
  int64_t *count;
  int32_t *cls;
  int n_bins() const { return n_choices + 3; }
  size_t table_bytes() const { return (size_t)G * n_bins() * 8; }
};

// The checks that need no engine, each with a message of its own, then the decrypt call's own (engine, (N, q), p).  `packed`: the
// rows arrive as packOutput rows.  `host`: the arrays are host memory, so the group ids are read and checked here.
int check_count_args(const ntru_engine *eng, const char *who, bool packed, bool host, const CountArgs &a, int *os) {
  const std::string name(who);
  if (a.N < 8 || a.N > NTRU_MAX_N)
    return fail(NTRU_ERR_ARG, name + ": need 8 <= N <= " + std::to_string(NTRU_MAX_N) + ", got N = " + std::to_string(a.N));
  if (a.nbytes < 1 || a.nbytes > a.N / 8)
    return fail(NTRU_ERR_ARG, name + ": need 1 <= nbytes <= N / 8 = " + std::to_string(a.N / 8) + ", got " + std::to_string(a.nbytes));
  if (a.B < 0) return fail(NTRU_ERR_ARG, name + ": negative batch size");
  if (a.tag_len < 0 || a.tag_len > NTRU_SCAN_MAX_TAG)
    return fail(NTRU_ERR_ARG, name + ": need 0 <= tag_len <= " + std::to_string(NTRU_SCAN_MAX_TAG) + ", got " + std::to_string(a.tag_len));
  if (a.tag_off < 0 || a.tag_off > a.nbytes - a.tag_len)
    return fail(NTRU_ERR_ARG, name + ": the tag [" + std::to_string(a.tag_off) + ", " + std::to_string((long)a.tag_off + a.tag_len) +
                                  ") does not lie inside the " + std::to_string(a.nbytes) + " message bytes");
  if (a.tag_len > 0 && !a.tag) return fail(NTRU_ERR_ARG, name + ": tag is NULL");
  if (a.field_len < 1 || a.field_len > 4)
    return fail(NTRU_ERR_ARG, name + ": need 1 <= field_len <= 4, got " + std::to_string(a.field_len));
  if (a.field_off < 0 || a.field_off > a.nbytes - a.field_len)
    return fail(NTRU_ERR_ARG, name + ": the choice field [" + std::to_string(a.field_off) + ", " +
                                  std::to_string((long)a.field_off + a.field_len) + ") does not lie inside the " +
                                  std::to_string(a.nbytes) + " message bytes");
  if (a.first_choice >> 32) return fail(NTRU_ERR_ARG, name + ": first_choice = " + std::to_string(a.first_choice) + " does not fit 32 bits");
  if (a.n_choices < 1 || a.n_choices > NTRU_COUNT_MAX_CHOICES)
    return fail(NTRU_ERR_ARG, name + ": need 1 <= n_choices <= " + std::to_string(NTRU_COUNT_MAX_CHOICES) + ", got " + std::to_string(a.n_choices));
  if (a.G < 1) return fail(NTRU_ERR_ARG, name + ": need G >= 1 groups, got " + std::to_string(a.G));
  if ((int64_t)a.G * a.n_bins() > NTRU_COUNT_MAX_BINS)
    return fail(NTRU_ERR_ARG, name + ": G * (n_choices + 3) = " + std::to_string((int64_t)a.G * a.n_bins()) + " bins exceed " +
                                  std::to_string(NTRU_COUNT_MAX_BINS));
  if (!a.group && a.G > 1) return fail(NTRU_ERR_ARG, name + ": group is NULL with G = " + std::to_string(a.G) + " groups");
  if (!a.count) return fail(NTRU_ERR_ARG, name + ": count is NULL");
  if (a.B > 0 && (!a.f || !a.fp || !a.rows)) return fail(NTRU_ERR_ARG, name + ": NULL buffer");
  if (ntru_ranges_overlap(a.count, a.table_bytes(), a.cls, (size_t)a.B * 4)) return fail(NTRU_ERR_ARG, name + ": count and cls overlap");
  if (host && a.group)
    for (int64_t b = 0; b < a.B; b++)
      if (a.group[b] < 0 || a.group[b] >= a.G)
        return fail(NTRU_ERR_ARG, name + ": group[" + std::to_string(b) + "] = " + std::to_string(a.group[b]) + " is outside [0, G)");
  if (int rc = ntru_decrypt_batch_dev(const_cast<ntru_engine *>(eng), a.N, a.q, a.p, nullptr, nullptr, nullptr, 0, nullptr, nullptr, nullptr,
                                      nullptr))
    return rc;
  *os = 0;
  if (packed) {
    int bits, per, al;
    if (int rc = ntru_pack_params(a.q - 1, a.N, &bits, &per, &al, os)) return rc;
  }
  return NTRU_OK;
}

// Enqueues the classification of B rows -- dense (os == 0: d_rows is uint16_t [B][N]) or packed (uint64_t [B][os][4]) -- on eng->stream.
// d_group [B] and d_cls [B] may be NULL; d_count [G][n_bins] is added to, not set.
int count_flow(ntru_engine *eng, const CountArgs &a, const int8_t *d_f, const uint8_t *d_fp, const void *d_rows, int os, int64_t B,
               const ScanTag &tag, const int32_t *d_group, int32_t *d_cls, int64_t *d_count) {
  HIP_TRY(hipSetDevice(eng->device));
  const int N = a.N, nbytes = a.nbytes;
  const int64_t pass = std::min<int64_t>(B, CT_PASS);
  Carve c;
  const size_t at_unpacked = c.take(os ? (size_t)pass * N * 2 : 0), at_value = c.take((size_t)pass * N),
               at_bytes = c.take((size_t)pass * nbytes), at_flags = c.take((size_t)pass);
  ScratchHold hold(eng, c.total);
  if (hold.rc) return hold.rc;
  uint16_t *d_unpacked = (uint16_t *)(hold.p + at_unpacked);
  uint8_t *d_value = (uint8_t *)hold.p + at_value, *d_bytes = (uint8_t *)hold.p + at_bytes, *d_flags = (uint8_t *)hold.p + at_flags;
  const CountField fld = {a.field_off, a.field_len, (u32)a.first_choice, (u32)a.n_choices};
  const auto kern = (int64_t)a.G * a.n_bins() <= CT_LDS_BINS ? k_count_classify<true> : k_count_classify<false>;
  const int rc = for_each_pass(B, CT_PASS, [&](int64_t o, int64_t rows) -> int {
    const int n = (int)rows;
    const uint16_t *d_e = (const uint16_t *)d_rows + o * N;
    if (os) {
      if (int rc = ntru_launch_unpack_rows(eng, N, a.q, (const uint64_t *)d_rows + o * os * 4, n, d_unpacked)) return rc;
      d_e = d_unpacked;
    }
    if (int rc = ntru_decrypt_batch_dev(eng, N, a.q, a.p, d_f, d_fp, d_e, n, d_value, nullptr, nullptr, nullptr)) return rc;
    if (int rc = ntru_rows_to_bytes_dev(eng, N, nbytes, d_value, n, d_bytes, d_flags)) return rc;
    const int tiles = (n + CT_ROWS - 1) / CT_ROWS;
    const dim3 grid((unsigned)std::min(tiles, eng->cus * CT_WG_PER_CU));
    hipLaunchKernelGGL(kern, grid, dim3(CT_ROWS), 0, eng->stream, nbytes, tag, fld, a.G,
                       (const uint8_t *)d_bytes, (const uint8_t *)d_flags, (const int *)rows_at(d_group, o), n, (int *)rows_at(d_cls, o),
                       (unsigned long long *)d_count);
    HIP_TRY(hipGetLastError());
    return NTRU_OK;
  });
  if (rc) return rc;
  note_kernel(eng, "k_count_classify");
  return NTRU_OK;
}

int count_dev(ntru_engine *eng, const char *who, bool packed, const CountArgs &a) {
  int os;
  if (int rc = check_count_args(eng, who, packed, false, a, &os)) return rc;
  HIP_TRY(hipSetDevice(eng->device));
  HIP_TRY(hipMemsetAsync(a.count, 0, a.table_bytes(), eng->stream));
  if (a.B == 0) return NTRU_OK;
  return count_flow(eng, a, (const int8_t *)a.f, (const uint8_t *)a.fp, a.rows, os, a.B, tag_of(a.tag_off, a.tag_len, a.tag), a.group, a.cls,
                    a.count);
}

// The rows, and the group ids when given, stream through the chunked pipeline with the key as shared inputs and cls as a per-row
// output; the table stays on the device for the whole call (eng->shared_dev) and every chunk computes on one stream, in order.
// Afterwards the table comes down once.
int count_host(ntru_engine *eng, const char *who, bool packed, const CountArgs &a) {
  int os;
  if (int rc = check_count_args(eng, who, packed, true, a, &os)) return rc;
  memset(a.count, 0, a.table_bytes());
  if (a.B == 0) return NTRU_OK;
  HIP_TRY(hipSetDevice(eng->device));
  ResidentHold hold(eng, who, a.table_bytes());
  if (hold.rc) return hold.rc;
  int64_t *d_count = (int64_t *)hold.p;
  HIP_TRY(hipMemset(d_count, 0, a.table_bytes()));
  HIP_TRY(hipDeviceSynchronize());
  const ScanTag t = tag_of(a.tag_off, a.tag_len, a.tag);
  {
    Pipeline P(eng);
    const int jf = P.in(a.f, (size_t)a.N, true), jfp = P.in(a.fp, (size_t)a.N, true);
    const int ir = P.in(a.rows, os ? (size_t)os * 32 : (size_t)a.N * 2);
    const int ig = a.group ? P.in(a.group, 4) : -1, ic = a.cls ? P.out(a.cls, 4) : -1;
    if (int rc = P.run(a.B, ntru_chunk_items(a.B), [&](int64_t, int64_t n, void **d) {
          return count_flow(eng, a, (const int8_t *)d[jf], (const uint8_t *)d[jfp], d[ir], os, n, t, ig < 0 ? nullptr : (const int32_t *)d[ig],
                            ic < 0 ? nullptr : (int32_t *)d[ic], d_count);
        }))
      return rc;
  }
  HIP_TRY(hipMemcpy(a.count, d_count, a.table_bytes(), hipMemcpyDeviceToHost));
  return NTRU_OK;
}

}  // namespace

#define COUNT_ARGS(rows) \
  {N, q, p, nbytes, f, fp, rows, B, tag_off, tag_len, tag, field_off, field_len, first_choice, n_choices, G, group, count, cls}

extern "C" int ntru_count_bytes_batch_dev(ntru_engine_t *eng, int N, int q, int p, int nbytes, const int8_t *f, const uint8_t *fp,
                                          const uint16_t *e, int64_t B, int tag_off, int tag_len, const uint8_t *tag, int field_off,
                                          int field_len, uint64_t first_choice, int n_choices, int G, const int32_t *group, int64_t *count,
                                          int32_t *cls) {
  return count_dev(eng, "ntru_count_bytes_batch", false, COUNT_ARGS(e));
}

extern "C" int ntru_count_bytes_packed_batch_dev(ntru_engine_t *eng, int N, int q, int p, int nbytes, const int8_t *f, const uint8_t *fp,
                                                 const uint64_t *packed, int64_t B, int tag_off, int tag_len, const uint8_t *tag,
                                                 int field_off, int field_len, uint64_t first_choice, int n_choices, int G,
                                                 const int32_t *group, int64_t *count, int32_t *cls) {
  return count_dev(eng, "ntru_count_bytes_packed_batch", true, COUNT_ARGS(packed));
}

extern "C" int ntru_count_bytes_batch(ntru_engine_t *eng, int N, int q, int p, int nbytes, const int8_t *f, const uint8_t *fp,
                                      const uint16_t *e, int64_t B, int tag_off, int tag_len, const uint8_t *tag, int field_off,
                                      int field_len, uint64_t first_choice, int n_choices, int G, const int32_t *group, int64_t *count,
                                      int32_t *cls) {
  return count_host(eng, "ntru_count_bytes_batch", false, COUNT_ARGS(e));
}

extern "C" int ntru_count_bytes_packed_batch(ntru_engine_t *eng, int N, int q, int p, int nbytes, const int8_t *f, const uint8_t *fp,
                                             const uint64_t *packed, int64_t B, int tag_off, int tag_len, const uint8_t *tag,
                                             int field_off, int field_len, uint64_t first_choice, int n_choices, int G,
                                             const int32_t *group, int64_t *count, int32_t *cls) {
  return count_host(eng, "ntru_count_bytes_packed_batch", true, COUNT_ARGS(packed));
}
