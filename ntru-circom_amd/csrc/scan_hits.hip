// scan_hits.hip -- scanning a batch of ciphertexts for the rows a key decrypts to a well-formed, tagged message (the read side of the
// README's "pad the message with data that can be confirmed during decryption"; decryptStr, index.js:84-86, on decryptBits,
// index.js:111-140): decrypt, test and compact on the device, so that only the hits cross the bus.  Kernels, *_dev entry points and
// the host-pointer forms (as ntru_pipeline_bytes_batch lives in message_bytes.hip).
//
//   row b is a hit for key k  <=>  ntru_rows_to_bytes of decryptBits(e[b]).value under key k gives flag byte 0 (the first 8 nbytes
//                                  coefficients are bits, every later one is 0) and bytes [tag_off, tag_off + tag_len) equal the tag
//
// Rows go in passes of at most 65536.  Per pass and key the existing calls run unchanged -- ntru_decrypt_batch_dev into scratch, then
// ntru_rows_to_bytes_dev into scratch -- and three select kernels follow on those bytes and flags, one lane per row, SC_ROWS rows per
// workgroup:
//   k_scan_mark     evaluates the predicate and leaves ONE hit count per workgroup (wave ballot, four counts added through the LDS);
//   k_scan_offsets  one workgroup: exclusive prefix sum of the (at most 256) block counts, plus the key's running count, which it then
//                   advances by the pass's total;
//   k_scan_emit     evaluates the predicate again; a hit's position is offset[block] + hits in the waves before it (LDS) + hits in
//                   the lanes below it (ballot + mbcnt).  The hits of a block are consecutive in the output, so the block stores
//                   their row indices one per lane and their bytes as ONE stretch, a byte per lane and step (hit_bytes rows start at
//                   any byte offset: nothing wider is assumed).  Positions >= max_hits are not stored.
// Positions come from prefix sums only: no global atomic, hence ascending row order and the same bytes whatever the launch shape.
// Every dependency between workgroups is a kernel boundary: no workgroup waits for another.
// The tag (at most NTRU_SCAN_MAX_TAG bytes) is read on the host when the call enqueues and reaches the kernels by value.
#include <hip/hip_runtime.h>

#include <cstdint>
#include <cstdio>
#include <cstring>
#include <string>

#include "kernels_common.h"

namespace {

constexpr int SC_ROWS = 256;                   // rows = lanes per workgroup of the select kernels
constexpr int64_t SC_PASS = 1 << 16;           // rows per pass, as the byte and packed calls
static_assert(SC_PASS / SC_ROWS <= SC_ROWS, "k_scan_offsets scans the block counts of a pass in one workgroup");

// Is row r of the pass a hit?  (ScanTag and the tag test are in kernels_common.h: count_bytes.hip classifies rows with them too.)
__device__ __forceinline__ bool row_hits(const uint8_t *__restrict__ bytes, const uint8_t *__restrict__ flags, int r, int nbytes,
                                         const ScanTag &tag) {
  if (flags[r] != 0) return false;
  return tag_matches(bytes + (long)r * nbytes, tag);
}

__global__ void __launch_bounds__(SC_ROWS) k_scan_mark(int nbytes, ScanTag tag, const uint8_t *__restrict__ bytes,
                                                       const uint8_t *__restrict__ flags, int n, u32 *__restrict__ counts) {
  __shared__ u32 s_wave[SC_ROWS / 64];
  const int tid = threadIdx.x, r = blockIdx.x * SC_ROWS + tid;
  const bool hit = r < n && row_hits(bytes, flags, r, nbytes, tag);
  const unsigned long long ballot = __ballot(hit);
  if ((tid & 63) == 0) s_wave[tid >> 6] = (u32)__popcll(ballot);
  __syncthreads();
  if (tid == 0) {
    u32 c = 0;
#pragma unroll
    for (int w = 0; w < SC_ROWS / 64; w++) c += s_wave[w];
    counts[blockIdx.x] = c;
  }
}

// One workgroup.  offsets[b] = *count + (sum of counts[0 .. b - 1]); then *count += sum of every counts[b].
__global__ void __launch_bounds__(SC_ROWS) k_scan_offsets(const u32 *__restrict__ counts, int nblocks, long long *__restrict__ offsets,
                                                          long long *count) {
  __shared__ u32 s_sum[SC_ROWS];
  const int tid = threadIdx.x;
  const u32 c = tid < nblocks ? counts[tid] : 0u;
  const long long base = *count;
  s_sum[tid] = c;
  __syncthreads();
  wg_inclusive_scan<SC_ROWS>(s_sum, tid);       // (its first barrier also orders every lane's read of *count before its update)
  if (tid < nblocks) offsets[tid] = base + (long long)(s_sum[tid] - c);
  if (tid == SC_ROWS - 1) *count = base + (long long)s_sum[tid];
}

// hit_row / hit_bytes are the key's own arrays; positions >= limit are not stored.
__global__ void __launch_bounds__(SC_ROWS) k_scan_emit(int nbytes, ScanTag tag, const uint8_t *__restrict__ bytes,
                                                       const uint8_t *__restrict__ flags, int n, long long row_base,
                                                       const long long *__restrict__ offsets, long long limit,
                                                       long long *__restrict__ hit_row, uint8_t *__restrict__ hit_bytes) {
  __shared__ u32 s_wave[SC_ROWS / 64];
  __shared__ u16 s_src[SC_ROWS];                // row (within the block) of the block's i-th hit
  const int tid = threadIdx.x, r0 = blockIdx.x * SC_ROWS, r = r0 + tid;
  const long long base = offsets[blockIdx.x];
  if (base >= limit) return;                    // uniform: the whole block lies behind the stored prefix
  const bool hit = r < n && row_hits(bytes, flags, r, nbytes, tag);
  const unsigned long long ballot = __ballot(hit);
  const u32 below = lanes_below(ballot);
  if ((tid & 63) == 0) s_wave[tid >> 6] = (u32)__popcll(ballot);
  __syncthreads();
  u32 before = 0, total = 0;
#pragma unroll
  for (int w = 0; w < SC_ROWS / 64; w++) {
    const u32 c = s_wave[w];
    if (w < (tid >> 6)) before += c;
    total += c;
  }
  if (total == 0) return;                       // uniform
  if (hit) s_src[before + below] = (u16)tid;
  __syncthreads();
  const int keep = (int)(limit - base < (long long)total ? limit - base : (long long)total);
  if (tid < keep) hit_row[base + tid] = row_base + r0 + s_src[tid];
  uint8_t *dst = hit_bytes + base * nbytes;
  const int len = keep * nbytes;
  for (int idx = tid; idx < len; idx += SC_ROWS) {
    const int i = idx / nbytes, j = idx - i * nbytes;
    dst[idx] = bytes[(long)(r0 + s_src[i]) * nbytes + j];
  }
}

// ---- host side --------------------------------------------------------------------------------------------------------------------

// The checks that need no engine, then the decrypt call's own (engine, (N, q), p).  `packed`: the rows arrive as packOutput rows.
int check_scan_args(const ntru_engine *eng, const char *who, bool packed, int N, int q, int p, int nbytes, int K, int64_t B, int tag_off,
                    int tag_len, const uint8_t *tag, int64_t max_hits, const void *hit_row, const void *hit_bytes, const void *count,
                    int *os) {
  const std::string name(who);
  if (N < 8 || N > NTRU_MAX_N) return fail(NTRU_ERR_ARG, name + ": need 8 <= N <= " + std::to_string(NTRU_MAX_N) + ", got N = " + std::to_string(N));
  if (nbytes < 1 || nbytes > N / 8)
    return fail(NTRU_ERR_ARG, name + ": need 1 <= nbytes <= N / 8 = " + std::to_string(N / 8) + ", got " + std::to_string(nbytes));
  if (B < 0) return fail(NTRU_ERR_ARG, name + ": negative batch size");
  if (K < 1) return fail(NTRU_ERR_ARG, name + ": need K >= 1 keys, got " + std::to_string(K));
  if (tag_len < 0 || tag_len > NTRU_SCAN_MAX_TAG)
    return fail(NTRU_ERR_ARG, name + ": need 0 <= tag_len <= " + std::to_string(NTRU_SCAN_MAX_TAG) + ", got " + std::to_string(tag_len));
  if (tag_off < 0 || tag_off > nbytes - tag_len)
    return fail(NTRU_ERR_ARG, name + ": the tag [" + std::to_string(tag_off) + ", " + std::to_string((long)tag_off + tag_len) +
                                  ") does not lie inside the " + std::to_string(nbytes) + " message bytes");
  if (tag_len > 0 && !tag) return fail(NTRU_ERR_ARG, name + ": tag is NULL");
  if (max_hits < 0) return fail(NTRU_ERR_ARG, name + ": negative max_hits");
  if (max_hits > 0 && (!hit_row || !hit_bytes)) return fail(NTRU_ERR_ARG, name + ": NULL hit buffer with max_hits > 0");
  if (!count) return fail(NTRU_ERR_ARG, name + ": count is NULL");
  if (int rc = ntru_decrypt_batch_dev(const_cast<ntru_engine *>(eng), N, q, p, nullptr, nullptr, nullptr, 0, nullptr, nullptr, nullptr, nullptr))
    return rc;
  *os = 0;
  if (packed) {
    int bits, per, al;
    if (int rc = ntru_pack_params(q - 1, N, &bits, &per, &al, os)) return rc;
  }
  return NTRU_OK;
}

// Enqueues the scan of B rows -- dense (os == 0: d_rows is uint16_t [B][N]) or packed (uint64_t [B][os][4]) -- under K keys on
// eng->stream.  Row b counts as row row_base + b; d_count [K] is advanced, not set; key k's hits go to d_hit_row + k * stride and
// d_hit_bytes + k * stride * nbytes, positions below `limit` only.
int scan_flow(ntru_engine *eng, int N, int q, int p, int nbytes, int K, const int8_t *d_f, const uint8_t *d_fp, const void *d_rows, int os,
              int64_t B, int64_t row_base, const ScanTag &tag, int64_t limit, int64_t stride, int64_t *d_hit_row, uint8_t *d_hit_bytes,
              int64_t *d_count) {
  HIP_TRY(hipSetDevice(eng->device));
  const int64_t pass = std::min<int64_t>(B, SC_PASS);
  const int max_blocks = (int)((pass + SC_ROWS - 1) / SC_ROWS);
  Carve c;
  const size_t at_unpacked = c.take(os ? (size_t)pass * N * 2 : 0), at_value = c.take((size_t)pass * N),
               at_bytes = c.take((size_t)pass * nbytes), at_flags = c.take((size_t)pass), at_counts = c.take((size_t)max_blocks * 4),
               at_offsets = c.take((size_t)max_blocks * 8);
  ScratchHold hold(eng, c.total);
  if (hold.rc) return hold.rc;
  uint16_t *d_unpacked = (uint16_t *)(hold.p + at_unpacked);
  uint8_t *d_value = (uint8_t *)hold.p + at_value, *d_bytes = (uint8_t *)hold.p + at_bytes, *d_flags = (uint8_t *)hold.p + at_flags;
  u32 *d_counts = (u32 *)(hold.p + at_counts);
  long long *d_offsets = (long long *)(hold.p + at_offsets);
  const int rc = for_each_pass(B, SC_PASS, [&](int64_t o, int64_t rows) -> int {
    const int n = (int)rows;
    const dim3 grid((unsigned)((n + SC_ROWS - 1) / SC_ROWS));
    const uint16_t *d_e = (const uint16_t *)d_rows + o * N;
    if (os) {
      if (int rc = ntru_launch_unpack_rows(eng, N, q, (const uint64_t *)d_rows + o * os * 4, n, d_unpacked)) return rc;
      d_e = d_unpacked;
    }
    for (int k = 0; k < K; k++) {
      if (int rc = ntru_decrypt_batch_dev(eng, N, q, p, d_f + (size_t)k * N, d_fp + (size_t)k * N, d_e, n, d_value, nullptr, nullptr, nullptr))
        return rc;
      if (int rc = ntru_rows_to_bytes_dev(eng, N, nbytes, d_value, n, d_bytes, d_flags)) return rc;
      hipLaunchKernelGGL(k_scan_mark, grid, dim3(SC_ROWS), 0, eng->stream, nbytes, tag, (const uint8_t *)d_bytes, (const uint8_t *)d_flags, n,
                         d_counts);
      hipLaunchKernelGGL(k_scan_offsets, dim3(1), dim3(SC_ROWS), 0, eng->stream, (const u32 *)d_counts, (int)grid.x, d_offsets,
                         (long long *)d_count + k);
      if (limit > 0)
        hipLaunchKernelGGL(k_scan_emit, grid, dim3(SC_ROWS), 0, eng->stream, nbytes, tag, (const uint8_t *)d_bytes, (const uint8_t *)d_flags,
                           n, (long long)(row_base + o), (const long long *)d_offsets, (long long)limit,
                           (long long *)d_hit_row + (size_t)k * stride, d_hit_bytes + (size_t)k * stride * nbytes);
      HIP_TRY(hipGetLastError());
    }
    return NTRU_OK;
  });
  if (rc) return rc;
  note_kernel(eng, limit > 0 ? "k_scan_emit" : "k_scan_offsets");
  return NTRU_OK;
}

int scan_dev(ntru_engine *eng, const char *who, bool packed, int N, int q, int p, int nbytes, int K, const int8_t *d_f, const uint8_t *d_fp,
             const void *d_rows, int64_t B, int tag_off, int tag_len, const uint8_t *tag, int64_t max_hits, int64_t *d_hit_row,
             uint8_t *d_hit_bytes, int64_t *d_count) {
  int os;
  if (int rc = check_scan_args(eng, who, packed, N, q, p, nbytes, K, B, tag_off, tag_len, tag, max_hits, d_hit_row, d_hit_bytes, d_count, &os))
    return rc;
  if (B > 0 && (!d_f || !d_fp || !d_rows)) return fail(NTRU_ERR_ARG, std::string(who) + ": NULL buffer");
  HIP_TRY(hipSetDevice(eng->device));
  HIP_TRY(hipMemsetAsync(d_count, 0, (size_t)K * 8, eng->stream));
  if (B == 0) return NTRU_OK;
  return scan_flow(eng, N, q, p, nbytes, K, d_f, d_fp, d_rows, os, B, 0, tag_of(tag_off, tag_len, tag), max_hits, max_hits, d_hit_row,
                   d_hit_bytes, d_count);
}

// The rows stream through the chunked pipeline with the K keys as shared inputs and no per-row output; the counts and the hit buffers
// stay on the device for the whole call (eng->shared_dev, [K][cap] with cap = min(max_hits, B)) and every chunk computes on one stream,
// in order.  Afterwards the K counts come down, then the stored prefix of each key's hits.
int scan_host(ntru_engine *eng, const char *who, bool packed, int N, int q, int p, int nbytes, int K, const int8_t *f, const uint8_t *fp,
              const void *rows, int64_t B, int tag_off, int tag_len, const uint8_t *tag, int64_t max_hits, int64_t *hit_row,
              uint8_t *hit_bytes, int64_t *count) {
  int os;
  if (int rc = check_scan_args(eng, who, packed, N, q, p, nbytes, K, B, tag_off, tag_len, tag, max_hits, hit_row, hit_bytes, count, &os))
    return rc;
  for (int k = 0; k < K; k++) count[k] = 0;
  if (B == 0) return NTRU_OK;
  if (!f || !fp || !rows) return fail(NTRU_ERR_ARG, std::string(who) + ": NULL buffer");
  HIP_TRY(hipSetDevice(eng->device));
  const int64_t cap = std::min<int64_t>(max_hits, B);
  Carve c;
  const size_t at_count = c.take((size_t)K * 8), at_row = c.take((size_t)K * cap * 8), at_bytes = c.take((size_t)K * cap * nbytes);
  ResidentHold hold(eng, who, c.total);
  if (hold.rc) return hold.rc;
  int64_t *d_count = (int64_t *)(hold.p + at_count), *d_hit_row = (int64_t *)(hold.p + at_row);
  uint8_t *d_hit_bytes = (uint8_t *)hold.p + at_bytes;
  HIP_TRY(hipMemset(d_count, 0, (size_t)K * 8));
  HIP_TRY(hipDeviceSynchronize());
  const ScanTag t = tag_of(tag_off, tag_len, tag);
  {
    Pipeline P(eng);
    const int jf = P.in(f, (size_t)K * N, true), jfp = P.in(fp, (size_t)K * N, true);
    const int ir = P.in(rows, os ? (size_t)os * 32 : (size_t)N * 2);
    if (int rc = P.run(B, ntru_chunk_items(B), [&](int64_t o, int64_t n, void **d) {
          return scan_flow(eng, N, q, p, nbytes, K, (const int8_t *)d[jf], (const uint8_t *)d[jfp], d[ir], os, n, o, t, cap, cap, d_hit_row,
                           d_hit_bytes, d_count);
        }))
      return rc;
  }
  HIP_TRY(hipMemcpy(count, d_count, (size_t)K * 8, hipMemcpyDeviceToHost));
  for (int k = 0; k < K; k++) {
    const int64_t stored = std::min<int64_t>(count[k], cap);
    if (stored == 0) continue;
    HIP_TRY(hipMemcpy(hit_row + (size_t)k * max_hits, d_hit_row + (size_t)k * cap, (size_t)stored * 8, hipMemcpyDeviceToHost));
    HIP_TRY(hipMemcpy(hit_bytes + (size_t)k * max_hits * nbytes, d_hit_bytes + (size_t)k * cap * nbytes, (size_t)stored * nbytes,
                      hipMemcpyDeviceToHost));
  }
  return NTRU_OK;
}

}  // namespace

extern "C" int ntru_scan_bytes_batch_dev(ntru_engine_t *eng, int N, int q, int p, int nbytes, int K, const int8_t *d_f, const uint8_t *d_fp,
                                         const uint16_t *d_e, int64_t B, int tag_off, int tag_len, const uint8_t *tag, int64_t max_hits,
                                         int64_t *d_hit_row, uint8_t *d_hit_bytes, int64_t *d_count) {
  return scan_dev(eng, "ntru_scan_bytes_batch", false, N, q, p, nbytes, K, d_f, d_fp, d_e, B, tag_off, tag_len, tag, max_hits, d_hit_row,
                  d_hit_bytes, d_count);
}

extern "C" int ntru_scan_bytes_packed_batch_dev(ntru_engine_t *eng, int N, int q, int p, int nbytes, int K, const int8_t *d_f,
                                                const uint8_t *d_fp, const uint64_t *d_packed, int64_t B, int tag_off, int tag_len,
                                                const uint8_t *tag, int64_t max_hits, int64_t *d_hit_row, uint8_t *d_hit_bytes,
                                                int64_t *d_count) {
  return scan_dev(eng, "ntru_scan_bytes_packed_batch", true, N, q, p, nbytes, K, d_f, d_fp, d_packed, B, tag_off, tag_len, tag, max_hits,
                  d_hit_row, d_hit_bytes, d_count);
}

extern "C" int ntru_scan_bytes_batch(ntru_engine_t *eng, int N, int q, int p, int nbytes, int K, const int8_t *f, const uint8_t *fp,
                                     const uint16_t *e, int64_t B, int tag_off, int tag_len, const uint8_t *tag, int64_t max_hits,
                                     int64_t *hit_row, uint8_t *hit_bytes, int64_t *count) {
  return scan_host(eng, "ntru_scan_bytes_batch", false, N, q, p, nbytes, K, f, fp, e, B, tag_off, tag_len, tag, max_hits, hit_row, hit_bytes,
                   count);
}

extern "C" int ntru_scan_bytes_packed_batch(ntru_engine_t *eng, int N, int q, int p, int nbytes, int K, const int8_t *f, const uint8_t *fp,
                                            const uint64_t *packed, int64_t B, int tag_off, int tag_len, const uint8_t *tag,
                                            int64_t max_hits, int64_t *hit_row, uint8_t *hit_bytes, int64_t *count) {
  return scan_host(eng, "ntru_scan_bytes_packed_batch", true, N, q, p, nbytes, K, f, fp, packed, B, tag_off, tag_len, tag, max_hits, hit_row,
                   hit_bytes, count);
}
