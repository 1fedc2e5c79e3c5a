// mix_audit.hip -- MI355X (gfx950): auditing a mix by checking revealed re-encryption links (include/ntru_engine.h "auditing a mix").
// Link l claims e_out[o] == r[l] * h + e_in[i] modulo (x^N - 1, q): the product k_reencrypt_m computes, compared against a row instead
// of stored.  k_linkcheck_m / k_linkcheck_md are the body of k_encrypt_m / k_encrypt_md (matrix_encrypt_body.h, AddCheckLinks) with the
// gathered e_in row as the epilogue's addend and a compare against the columns of e_out[o] in the place of the stores: r, both rows
// in, one flag byte out -- 5 N bytes per link.  Outside the matrix path's range (q > 8192, N > 1024, kernel paths 1-3) the vector-ALU
// encrypt runs on a zero message from the engine's scratch buffer and k_compare_links gathers both rows, tests r and writes the flag.
// The entry points, _dev and host-pointer form, are at the end of this file.
#include <algorithm>
#include <vector>

#include "matrix_encrypt_body.h"

constexpr size_t LINK_STAGE_BYTES = (size_t)WAVES_PER_BLOCK * 32 * ADD_ROW_PITCH;    // every wave's staged addend columns

// e_in and e_out are not __restrict__: they may be the same array (both are only read).
__global__ __launch_bounds__(BLOCK_THREADS, 2) void k_linkcheck_m(MGeom g, u32 q, const u16 *__restrict__ h,
                                                               const uint8_t *__restrict__ r, long L, AddCheckLinks links) {
  encrypt_m_body<4, false, AddCheckLinks>(g, q, h, r, nullptr, L, nullptr, nullptr, links);
}

__global__ __launch_bounds__(BLOCK_THREADS, 2) void k_linkcheck_md(MGeom g, u32 q, const u16 *__restrict__ h,
                                                                const uint8_t *__restrict__ r, long L, AddCheckLinks links) {
  encrypt_m_body<4, true, AddCheckLinks>(g, q, h, r, nullptr, L, nullptr, nullptr, links);
}

// The vector-ALU encrypt is given its documented operands only: a byte of r outside {0, 1, other} becomes 0 (that link is
// NTRU_LINK_BAD_R whatever its product).  One byte per thread.
__global__ void __launch_bounds__(256) k_clean_r(long total, u32 other, const uint8_t *__restrict__ r, uint8_t *__restrict__ clean) {
  for (long idx = (long)blockIdx.x * blockDim.x + threadIdx.x; idx < total; idx += (long)gridDim.x * blockDim.x) {
    const u32 b = r[idx];
    clean[idx] = (uint8_t)(b <= 1 || b == other ? b : 0u);
  }
}

// The flags of the n links of a pass from enc0[i] = Enc(0; r[first + i]): one wave per link, a lane per 64th column.  links.src /
// links.dst index the whole call's links, r is the caller's array (not the cleaned copy).  One atomic per workgroup counts the bad.
__global__ void __launch_bounds__(BLOCK_THREADS) k_compare_links(int N, u32 q, const u16 *__restrict__ enc0, const uint8_t *__restrict__ r,
                                                                 long first, long n, AddCheckLinks links) {
  __shared__ u32 wave_bad[WAVES_PER_BLOCK];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  u32 bad_links = 0;
  for (long i = (long)blockIdx.x * WAVES_PER_BLOCK + wave; i < n; i += (long)gridDim.x * WAVES_PER_BLOCK) {
    const long l = first + i;
    long in_ofs, out_ofs;
    const bool bad_index = links.link_offsets(l, first + n, N, in_ofs, out_ofs);
    const uint8_t *rr = r + l * N;
    const u16 *mine = enc0 + i * N;
    u32 pair = 0, diff = 0;
    bool outside = false;
    for (int c = lane; c < N; c += 64) {
      const u32 b = rr[c];
      pair += (b == 1u ? 1u : 0u) + (b == (u32)links.other ? 0x10000u : 0u);
      outside |= !(b <= 1u || b == (u32)links.other);
      if (!bad_index) diff |= (((u32)mine[c] + links.e_in[in_ofs + c]) ^ links.e_out[out_ofs + c]) & (q - 1);
    }
#pragma unroll
    for (int s = 32; s > 0; s >>= 1) pair += (u32)__shfl_xor((int)pair, s, 64);
    const bool any_outside = __ballot(outside) != 0, any_diff = __ballot(diff != 0) != 0;
    u32 fl = (bad_index ? 1u : 0u) | links.r_verdict(any_outside, (int)(pair & 0xFFFFu), (int)(pair >> 16));
    if (fl == 0 && any_diff) fl = 4u;
    if (lane == 0) links.flags[l] = (uint8_t)fl;
    bad_links += fl != 0 ? 1u : 0u;
  }
  if (lane == 0) wave_bad[wave] = bad_links;
  __syncthreads();
  if (threadIdx.x == 0 && links.n_bad) {
    u32 total = 0;
    for (int w = 0; w < WAVES_PER_BLOCK; w++) total += wave_bad[w];
    if (total) atomicAdd(links.n_bad, (unsigned long long)total);
  }
}

namespace {

constexpr int64_t LINK_PASS = 65536;     // links per pass of the vector-ALU route (bounds the scratch it takes)

// Kernel paths and the md / m rule as for launch_reencrypt_matrix.  LDS: what k_reencrypt_m takes plus the 512 bytes of the check's
// tables.
int launch_linkcheck_matrix(ntru_engine *eng, int N, int q, const uint16_t *d_h, const uint8_t *d_r, int64_t L, const AddCheckLinks &links) {
  MGeom mg;
  if (!make_mgeom(eng, N, q, N, &mg)) return NTRU_NOT_TAKEN;
  const size_t lds = (size_t)32 * mg.tpitch + (size_t)32 * mg.pitchA + 256 + LINK_STAGE_BYTES + CHECK_TABLE_BYTES + 16;
  if (lds > 160 * 1024) return NTRU_NOT_TAKEN;
  const long nrb = (long)((L + 31) / 32);
  const bool rows_dword_aligned = (N & 3) == 0 && ((uintptr_t)d_r & 3) == 0;
  const bool md = eng->path != 4 && (N + 3 <= 1024 || (rows_dword_aligned && N <= 1024));
  note_kernel(eng, md ? "k_linkcheck_md" : "k_linkcheck_m");
  return launch_resident(eng, md ? k_linkcheck_md : k_linkcheck_m, nrb, BLOCK_THREADS, lds, mg, (u32)q, d_h, d_r, (long)L, links);
}

// Per pass: r cleaned into scratch, Enc(0; r) of the pass beside it, then the compare.
int launch_linkcheck_valu(ntru_engine *eng, int N, int q, const uint16_t *d_h, const uint8_t *d_r, int64_t L, const AddCheckLinks &links) {
  const int64_t pass = std::min<int64_t>(L, LINK_PASS);
  Carve c;
  const size_t at_zero = c.take((size_t)pass * N), at_clean = c.take((size_t)pass * N), at_enc0 = c.total;
  ScratchHold hold(eng, at_enc0 + (size_t)pass * N * 2);          // (the last array is not rounded up)
  if (hold.rc) return hold.rc;
  uint8_t *d_zero = (uint8_t *)hold.p + at_zero, *d_clean = (uint8_t *)hold.p + at_clean;
  uint16_t *d_enc0 = (uint16_t *)(hold.p + at_enc0);
  HIP_TRY(hipMemsetAsync(d_zero, 0, (size_t)pass * N, eng->stream));
  const int rc = for_each_pass(L, LINK_PASS, [&](int64_t o, int64_t n) -> int {
    hipLaunchKernelGGL(k_clean_r, elementwise_grid(eng, (long)n * N), dim3(256), 0, eng->stream, (long)n * N, (u32)links.other, d_r + o * N,
                       d_clean);
    HIP_TRY(hipGetLastError());
    if (int rc = ntru_launch_encrypt_valu(eng, N, q, d_h, d_clean, d_zero, n, d_enc0, nullptr)) return rc;
    const long blocks = (long)((n + WAVES_PER_BLOCK - 1) / WAVES_PER_BLOCK), cap = (long)eng->cus * 8;
    hipLaunchKernelGGL(k_compare_links, dim3((unsigned)std::min(blocks, cap)), dim3(BLOCK_THREADS), 0, eng->stream, N, (u32)q, d_enc0, d_r,
                       (long)o, (long)n, links);
    HIP_TRY(hipGetLastError());
    return NTRU_OK;
  });
  if (rc) return rc;
  note_kernel(eng, "k_compare_links");
  return NTRU_OK;
}

// The checks both forms share; *done: nothing to launch (L == 0).
int check_links_args(ntru_engine *eng, int N, int q, int other, int n1, int n2, const void *h, const uint8_t *r, const uint16_t *e_in,
                     int64_t B_in, const int64_t *in_idx, const uint16_t *e_out, int64_t B_out, const int64_t *out_idx, int64_t L,
                     const uint8_t *flags, const int64_t *n_bad, bool *done) {
  *done = false;
  if (int rc = ntru_check_common(eng, N, q, L)) return rc;
  if (B_in < 0 || B_out < 0) return fail(NTRU_ERR_ARG, "ntru_check_links_batch: negative row count");
  if (other < 1 || other > 3) return fail(NTRU_ERR_ARG, "ntru_check_links_batch: other must be 1, 2 or 3, got " + std::to_string(other));
  if ((long)std::max(n1, 0) + std::max(n2, 0) > N) return fail(NTRU_ERR_ARG, "ntru_check_links_batch: n1 + n2 exceeds N");
  if (L == 0) { *done = true; return NTRU_OK; }
  if (!h || !r || !e_in || !e_out || !flags) return fail(NTRU_ERR_ARG, "ntru_check_links_batch: NULL buffer");
  const struct { const void *p; size_t n; } inputs[] = {{h, (size_t)N * 2}, {r, (size_t)L * N}, {e_in, (size_t)B_in * N * 2},
                                                        {e_out, (size_t)B_out * N * 2}, {in_idx, (size_t)L * 8}, {out_idx, (size_t)L * 8}};
  for (const auto &in : inputs)
    if (ntru_ranges_overlap(in.p, in.n, flags, (size_t)L) || ntru_ranges_overlap(in.p, in.n, n_bad, 8))
      return fail(NTRU_ERR_ARG, "ntru_check_links_batch: flags or n_bad overlaps an input");
  if (ntru_ranges_overlap(flags, (size_t)L, n_bad, 8)) return fail(NTRU_ERR_ARG, "ntru_check_links_batch: flags and n_bad overlap");
  return NTRU_OK;
}

}  // namespace

extern "C" int ntru_check_links_batch_dev(ntru_engine_t *eng, int N, int q, int other, int n1, int n2, const uint16_t *d_h, const uint8_t *d_r,
                                          const uint16_t *d_e_in, int64_t B_in, const int64_t *d_in_idx, const uint16_t *d_e_out,
                                          int64_t B_out, const int64_t *d_out_idx, int64_t L, uint8_t *d_flags, int64_t *d_n_bad) {
  bool done;
  if (int rc = check_links_args(eng, N, q, other, n1, n2, d_h, d_r, d_e_in, B_in, d_in_idx, d_e_out, B_out, d_out_idx, L, d_flags, d_n_bad,
                                &done))
    return rc;
  HIP_TRY(hipSetDevice(eng->device));
  if (d_n_bad) HIP_TRY(hipMemsetAsync(d_n_bad, 0, sizeof(int64_t), eng->stream));
  if (done) return NTRU_OK;
  const AddCheckLinks links = {d_e_in, (long)B_in, (const long *)d_in_idx, d_e_out, (long)B_out, (const long *)d_out_idx, other, n1, n2,
                               d_flags, (unsigned long long *)d_n_bad};
  const int rc = launch_linkcheck_matrix(eng, N, q, d_h, d_r, L, links);
  if (rc != NTRU_NOT_TAKEN) return rc;
  return launch_linkcheck_valu(eng, N, q, d_h, d_r, L, links);
}

// The host form gathers both rows of every link while it fills the staging buffers, one chunk's links at a time, so the device sees
// the identity on both sides -- and -1 on both for a link with an index outside its array, which the kernels then flag without
// reading a row.  n_bad is counted from the flags that came down.
extern "C" int ntru_check_links_batch(ntru_engine_t *eng, int N, int q, int other, int n1, int n2, const uint16_t *h, const uint8_t *r,
                                      const uint16_t *e_in, int64_t B_in, const int64_t *in_idx, const uint16_t *e_out, int64_t B_out,
                                      const int64_t *out_idx, int64_t L, uint8_t *flags, int64_t *n_bad) {
  bool done;
  if (int rc = check_links_args(eng, N, q, other, n1, n2, h, r, e_in, B_in, in_idx, e_out, B_out, out_idx, L, flags, n_bad, &done)) return rc;
  if (n_bad) *n_bad = 0;
  if (done) return NTRU_OK;
  const size_t row = (size_t)N * 2;
  const int64_t C = std::min(ntru_chunk_items(L), L);
  std::vector<uint16_t> rows_in((size_t)C * N), rows_out((size_t)C * N);
  std::vector<int64_t> idx((size_t)C);
  for (int64_t o = 0; o < L; o += C) {                    // one pipeline run per chunk, on the rows gathered for it
    const int64_t n = std::min(C, L - o);
    for (int64_t k = 0; k < n; k++) {
      const int64_t i = in_idx ? in_idx[o + k] : o + k, t = out_idx ? out_idx[o + k] : o + k;
      const bool inside = i >= 0 && i < B_in && t >= 0 && t < B_out;
      idx[k] = inside ? k : -1;
      if (inside) {
        memcpy(rows_in.data() + (size_t)k * N, e_in + (size_t)i * N, row);
        memcpy(rows_out.data() + (size_t)k * N, e_out + (size_t)t * N, row);
      } else {
        memset(rows_in.data() + (size_t)k * N, 0, row);
        memset(rows_out.data() + (size_t)k * N, 0, row);
      }
    }
    Pipeline P(eng);
    const int ih = P.in(h, row, true), ir = P.in(r + o * N, N), ii = P.in(rows_in.data(), row), io = P.in(rows_out.data(), row);
    const int ix = P.in(idx.data(), sizeof(int64_t)), ifl = P.out(flags + o, 1);
    const int rc = P.run(n, C, [&](int64_t, int64_t cnt, void **d) {
      return ntru_check_links_batch_dev(eng, N, q, other, n1, n2, (const uint16_t *)d[ih], (const uint8_t *)d[ir], (const uint16_t *)d[ii], cnt,
                                        (const int64_t *)d[ix], (const uint16_t *)d[io], cnt, (const int64_t *)d[ix], cnt, (uint8_t *)d[ifl],
                                        nullptr);
    });
    if (rc) return rc;
  }
  if (n_bad) *n_bad = (int64_t)std::count_if(flags, flags + L, [](uint8_t f) { return f != 0; });
  return NTRU_OK;
}
