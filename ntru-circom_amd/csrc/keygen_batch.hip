// keygen_batch.hip -- key generation as one batched call: generatePrivateKeyF + generateNewPublicKeyGH (index.js:51-79) for B items,
// with non-units redrawn on the device (ntru_keygen_batch[_dev], include/ntru_engine.h).
//
// The chain: g and the first f of every item from k_sample_ternary (ntru_sample_ternary_dev), fq / fp from ntru_invert_key_batch_dev,
// then the redraw passes, then h from ntru_public_key_batch_dev over the whole batch.  A redraw pass:
//   k_keygen_compact          flags -> list of the items still waiting for attempt t (wave ballot + prefix, one atomic per wave) + count
//   k_sample_ternary (listed) attempt t of every listed item into compact rows (position (t << 44) + item: its own, whatever else failed),
//                             through ntru_launch_sample_listed (ternary_sampler.hip)
//   ntru_invert_key_batch_dev the compact rows
//   k_keygen_scatter          compact rows back to their items: f, tries and flags always, fq / fp where the new f is a unit
// An item that still waits carries a parity mark (bit 0 of its flags byte: t & 1 after a failed attempt t), so that a pass of at most
// KG_PASS_ROWS rows can leave the rest of attempt t's items for the next pass without confusing them with the items that just failed
// attempt t.  k_keygen_finalize clears the marks and zeroes fq / fp of the items that never drew a unit.
#include "kernels_common.h"

namespace {

constexpr int KG_PASS_ROWS = 4096;            // compact rows per redraw pass: the workspace does not grow with B
constexpr u32 KG_NOT_UNIT = NTRU_FLAG_NOT_UNIT_MOD2 | NTRU_FLAG_NOT_UNIT_MODP;
constexpr u32 KG_MARK = 1;                    // parity mark of a waiting item (never set in a returned flags byte)
constexpr int KG_ATTEMPT_SHIFT = 44;          // stream position of attempt t of item i: (t << 44) + i
constexpr uint64_t KG_G_BASE = 1ull << 40;    // stream position of g of item i: 2^40 + i; every item index is below 2^40

// The items b < B whose flags say "not a unit" and whose mark equals `mark` -> list[0 .. min(count, cap)), count = how many there are
// (all of them, also past cap).  List order is whatever the atomics make it: every row's draw depends on its own index only.
// tries != NULL: tries[b] = 1 for every item (the first compaction of a call).
__global__ void k_keygen_compact(const uint8_t *__restrict__ flags, long B, u32 mark, u32 cap, u32 *__restrict__ list,
                                 u32 *__restrict__ count, uint8_t *__restrict__ tries) {
  const int lane = threadIdx.x & 63;
  const long stride = (long)gridDim.x * blockDim.x;
  for (long base = (long)blockIdx.x * blockDim.x + (threadIdx.x & ~63); base < B; base += stride) {    // wave-uniform
    const long b = base + lane;
    const bool valid = b < B;
    const u32 fl = valid ? flags[b] : 0u;
    if (tries && valid) tries[b] = 1;
    const bool waiting = (fl & KG_NOT_UNIT) && (fl & KG_MARK) == mark;
    const unsigned long long ballot = __ballot(waiting);
    if (!ballot) continue;
    const u32 below = lanes_below(ballot);
    u32 first = 0;
    if (lane == 0) first = atomicAdd(count, (u32)__popcll(ballot));
    first = __shfl(first, 0);
    if (waiting && first + below < cap) list[first + below] = (u32)b;
  }
}

// Compact rows k < n back to item list[k]: f, tries and flags always (flags | mark while the item still waits), fq / fp when the
// row is a unit.  One workgroup per row.
__global__ void k_keygen_scatter(int N, int n, const u32 *__restrict__ list, const int8_t *__restrict__ fc, const u16 *__restrict__ fqc,
                                 const uint8_t *__restrict__ fpc, const uint8_t *__restrict__ flc, u32 mark, u32 tries_val,
                                 int8_t *__restrict__ f, u16 *__restrict__ fq, uint8_t *__restrict__ fp, uint8_t *__restrict__ tries,
                                 uint8_t *__restrict__ flags) {
  for (int k = blockIdx.x; k < n; k += gridDim.x) {
    const size_t b = list[k];
    const u32 fl = flc[k];
    const size_t src = (size_t)k * N, dst = b * N;
    for (int c = threadIdx.x; c < N; c += blockDim.x) {
      f[dst + c] = fc[src + c];
      if (!fl) {
        fq[dst + c] = fqc[src + c];
        fp[dst + c] = fpc[src + c];
      }
    }
    if (threadIdx.x == 0) {
      if (tries) tries[b] = (uint8_t)tries_val;
      flags[b] = (uint8_t)(fl ? (fl | mark) : 0u);
    }
  }
}

// After the last pass: items that never drew a unit get zero fq / fp rows; every mark is cleared.  One wave per item.
__global__ void k_keygen_finalize(int N, long B, uint8_t *__restrict__ flags, u16 *__restrict__ fq, uint8_t *__restrict__ fp) {
  const int lane = threadIdx.x & 63;
  const long waves = (long)gridDim.x * (blockDim.x / 64);
  for (long b = (long)blockIdx.x * (blockDim.x / 64) + (threadIdx.x >> 6); b < B; b += waves) {
    const u32 fl = flags[b];
    if (!(fl & KG_NOT_UNIT)) continue;
    for (int c = lane; c < N; c += 64) {
      fq[(size_t)b * N + c] = 0;
      fp[(size_t)b * N + c] = 0;
    }
    if (lane == 0) flags[b] = (uint8_t)(fl & KG_NOT_UNIT);
  }
}

// ---- host side --------------------------------------------------------------------------------------------------------------------

// Workspace of one _dev call: the list and count of a pass and the compact rows of its sample / inversion.
struct Layout {
  int64_t rows;
  size_t list, count, f, fq, fp, fl, total;
};

Layout layout_of(int N, int64_t B) {
  Layout L;
  L.rows = std::max<int64_t>(1, std::min<int64_t>(B, KG_PASS_ROWS));
  const size_t r = (size_t)L.rows;
  Carve c;
  L.list = c.take(4 * r);
  L.count = c.take(256);
  L.f = c.take(r * N);
  L.fq = c.take(2 * r * N);
  L.fp = c.take(r * N);
  L.fl = c.take(r);
  L.total = c.total;
  return L;
}

// Every parameter is checked before the engine pointer, so that a host without a device still gets the parameter's message.
int check_args(ntru_engine *eng, int N, int q, int p, int df, int dg, const uint32_t *key, uint64_t first_item, int max_tries, int64_t B) {
  if (N < 2 || N > NTRU_MAX_N) return fail(NTRU_ERR_UNSUPPORTED, "key generation: need 2 <= N <= " + std::to_string(NTRU_MAX_N));
  if (q < 2 || q > 65536 || !is_pow2(q)) return fail(NTRU_ERR_UNSUPPORTED, "key generation: q must be a power of two, 2 <= q <= 65536");
  if (p != 3) return fail(NTRU_ERR_UNSUPPORTED, "key generation implements p = 3 (the key inversion's domain)");
  if ((long)p * (q - 1) >= 65536) return fail(NTRU_ERR_UNSUPPORTED, "key generation: p*(q-1) must fit 16 bits (the public key's domain)");
  if (df < 1 || 2 * df - 1 > N) return fail(NTRU_ERR_ARG, "key generation: need 1 <= df and 2 df - 1 <= N (f has df ones and df - 1 minus ones)");
  if (dg < 0 || 2 * dg > N) return fail(NTRU_ERR_ARG, "key generation: need 0 <= dg and 2 dg <= N (g has dg ones and dg minus ones)");
  if (max_tries < 1 || max_tries > 255) return fail(NTRU_ERR_ARG, "key generation: need 1 <= max_tries <= 255");
  if (!key) return fail(NTRU_ERR_ARG, "key generation: key is NULL");
  if (B < 0) return fail(NTRU_ERR_ARG, "negative batch size");
  if (first_item > KG_G_BASE || (uint64_t)B > KG_G_BASE - first_item)
    return fail(NTRU_ERR_ARG, "key generation: need first_item + B <= 2^40 (the stream positions of f and g must not meet)");
  if (!eng) return fail(NTRU_ERR_ARG, "engine is NULL");
  return NTRU_OK;
}

// The engine's sampler setting, restored on every way out: key material is always drawn with ChaCha20.
struct RoundsHold {
  ntru_engine *eng;
  int saved;
  explicit RoundsHold(ntru_engine *e) : eng(e), saved(e->sampler_rounds) { e->sampler_rounds = 20; }
  ~RoundsHold() { eng->sampler_rounds = saved; }
  RoundsHold(const RoundsHold &) = delete;
  RoundsHold &operator=(const RoundsHold &) = delete;
};

}  // namespace

extern "C" int ntru_keygen_workspace_bytes(int N, int64_t B, size_t *bytes) {
  if (N < 2 || N > NTRU_MAX_N) return fail(NTRU_ERR_ARG, "key generation: need 2 <= N <= " + std::to_string(NTRU_MAX_N));
  if (B < 0) return fail(NTRU_ERR_ARG, "negative batch size");
  if (!bytes) return fail(NTRU_ERR_ARG, "ntru_keygen_workspace_bytes: bytes is NULL");
  *bytes = layout_of(N, B).total;
  return NTRU_OK;
}

extern "C" int ntru_keygen_batch_dev(ntru_engine_t *eng, int N, int q, int p, int df, int dg, const uint32_t *key, uint64_t first_item,
                                     int max_tries, int64_t B, void *d_work, int8_t *d_f, int8_t *d_g, uint16_t *d_fq, uint8_t *d_fp,
                                     uint16_t *d_h, uint8_t *d_tries, uint8_t *d_flags) {
  if (int rc = check_args(eng, N, q, p, df, dg, key, first_item, max_tries, B)) return rc;
  if (B == 0) return NTRU_OK;
  if (!d_work || !d_f || !d_g || !d_fq || !d_fp || !d_h || !d_flags) return fail(NTRU_ERR_ARG, "ntru_keygen_batch: NULL buffer");
  HIP_TRY(hipSetDevice(eng->device));
  RoundsHold rounds(eng);
  const Layout L = layout_of(N, B);
  char *const w = (char *)d_work;
  u32 *const list = (u32 *)(w + L.list), *const count = (u32 *)(w + L.count);
  int8_t *const wf = (int8_t *)(w + L.f);
  uint16_t *const wfq = (uint16_t *)(w + L.fq);
  uint8_t *const wfp = (uint8_t *)(w + L.fp), *const wfl = (uint8_t *)(w + L.fl);

  if (int rc = ntru_sample_ternary_dev(eng, N, dg, dg, 255, key, KG_G_BASE + first_item, B, (uint8_t *)d_g)) return rc;
  if (int rc = ntru_sample_ternary_dev(eng, N, df, df - 1, 255, key, first_item, B, (uint8_t *)d_f)) return rc;
  if (int rc = ntru_invert_key_batch_dev(eng, N, q, p, d_f, B, d_fq, d_fp, d_flags)) return rc;

  // Items with the given mark that are not units yet: list + count on the device, the count read back (the one synchronisation).
  auto compact = [&](u32 mark, uint8_t *tries_init, int64_t *waiting) -> int {
    HIP_TRY(hipMemsetAsync(count, 0, 4, eng->stream));
    hipLaunchKernelGGL(k_keygen_compact, elementwise_grid(eng, B), dim3(256), 0, eng->stream, (const uint8_t *)d_flags, (long)B, mark,
                       (u32)L.rows, list, count, tries_init);
    HIP_TRY(hipGetLastError());
    u32 host = 0;
    HIP_TRY(hipMemcpyAsync(&host, count, 4, hipMemcpyDeviceToHost, eng->stream));
    HIP_TRY(hipStreamSynchronize(eng->stream));
    *waiting = host;
    return NTRU_OK;
  };
  int64_t waiting = 0;
  if (int rc = compact(0, d_tries, &waiting)) return rc;       // every mark is 0 after the first inversion
  const bool redrawn = waiting > 0;
  for (int t = 1; t < max_tries && waiting > 0; t++) {
    const u32 mark_in = (u32)(t - 1) & KG_MARK, mark_out = (u32)t & KG_MARK;
    for (;;) {                                                 // passes of at most L.rows items of attempt t
      const int n = (int)std::min<int64_t>(waiting, L.rows);
      if (int rc = ntru_launch_sample_listed(eng, N, df, df - 1, 255, key, ((uint64_t)t << KG_ATTEMPT_SHIFT) + first_item, list, n,
                                             (uint8_t *)wf))
        return rc;
      if (int rc = ntru_invert_key_batch_dev(eng, N, q, p, wf, n, wfq, wfp, wfl)) return rc;
      hipLaunchKernelGGL(k_keygen_scatter, dim3((unsigned)std::min(n, eng->cus * 8)), dim3(256), 0, eng->stream, N, n, (const u32 *)list,
                         (const int8_t *)wf, (const u16 *)wfq, (const uint8_t *)wfp, (const uint8_t *)wfl, mark_out, (u32)(t + 1), d_f,
                         (u16 *)d_fq, d_fp, d_tries, d_flags);
      HIP_TRY(hipGetLastError());
      if (waiting <= L.rows) break;
      if (int rc = compact(mark_in, nullptr, &waiting)) return rc;       // the rest of attempt t's items
      if (waiting == 0) break;
    }
    if (t + 1 < max_tries)
      if (int rc = compact(mark_out, nullptr, &waiting)) return rc;      // the items that failed attempt t
  }
  if (redrawn) {
    hipLaunchKernelGGL(k_keygen_finalize, elementwise_grid(eng, B * 64), dim3(256), 0, eng->stream, N, (long)B, d_flags, (u16 *)d_fq, d_fp);
    HIP_TRY(hipGetLastError());
  }
  if (int rc = ntru_public_key_batch_dev(eng, N, q, p, d_fq, d_g, B, d_h)) return rc;
  note_kernel(eng, "k_keygen");
  return NTRU_OK;
}

// ---- host-pointer form: the chunked pipeline of ntru_host.hip, the workspace engine-owned --------------------------------------------

extern "C" int ntru_keygen_batch(ntru_engine_t *eng, int N, int q, int p, int df, int dg, const uint32_t *key, uint64_t first_item,
                                 int max_tries, int64_t B, int8_t *f, int8_t *g, uint16_t *fq, uint8_t *fp, uint16_t *h, uint8_t *tries,
                                 uint8_t *flags, uint64_t *packed_h) {
  if (int rc = check_args(eng, N, q, p, df, dg, key, first_item, max_tries, B)) return rc;
  if (B == 0) return NTRU_OK;
  if (!flags) return fail(NTRU_ERR_ARG, "ntru_keygen_batch: flags is NULL");
  int bits = 0, per = 0, al = 0, os = 0;
  if (packed_h)
    if (int rc = ntru_pack_params(q - 1, N, &bits, &per, &al, &os)) return rc;
  const int64_t C = ntru_chunk_items(B);
  size_t wbytes = 0;
  if (int rc = ntru_keygen_workspace_bytes(N, C, &wbytes)) return rc;
  HIP_TRY(hipSetDevice(eng->device));
  if (int rc = ntru_grow_dev(&eng->keygen_work, wbytes)) return rc;
  Pipeline P(eng);
  const size_t n8 = (size_t)N, n16 = 2 * (size_t)N;
  auto out_or_tmp = [&](void *ptr, size_t row) { return ptr ? P.out(ptr, row) : P.tmp(row); };
  const int jf = out_or_tmp(f, n8), jg = out_or_tmp(g, n8), jq = out_or_tmp(fq, n16), jp = out_or_tmp(fp, n8), jh = out_or_tmp(h, n16);
  const int jt = tries ? P.out(tries, 1) : -1, jl = P.out(flags, 1);
  const int jk = packed_h ? P.out(packed_h, (size_t)os * 32) : -1;
  void *const work = eng->keygen_work.p;
  return P.run(B, C, [&](int64_t o, int64_t n, void **d) {
    if (int rc = ntru_keygen_batch_dev(eng, N, q, p, df, dg, key, first_item + (uint64_t)o, max_tries, n, work, (int8_t *)d[jf], (int8_t *)d[jg],
                                       (uint16_t *)d[jq], (uint8_t *)d[jp], (uint16_t *)d[jh], jt >= 0 ? (uint8_t *)d[jt] : nullptr,
                                       (uint8_t *)d[jl]))
      return rc;
    if (jk >= 0) return ntru_pack_batch_dev(eng, q - 1, N, (const uint16_t *)d[jh], n, (uint64_t *)d[jk]);
    return NTRU_OK;
  });
}
