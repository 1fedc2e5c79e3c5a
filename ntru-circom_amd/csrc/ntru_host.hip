// ntru_host.hip -- the host-pointer entry points of include/ntru_engine.h (the ones Node.js reaches through the addon): every regular
// one (a _dev form run chunk by chunk, with its ntru_multi_ form where it has one), ntru_pipeline_batch, plain device buffers and the
// multi-device engine.  No kernels here: tests/hostcheck builds this file and abi.hip for the CPU under the sanitizers.
//
// The reference keeps everything in JS arrays (index.js:87-197); a host binding therefore hands the engine HOST buffers.
// This file moves them through the GPU as a pipeline instead of "allocate, copy, run, copy, free" per call:
//   * a batch is cut into chunks; a chunk passes three stages -- upload, compute, download -- each on its own engine-owned stream,
//     chained by events: while chunk k computes, chunk k+1 is uploaded and chunk k-1 downloaded, one copy per direction at a time
//     (PCIe is full duplex), and the CPU-side staging copies of the next chunk overlap all three;
//   * chunk k owns buffer set k % 3 (pinned host arena, device arena, scratch: they only grow -- no hipMalloc / hipFree /
//     hipHostMalloc on the steady-state path) until its download is done;
//   * buffers the caller allocated with ntru_host_alloc (pinned; the addon exposes them as TypedArrays) are DMA'd in place;
//     ordinary pageable memory is staged through the set's pinned arena with a multi-threaded memcpy.
// Shared key rows (h, f, fp) travel with every chunk (<= 4N bytes), which keeps a single-item call at one H2D, one launch
// and one D2H with a single host synchronisation.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdint>
#include <cstring>
#include <string>
#include <thread>
#include <type_traits>
#include <vector>

#include "engine_internal.h"

// ---- the helpers of Pipeline (engine_internal.h)
bool ntru_is_pinned(const void *p) {
  hipPointerAttribute_t at;
  if (hipPointerGetAttributes(&at, p) != hipSuccess) { (void)hipGetLastError(); return false; }
  return at.type == hipMemoryTypeHost;
}

void ntru_big_memcpy(void *dst, const void *src, size_t bytes) {
  constexpr size_t PER_THREAD = (size_t)4 << 20;
  unsigned hw = std::thread::hardware_concurrency();
  size_t nt = std::min<size_t>(std::min<size_t>(hw ? hw : 1, 8), bytes / PER_THREAD);
  if (nt <= 1) { memcpy(dst, src, bytes); return; }
  std::vector<std::thread> th;
  const size_t part = ((bytes / nt) + 63) & ~(size_t)63;
  for (size_t t = 1; t < nt; t++) {
    const size_t o = t * part, n = o >= bytes ? 0 : std::min(part, bytes - o);
    if (n) th.emplace_back([=] { memcpy((char *)dst + o, (const char *)src + o, n); });
  }
  memcpy(dst, src, std::min(part, bytes));
  for (auto &t : th) t.join();
}

// Items per chunk: large enough that a kernel launch fills the chip, small enough that a batch has several chunks in
// flight (a chunk of 2^15 N=821 round trips is ~0.4 GB over PCIe, ~7 ms; its kernels take ~0.15 ms).
int64_t ntru_chunk_items(int64_t B) {
  const int64_t big = 1 << 15;
  if (B >= 4 * big) return big;
  if (B >= 4 * 2048) return (B + 3) / 4;
  return B;
}

extern "C" void *ntru_host_alloc(size_t bytes) {
  void *p = nullptr;
  if (hipHostMalloc(&p, bytes ? bytes : 1, hipHostMallocDefault) != hipSuccess) {
    ntru_fail(NTRU_ERR_HIP, "hipHostMalloc failed");
    return nullptr;
  }
  return p;
}

extern "C" void ntru_host_free(void *p) {
  if (p) (void)hipHostFree(p);
}

// ---- one description per call ---------------------------------------------------------------------------------------------------
// A regular host form is its own _dev form, run chunk by chunk through a Pipeline.  It states the _dev form's arguments once, in
// order, and describes each array where it passes it:
//   rows(p, len)       one row of len elements per item
//   shared(p, len)     one row that travels with every chunk (key material; inputs only)
//   optional(p, len)   rows per item that may be NULL
// The element type gives the bytes; a pointer to const is an input (uploaded), a pointer to non-const an output (downloaded).
// `items` stands where the _dev form takes the item count and first(v) where it takes the index of its first item: the two
// scalars that change per chunk (and per shard).  Every other argument is passed on as it is.
namespace {
enum Role { ROWS, SHARED, OPTIONAL };
template <class T>
struct Arr {
  T *p;
  size_t len;
  Role role;
  int slot;                  // its index in the Pipeline, once declared
};
template <class T> Arr<T> rows(T *p, size_t len) { return {p, len, ROWS, -1}; }
template <class T> Arr<const T> shared(const T *p, size_t len) { return {p, len, SHARED, -1}; }
template <class T> Arr<T> optional(T *p, size_t len) { return {p, len, OPTIONAL, -1}; }
struct Items {};
constexpr Items items;
struct First { uint64_t v; };
inline First first(uint64_t v) { return {v}; }

// An argument as the _dev form gets it for n items from item o on: arrays at their device addresses d (without d: NULL).
template <class T> T *dev_arg(const Arr<T> &a, int64_t, int64_t, void **d) { return d ? static_cast<T *>(d[a.slot]) : nullptr; }
inline int64_t dev_arg(Items, int64_t, int64_t n, void **) { return n; }
inline uint64_t dev_arg(First f, int64_t o, int64_t, void **) { return f.v + (uint64_t)o; }
template <class S> S dev_arg(S s, int64_t, int64_t, void **) { return s; }

template <class T> bool missing(const Arr<T> &a) { return a.role != OPTIONAL && !a.p; }
template <class S> bool missing(const S &) { return false; }

template <class T> void declare(Pipeline &P, Arr<T> &a) {
  if constexpr (std::is_const_v<T>) a.slot = P.in(a.p, a.len * sizeof(T), a.role == SHARED);
  else a.slot = P.out(a.p, a.len * sizeof(T));
}
template <class S> void declare(Pipeline &, S &) {}

// The host form of dev_form: its parameter checks (no arrays, no items; a negative B goes through as it is), nothing to do at B = 0,
// "<name>: NULL buffer" for a missing array, then the arrays through the Pipeline in argument order, one dev_form call per chunk.
template <class Fn, class... A>
int host_call(const char *name, ntru_engine_t *eng, int64_t B, Fn dev_form, A... a) {
  if (int rc = dev_form(eng, dev_arg(a, 0, B < 0 ? B : 0, nullptr)...)) return rc;
  if (B == 0) return NTRU_OK;
  if ((missing(a) || ...)) return ntru_fail(NTRU_ERR_ARG, std::string(name) + ": NULL buffer");
  Pipeline P(eng);
  (declare(P, a), ...);
  return P.run(B, ntru_chunk_items(B), [&](int64_t o, int64_t n, void **d) { return dev_form(eng, dev_arg(a, o, n, d)...); });
}
}  // namespace

// ---- several devices in ONE process: contiguous shards, one host thread + engine (with its three stage streams) per device ------
// item b depends only on (key, m[b], r[b]) / (key, e[b]) / key[b], so a host batch is cut into contiguous
// slices [g B / G, (g + 1) B / G) and every slice runs the single-device host form on its own thread; nothing is exchanged
// between devices.  (The benchmark's multi-GPU mode is one PROCESS per GPU instead -- bench.py under torchrun; this is for a
// host program, e.g. the Node.js addon, that owns all the GPUs of a node itself.)
struct ntru_multi {
  std::vector<ntru_engine_t *> eng;
};

extern "C" int ntru_multi_create(const int *device_ids, int n_dev, ntru_multi_t **out) {
  if (!out) return ntru_fail(NTRU_ERR_ARG, "ntru_multi_create: out is NULL");
  *out = nullptr;
  if (!device_ids || n_dev < 1 || n_dev > 64) return ntru_fail(NTRU_ERR_ARG, "ntru_multi_create: need 1 .. 64 device ids");
  ntru_multi *m = new ntru_multi;
  for (int i = 0; i < n_dev; i++) {
    ntru_engine_t *e = nullptr;
    if (int rc = ntru_engine_create(device_ids[i], &e)) {
      for (ntru_engine_t *x : m->eng) ntru_engine_destroy(x);
      delete m;
      return rc;
    }
    m->eng.push_back(e);
  }
  *out = m;
  return NTRU_OK;
}

extern "C" void ntru_multi_destroy(ntru_multi_t *m) {
  if (!m) return;
  for (ntru_engine_t *e : m->eng) ntru_engine_destroy(e);
  delete m;
}

extern "C" int ntru_multi_engines(const ntru_multi_t *m) { return m ? (int)m->eng.size() : 0; }

extern "C" int ntru_multi_set_lift(ntru_multi_t *m, int lift) {
  if (!m) return ntru_fail(NTRU_ERR_ARG, "multi-device engine is NULL");
  if (lift != NTRU_LIFT_REFERENCE && lift != NTRU_LIFT_CENTRED) return ntru_engine_set_lift(m->eng[0], lift);   // its message; nothing changed
  for (ntru_engine_t *e : m->eng) (void)ntru_engine_set_lift(e, lift);
  return NTRU_OK;
}

namespace {
// fn(engine, first item, items) on one thread per engine; the first failure (lowest shard) is what the caller sees
template <class F>
int for_each_shard(ntru_multi_t *m, int64_t B, F fn) {
  if (!m) return ntru_fail(NTRU_ERR_ARG, "multi-device engine is NULL");
  if (B < 0) return ntru_fail(NTRU_ERR_ARG, "negative batch size");
  const int G = (int)m->eng.size();
  std::vector<int> rc(G, NTRU_OK);
  std::vector<std::string> msg(G);
  std::vector<std::thread> th;
  auto shard = [&](int g) {
    const int64_t base = B / G, extra = B % G, lo = g * base + (g < extra ? g : extra), n = base + (g < extra ? 1 : 0);
    rc[g] = fn(m->eng[g], lo, n);
    if (rc[g]) msg[g] = ntru_last_error();               // the message is per thread: carry it over
  };
  for (int g = 1; g < G; g++) th.emplace_back(shard, g);
  shard(0);
  for (auto &t : th) t.join();
  for (int g = 0; g < G; g++)
    if (rc[g]) return ntru_fail(rc[g], "device shard " + std::to_string(g) + ": " + msg[g]);
  return NTRU_OK;
}

// The same argument list for the shard of n items from item lo on: rows per item move by lo rows, shared rows stay.
template <class T> Arr<T> shard_arg(Arr<T> a, int64_t lo) {
  if (a.p && a.role != SHARED) a.p += (size_t)lo * a.len;
  return a;
}
inline First shard_arg(First f, int64_t lo) { return {f.v + (uint64_t)lo}; }
template <class S> S shard_arg(S s, int64_t) { return s; }

// Where a form runs: on one engine, or in shards on the engines of a multi-device engine.  Either takes (name, _dev form, arguments),
// so a call that has both forms states its arguments once.
auto on_engine(ntru_engine_t *eng, int64_t B) {
  return [=](const char *name, auto dev_form, auto... a) { return host_call(name, eng, B, dev_form, a...); };
}
auto on_shards(ntru_multi_t *m, int64_t B) {
  return [=](const char *name, auto dev_form, auto... a) {
    return for_each_shard(m, B, [&](ntru_engine_t *eng, int64_t lo, int64_t n) { return host_call(name, eng, n, dev_form, shard_arg(a, lo)...); });
  };
}
template <class... P> bool any_null(const P *...p) { return (!p || ...); }
}  // namespace

// ---- the calls that have a multi-device form: arguments stated once, run on an engine or in shards ----------------------------------
template <class Run>
static int encrypt_form(Run run, int N, int q, const uint16_t *h, const uint8_t *r, const uint8_t *m, uint16_t *e, uint16_t *quotE) {
  return run("ntru_encrypt_batch", ntru_encrypt_batch_dev, N, q, shared(h, N), rows(r, N), rows(m, N), items, rows(e, N), optional(quotE, N));
}
extern "C" int ntru_encrypt_batch(ntru_engine_t *eng, int N, int q, const uint16_t *h, const uint8_t *r,
                                  const uint8_t *m, int64_t B, uint16_t *e, uint16_t *quotE) {
  return encrypt_form(on_engine(eng, B), N, q, h, r, m, e, quotE);
}
extern "C" int ntru_multi_encrypt_batch(ntru_multi_t *m, int N, int q, const uint16_t *h, const uint8_t *r, const uint8_t *mm,
                                        int64_t B, uint16_t *e, uint16_t *quotE) {
  return encrypt_form(on_shards(m, B), N, q, h, r, mm, e, quotE);
}

template <class Run>
static int decrypt_form(Run run, int N, int q, int p, const int8_t *f, const uint8_t *fp, const uint16_t *e, uint8_t *value, uint16_t *quot1,
                        uint16_t *rem1, uint8_t *quot2) {
  return run("ntru_decrypt_batch", ntru_decrypt_batch_dev, N, q, p, shared(f, N), shared(fp, N), rows(e, N), items, rows(value, N),
             optional(quot1, N), optional(rem1, N), optional(quot2, N));
}
extern "C" int ntru_decrypt_batch(ntru_engine_t *eng, int N, int q, int p, const int8_t *f, const uint8_t *fp,
                                  const uint16_t *e, int64_t B, uint8_t *value, uint16_t *quot1, uint16_t *rem1,
                                  uint8_t *quot2) {
  return decrypt_form(on_engine(eng, B), N, q, p, f, fp, e, value, quot1, rem1, quot2);
}
extern "C" int ntru_multi_decrypt_batch(ntru_multi_t *m, int N, int q, int p, const int8_t *f, const uint8_t *fp,
                                        const uint16_t *e, int64_t B, uint8_t *value, uint16_t *quot1, uint16_t *rem1,
                                        uint8_t *quot2) {
  return decrypt_form(on_shards(m, B), N, q, p, f, fp, e, value, quot1, rem1, quot2);
}

template <class Run>
static int polymul_split_form(Run run, int N, int mod, const uint16_t *a, const uint16_t *b, uint16_t *quot, uint16_t *rem) {
  return run("ntru_polymul_split", ntru_polymul_split_dev, N, mod, rows(a, N), rows(b, N), items, rows(quot, N), rows(rem, N));
}
extern "C" int ntru_polymul_split(ntru_engine_t *eng, int N, int mod, const uint16_t *a, const uint16_t *b,
                                  int64_t B, uint16_t *quot, uint16_t *rem) {
  return polymul_split_form(on_engine(eng, B), N, mod, a, b, quot, rem);
}
extern "C" int ntru_multi_polymul_split(ntru_multi_t *m, int N, int mod, const uint16_t *a, const uint16_t *b, int64_t B,
                                        uint16_t *quot, uint16_t *rem) {
  if (B > 0 && any_null(a, b, quot, rem)) return ntru_fail(NTRU_ERR_ARG, "ntru_multi_polymul_split: NULL buffer");
  return polymul_split_form(on_shards(m, B), N, mod, a, b, quot, rem);
}

template <class Run>
static int invert_key_form(Run run, int N, int q, int p, const int8_t *f, uint16_t *fq, uint8_t *fp, uint8_t *flags) {
  if (!fq && !fp) flags = nullptr;       // "fq or fp, at least one": with neither, the call lacks a buffer as if flags were missing
  return run("ntru_invert_key_batch", ntru_invert_key_batch_dev, N, q, p, rows(f, N), items, optional(fq, N), optional(fp, N), rows(flags, 1));
}
extern "C" int ntru_invert_key_batch(ntru_engine_t *eng, int N, int q, int p, const int8_t *f, int64_t B, uint16_t *fq,
                                     uint8_t *fp, uint8_t *flags) {
  return invert_key_form(on_engine(eng, B), N, q, p, f, fq, fp, flags);
}
extern "C" int ntru_multi_invert_key_batch(ntru_multi_t *m, int N, int q, int p, const int8_t *f, int64_t B, uint16_t *fq,
                                           uint8_t *fp, uint8_t *flags) {
  if (B > 0 && any_null(f, flags)) return ntru_fail(NTRU_ERR_ARG, "ntru_multi_invert_key_batch: NULL buffer");
  return invert_key_form(on_shards(m, B), N, q, p, f, fq, fp, flags);
}

template <class Run>
static int public_key_form(Run run, int N, int q, int p, const uint16_t *fq, const int8_t *g, uint16_t *h) {
  return run("ntru_public_key_batch", ntru_public_key_batch_dev, N, q, p, rows(fq, N), rows(g, N), items, rows(h, N));
}
extern "C" int ntru_public_key_batch(ntru_engine_t *eng, int N, int q, int p, const uint16_t *fq, const int8_t *g,
                                     int64_t B, uint16_t *h) {
  return public_key_form(on_engine(eng, B), N, q, p, fq, g, h);
}
extern "C" int ntru_multi_public_key_batch(ntru_multi_t *m, int N, int q, int p, const uint16_t *fq, const int8_t *g, int64_t B,
                                           uint16_t *h) {
  if (B > 0 && any_null(fq, g, h)) return ntru_fail(NTRU_ERR_ARG, "ntru_multi_public_key_batch: NULL buffer");
  return public_key_form(on_shards(m, B), N, q, p, fq, g, h);
}

template <class Run>
static int verify_keys_form(Run run, int N, int q, int p, const int8_t *f, const int8_t *g, const uint16_t *fq, const uint8_t *fp,
                            const uint16_t *h, uint16_t *quot_fq, uint16_t *rem_fq, uint8_t *quot_fp, uint8_t *rem_fp, uint16_t *quot_h,
                            uint16_t *rem_h, uint8_t *flags) {
  return run("ntru_verify_keys_batch", ntru_verify_keys_batch_dev, N, q, p, rows(f, N), rows(g, N), rows(fq, N), rows(fp, N), rows(h, N), items,
             rows(quot_fq, N), rows(rem_fq, N), rows(quot_fp, N), rows(rem_fp, N), rows(quot_h, N), rows(rem_h, N), rows(flags, 1));
}
extern "C" int ntru_verify_keys_batch(ntru_engine_t *eng, int N, int q, int p, const int8_t *f, const int8_t *g,
                                      const uint16_t *fq, const uint8_t *fp, const uint16_t *h, int64_t B,
                                      uint16_t *quot_fq, uint16_t *rem_fq, uint8_t *quot_fp, uint8_t *rem_fp,
                                      uint16_t *quot_h, uint16_t *rem_h, uint8_t *flags) {
  return verify_keys_form(on_engine(eng, B), N, q, p, f, g, fq, fp, h, quot_fq, rem_fq, quot_fp, rem_fp, quot_h, rem_h, flags);
}
extern "C" int ntru_multi_verify_keys_batch(ntru_multi_t *m, int N, int q, int p, const int8_t *f, const int8_t *g,
                                            const uint16_t *fq, const uint8_t *fp, const uint16_t *h, int64_t B,
                                            uint16_t *quot_fq, uint16_t *rem_fq, uint8_t *quot_fp, uint8_t *rem_fp,
                                            uint16_t *quot_h, uint16_t *rem_h, uint8_t *flags) {
  if (B > 0 && any_null(f, g, fq, fp, h, quot_fq, rem_fq, quot_fp, rem_fp, quot_h, rem_h, flags))
    return ntru_fail(NTRU_ERR_ARG, "ntru_multi_verify_keys_batch: NULL buffer");
  return verify_keys_form(on_shards(m, B), N, q, p, f, g, fq, fp, h, quot_fq, rem_fq, quot_fp, rem_fp, quot_h, rem_h, flags);
}

// ---- the other regular calls -------------------------------------------------------------------------------------------------------
extern "C" int ntru_split_by_I(ntru_engine_t *eng, int N, int mod, const uint16_t *a, int64_t B, uint16_t *quot,
                               uint16_t *rem) {
  return host_call("ntru_split_by_I", eng, B, ntru_split_by_I_dev, N, mod, rows(a, 2 * (size_t)N), items, rows(quot, N), rows(rem, N));
}

extern "C" int ntru_add_batch(ntru_engine_t *eng, int N, int mod, const uint16_t *a, const uint16_t *b, int64_t B,
                              uint16_t *out) {
  return host_call("ntru_add_batch", eng, B, ntru_add_batch_dev, N, mod, rows(a, N), rows(b, N), items, rows(out, N));
}

extern "C" int ntru_sample_ternary(ntru_engine_t *eng, int N, int n1, int n2, int other, const uint32_t *key,
                                   uint64_t first_item, int64_t B, uint8_t *out) {
  if (eng && B > 0 && !out) return ntru_fail(NTRU_ERR_ARG, "ntru_sample_ternary: NULL buffer");   // ahead of the parameter checks here
  return host_call("ntru_sample_ternary", eng, B, ntru_sample_ternary_dev, N, n1, n2, other, key, first(first_item), items, rows(out, N));
}

extern "C" int ntru_pack_batch(ntru_engine_t *eng, int max_val, int data_len, const uint16_t *data, int64_t B,
                               uint64_t *out) {
  if (!eng) return ntru_fail(NTRU_ERR_ARG, "engine is NULL");
  int bits, per, al, os;
  if (int rc = ntru_pack_params(max_val, data_len, &bits, &per, &al, &os)) return rc;                // ahead of the batch size here
  if (B > 0 && !data && data_len) return ntru_fail(NTRU_ERR_ARG, "ntru_pack_batch: NULL buffer");   // rows of no elements need no array
  return host_call("ntru_pack_batch", eng, B, ntru_pack_batch_dev, max_val, data_len, optional(data_len ? data : nullptr, data_len), items,
                   rows(out, (size_t)os * 4));
}

extern "C" int ntru_unpack_batch(ntru_engine_t *eng, int max_val, int packed_bits, const uint64_t *in, int packed_size,
                                 int64_t B, uint16_t *out) {
  if (int rc = ntru_unpack_batch_dev(eng, max_val, packed_bits, nullptr, packed_size, 0, nullptr)) return rc;   // ahead of the batch size here
  if (B < 0) return ntru_fail(NTRU_ERR_ARG, "negative batch size");
  if (packed_size == 0) return NTRU_OK;
  int bits = 0;
  while ((max_val >> bits) != 0) bits++;
  const size_t per = packed_bits / bits;
  return host_call("ntru_unpack_batch", eng, B, ntru_unpack_batch_dev, max_val, packed_bits, rows(in, (size_t)packed_size * 4), packed_size, items,
                   rows(out, (size_t)packed_size * per));
}

// per-item keys (matrix_peritem_scheme.hip)
extern "C" int ntru_encrypt_peritem_batch(ntru_engine_t *eng, int N, int q, const uint16_t *h, const uint8_t *r, const uint8_t *m,
                                          int64_t B, uint16_t *e, uint16_t *quotE) {
  return host_call("ntru_encrypt_peritem_batch", eng, B, ntru_encrypt_peritem_batch_dev, N, q, rows(h, N), rows(r, N), rows(m, N), items,
                   rows(e, N), optional(quotE, N));
}

extern "C" int ntru_decrypt_peritem_batch(ntru_engine_t *eng, int N, int q, int p, const int8_t *f, const uint8_t *fp, const uint16_t *e,
                                          int64_t B, uint8_t *value, uint16_t *quot1, uint16_t *rem1, uint8_t *quot2) {
  return host_call("ntru_decrypt_peritem_batch", eng, B, ntru_decrypt_peritem_batch_dev, N, q, p, rows(f, N), rows(fp, N), rows(e, N), items,
                   rows(value, N), optional(quot1, N), optional(rem1, N), optional(quot2, N));
}

// byte messages (message_bytes.hip)
extern "C" int ntru_bytes_to_rows(ntru_engine_t *eng, int N, int nbytes, const uint8_t *bytes, int64_t B, uint8_t *m) {
  return host_call("ntru_bytes_to_rows", eng, B, ntru_bytes_to_rows_dev, N, nbytes, rows(bytes, nbytes), items, rows(m, N));
}

extern "C" int ntru_rows_to_bytes(ntru_engine_t *eng, int N, int nbytes, const uint8_t *value, int64_t B, uint8_t *bytes, uint8_t *flags) {
  return host_call("ntru_rows_to_bytes", eng, B, ntru_rows_to_bytes_dev, N, nbytes, rows(value, N), items, rows(bytes, nbytes), optional(flags, 1));
}

extern "C" int ntru_encrypt_bytes_batch(ntru_engine_t *eng, int N, int q, int nbytes, const uint16_t *h, const uint8_t *r,
                                        const uint8_t *bytes, int64_t B, uint16_t *e, uint16_t *quotE) {
  return host_call("ntru_encrypt_bytes_batch", eng, B, ntru_encrypt_bytes_batch_dev, N, q, nbytes, shared(h, N), rows(r, N), rows(bytes, nbytes),
                   items, rows(e, N), optional(quotE, N));
}

extern "C" int ntru_decrypt_bytes_batch(ntru_engine_t *eng, int N, int q, int p, int nbytes, const int8_t *f, const uint8_t *fp,
                                        const uint16_t *e, int64_t B, uint8_t *bytes, uint8_t *flags) {
  return host_call("ntru_decrypt_bytes_batch", eng, B, ntru_decrypt_bytes_batch_dev, N, q, p, nbytes, shared(f, N), shared(fp, N), rows(e, N),
                   items, rows(bytes, nbytes), optional(flags, 1));
}

// witness checks (witness_check.hip): their batch-size message comes ahead of the parameter checks
extern "C" int ntru_check_encrypt_batch(ntru_engine_t *eng, int N, int q, int nq, const uint16_t *r, const uint16_t *m,
                                        const uint16_t *h, const uint16_t *quotE, const uint16_t *remE, int64_t B, uint8_t *flags) {
  if (B < 0) return ntru_fail(NTRU_ERR_ARG, "witness check: negative batch size");
  return host_call("ntru_check_encrypt_batch", eng, B, ntru_check_encrypt_batch_dev, N, q, nq, rows(r, N), rows(m, N), rows(h, N),
                   rows(quotE, (size_t)N + 1), rows(remE, (size_t)N + 1), items, rows(flags, 1));
}

extern "C" int ntru_check_decrypt_batch(ntru_engine_t *eng, int N, int q, int nq, int p, int np, const uint16_t *f, const uint16_t *fp,
                                        const uint16_t *e, const uint16_t *quot1, const uint16_t *rem1, const uint16_t *quot2,
                                        const uint16_t *rem2, int64_t B, uint8_t *flags) {
  if (B < 0) return ntru_fail(NTRU_ERR_ARG, "witness check: negative batch size");
  return host_call("ntru_check_decrypt_batch", eng, B, ntru_check_decrypt_batch_dev, N, q, nq, p, np, rows(f, N), rows(fp, N), rows(e, N),
                   rows(quot1, (size_t)N + 1), rows(rem1, (size_t)N + 1), rows(quot2, (size_t)N + 1), rows(rem2, (size_t)N + 1), items,
                   rows(flags, 1));
}

extern "C" int ntru_check_inverse_batch(ntru_engine_t *eng, int N, int M, int n, const uint16_t *f, const uint16_t *fq,
                                        const uint16_t *quotI, const uint16_t *remI, int64_t B, uint8_t *flags) {
  if (B < 0) return ntru_fail(NTRU_ERR_ARG, "witness check: negative batch size");
  return host_call("ntru_check_inverse_batch", eng, B, ntru_check_inverse_batch_dev, N, M, n, rows(f, N), rows(fq, N), rows(quotI, (size_t)N + 1),
                   rows(remI, (size_t)N + 1), items, rows(flags, 1));
}

// ---- device-resident stages for a caller without HIP of its own (Node.js) -------------------------------------------------------
// ntru_pipeline_batch: sampler -> encryptBits -> decryptBits -> packOutput per chunk, the intermediates (r, e, value) staying in the
// slot's device arena; only m (and r when the caller supplies it) crosses PCIe upwards and only the outputs asked for come back
// (index.js:461-488, :87-140, :572-620 chained).  The chunks flow through the same three-stage pipeline (upload / compute / download
// streams, three buffer sets) as every host-pointer entry point, so the upload of chunk k+1 and the download of chunk k-1 overlap
// the kernels of chunk k.
extern "C" int ntru_pipeline_batch(ntru_engine_t *eng, int N, int q, int p, const uint16_t *h, const int8_t *f, const uint8_t *fp,
                                   const uint32_t *key, uint64_t first_item, int n1, int n2, const uint8_t *r, const uint8_t *m,
                                   int64_t B, uint8_t *r_out, uint16_t *e, uint8_t *value, uint64_t *packed) {
  if (!eng) return ntru_fail(NTRU_ERR_ARG, "engine is NULL");
  if (B < 0) return ntru_fail(NTRU_ERR_ARG, "negative batch size");
  const bool decrypt = f != nullptr || fp != nullptr;
  if (decrypt && (!f || !fp)) return ntru_fail(NTRU_ERR_ARG, "ntru_pipeline_batch: the decrypt stage needs both f and fp");
  if (!decrypt && value) return ntru_fail(NTRU_ERR_ARG, "ntru_pipeline_batch: `value` needs the decrypt stage (f, fp)");
  if ((key != nullptr) == (r != nullptr)) return ntru_fail(NTRU_ERR_ARG, "ntru_pipeline_batch: give either a sampler key or r");
  if (!e && !value && !packed && !(r_out && key)) return ntru_fail(NTRU_ERR_ARG, "ntru_pipeline_batch: no output asked for");
  // parameter checks of every stage (B = 0 calls return after them)
  if (int rc = ntru_encrypt_batch_dev(eng, N, q, nullptr, nullptr, nullptr, 0, nullptr, nullptr)) return rc;
  if (decrypt) if (int rc = ntru_decrypt_batch_dev(eng, N, q, p, nullptr, nullptr, nullptr, 0, nullptr, nullptr, nullptr, nullptr)) return rc;
  if (key) if (int rc = ntru_sample_ternary_dev(eng, N, n1, n2, p - 1, key, first_item, 0, nullptr)) return rc;
  int bits = 0, per = 0, al = 0, os = 0;
  const int pack_max = decrypt ? p - 1 : q - 1;                    // packOutput of the last stage's result
  if (packed) if (int rc = ntru_pack_params(pack_max, N, &bits, &per, &al, &os)) return rc;
  if (B == 0) return NTRU_OK;
  if (!h || !m) return ntru_fail(NTRU_ERR_ARG, "ntru_pipeline_batch: NULL buffer");
  Pipeline P(eng);
  const int ih = P.in(h, (size_t)N * 2, true), im = P.in(m, N);
  const int jf = decrypt ? P.in(f, N, true) : -1, jfp = decrypt ? P.in(fp, N, true) : -1;
  const int ir = r ? P.in(r, N) : (r_out ? P.out(r_out, N) : P.tmp(N));
  const int ie = e ? P.out(e, (size_t)N * 2) : P.tmp((size_t)N * 2);
  const int iv = !decrypt ? -1 : (value ? P.out(value, N) : P.tmp(N));
  const int ip = packed ? P.out(packed, (size_t)os * 32) : -1;
  return P.run(B, ntru_chunk_items(B), [&](int64_t o, int64_t n, void **d) {
    if (key) if (int rc = ntru_sample_ternary_dev(eng, N, n1, n2, p - 1, key, first_item + (uint64_t)o, n, (uint8_t *)d[ir])) return rc;
    if (!decrypt && packed) {   // packOutput of e: out of the encrypt kernel itself when e is not an output too and the row-image kernel applies
      if (!e) {                                            // the launcher itself says whether the fused kernel applies (NTRU_NOT_TAKEN:
        const int rc = ntru_launch_encrypt_pack_rowimage(eng, N, q, (const uint16_t *)d[ih], (const uint8_t *)d[ir], (const uint8_t *)d[im], n,
                                                         (uint64_t *)d[ip], os);     // e as the intermediate, below); no public error
        if (rc != NTRU_NOT_TAKEN) return rc;               // code doubles as control flow
      }
      return ntru_encrypt_pack_batch_dev(eng, N, q, (const uint16_t *)d[ih], (const uint8_t *)d[ir], (const uint8_t *)d[im], n,
                                         (uint16_t *)d[ie], (uint64_t *)d[ip]);
    }
    if (int rc = ntru_encrypt_batch_dev(eng, N, q, (const uint16_t *)d[ih], (const uint8_t *)d[ir], (const uint8_t *)d[im], n,
                                        (uint16_t *)d[ie], nullptr)) return rc;
    if (decrypt && packed)      // packOutput fused into the decrypt kernel's second epilogue where the matrix path applies (no k_pack launch)
      return ntru_decrypt_pack_batch_dev(eng, N, q, p, (const int8_t *)d[jf], (const uint8_t *)d[jfp], (const uint16_t *)d[ie], n,
                                         (uint8_t *)d[iv], (uint64_t *)d[ip]);
    if (decrypt)
      return ntru_decrypt_batch_dev(eng, N, q, p, (const int8_t *)d[jf], (const uint8_t *)d[jfp], (const uint16_t *)d[ie], n,
                                    (uint8_t *)d[iv], nullptr, nullptr, nullptr);
    return NTRU_OK;
  });
}

// Plain device buffers on the engine's device, with copies ordered on the engine's stream: what a binding needs to keep arrays
// on the GPU between *_dev calls (the addon hands them to JavaScript as opaque handles).
extern "C" int ntru_dev_alloc(ntru_engine_t *eng, size_t bytes, void **d_ptr) {
  if (!eng || !d_ptr) return ntru_fail(NTRU_ERR_ARG, "ntru_dev_alloc: NULL argument");
  *d_ptr = nullptr;
  HIP_TRY(hipSetDevice(eng->device));
  if (hipMalloc(d_ptr, bytes ? bytes : 1) != hipSuccess) { *d_ptr = nullptr; return ntru_fail(NTRU_ERR_HIP, "hipMalloc failed"); }
  return NTRU_OK;
}

extern "C" int ntru_dev_free(ntru_engine_t *eng, void *d_ptr) {
  if (!eng) return ntru_fail(NTRU_ERR_ARG, "engine is NULL");
  if (!d_ptr) return NTRU_OK;
  HIP_TRY(hipSetDevice(eng->device));
  HIP_TRY(hipFree(d_ptr));                  // waits for the device: nothing in flight still uses the buffer
  return NTRU_OK;
}

// Returns when `src` may be reused (pageable memory is copied before the call returns, pinned memory once the DMA is done); the data
// is in place for every later call on the engine's stream.
extern "C" int ntru_dev_upload(ntru_engine_t *eng, void *d_dst, const void *src, size_t bytes) {
  if (!eng || (bytes && (!d_dst || !src))) return ntru_fail(NTRU_ERR_ARG, "ntru_dev_upload: NULL argument");
  if (!bytes) return NTRU_OK;
  HIP_TRY(hipSetDevice(eng->device));
  HIP_TRY(hipMemcpyAsync(d_dst, src, bytes, hipMemcpyHostToDevice, eng->stream));
  HIP_TRY(hipStreamSynchronize(eng->stream));
  return NTRU_OK;
}

// Waits for everything enqueued on the engine's stream, then returns with the bytes in `dst`.
extern "C" int ntru_dev_download(ntru_engine_t *eng, void *dst, const void *d_src, size_t bytes) {
  if (!eng || (bytes && (!dst || !d_src))) return ntru_fail(NTRU_ERR_ARG, "ntru_dev_download: NULL argument");
  HIP_TRY(hipSetDevice(eng->device));
  if (bytes) HIP_TRY(hipMemcpyAsync(dst, d_src, bytes, hipMemcpyDeviceToHost, eng->stream));
  HIP_TRY(hipStreamSynchronize(eng->stream));
  return NTRU_OK;
}
