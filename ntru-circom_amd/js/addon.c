/*
 * addon.c -- N-API binding of include/ntru_engine.h for Node.js (N-API version 6: BigInt64Array / BigUint64Array; Node 12.17+).
 *
 * Thin by design: every exported function unpacks TypedArray arguments into the plain pointers the C ABI takes
 * (napi_get_typedarray_info), calls the engine, and throws a JS Error carrying ntru_last_error() on failure.
 * All reference-shaped behaviour (padding, trimming, {value, inputs, params} objects) lives in index.mjs.
 * The batch calls are rows of one table (ops[], below the few calls written by hand); engine and handle management, the pack calls
 * (their sizes come from ntru_pack_params, whose refusal is an engine error before any buffer is looked at) and genericOp are by hand.
 */
#define NAPI_VERSION 6
#include <node_api.h>
#include <pthread.h>
#include <stddef.h>
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "ntru_engine.h"

#define NAPI_OK(call)                                                              \
  do {                                                                             \
    if ((call) != napi_ok) {                                                       \
      napi_throw_error(env, NULL, "N-API call failed: " #call);                    \
      return NULL;                                                                 \
    }                                                                              \
  } while (0)

static ntru_engine_t *g_engine = NULL;
static ntru_multi_t *g_multi = NULL;     /* useDevices([...]): the batch entry points shard over these devices instead */
/* One engine, one caller at a time: the *Async entry points run on libuv worker threads, everything else on the JS thread. */
static pthread_mutex_t g_lock = PTHREAD_MUTEX_INITIALIZER;
#define ENGINE_CALL(rc, expr) do { pthread_mutex_lock(&g_lock); (rc) = (expr); pthread_mutex_unlock(&g_lock); } while (0)

static napi_value throw_engine(napi_env env, int rc) {
  char buf[512];
  snprintf(buf, sizeof buf, "ntru engine error %d: %s", rc, ntru_last_error());
  napi_throw_error(env, NULL, buf);
  return NULL;
}

static int get_i32(napi_env env, napi_value v, int32_t *out) { return napi_get_value_int32(env, v, out) == napi_ok; }

/* Returns the data pointer of a TypedArray of the wanted element type holding at least `need` elements;
 * null/undefined gives NULL when `optional`. */
static int get_buf(napi_env env, napi_value v, napi_typedarray_type want, size_t need, int optional, void **out) {
  napi_valuetype vt;
  *out = NULL;
  if (napi_typeof(env, v, &vt) != napi_ok) return 0;
  if (vt == napi_null || vt == napi_undefined) return optional;
  bool is_ta = false;
  if (napi_is_typedarray(env, v, &is_ta) != napi_ok || !is_ta) return 0;
  napi_typedarray_type t; size_t len; void *data;
  if (napi_get_typedarray_info(env, v, &t, &len, &data, NULL, NULL) != napi_ok) return 0;
  if (t != want || len < need) return 0;
  *out = data;
  return 1;
}

#define ARGS(n)                                                                    \
  size_t argc = (n);                                                               \
  napi_value argv[(n)];                                                            \
  NAPI_OK(napi_get_cb_info(env, info, &argc, argv, NULL, NULL));                   \
  if (argc < (n)) { napi_throw_type_error(env, NULL, "too few arguments"); return NULL; }

#define BAD_ARGS() do { napi_throw_type_error(env, NULL, "bad argument types / sizes"); return NULL; } while (0)

static napi_value undefined(napi_env env) { napi_value u; napi_get_undefined(env, &u); return u; }

static int ensure_engine(napi_env env) {
  if (g_engine) return 1;
  napi_throw_error(env, NULL, "ntru engine not created: call create(device) first (there is no CPU fallback)");
  return 0;
}

static napi_value DeviceCount(napi_env env, napi_callback_info info) {
  (void)info;
  napi_value r; NAPI_OK(napi_create_int32(env, ntru_engine_device_count(), &r)); return r;
}

static napi_value Create(napi_env env, napi_callback_info info) {
  ARGS(1)
  int32_t dev;
  if (!get_i32(env, argv[0], &dev)) BAD_ARGS();
  pthread_mutex_lock(&g_lock);
  if (g_engine) { ntru_engine_destroy(g_engine); g_engine = NULL; }
  int rc = ntru_engine_create(dev, &g_engine);
  pthread_mutex_unlock(&g_lock);
  if (rc) return throw_engine(env, rc);
  return undefined(env);
}

static napi_value Destroy(napi_env env, napi_callback_info info) {
  (void)info;
  pthread_mutex_lock(&g_lock);
  if (g_engine) { ntru_engine_destroy(g_engine); g_engine = NULL; }
  if (g_multi) { ntru_multi_destroy(g_multi); g_multi = NULL; }
  pthread_mutex_unlock(&g_lock);
  return undefined(env);
}

/* useDevices(ids:Int32Array) -> number of engines.  An empty array goes back to the single engine of create(). */
static napi_value UseDevices(napi_env env, napi_callback_info info) {
  ARGS(1)
  bool is_ta = false;
  if (napi_is_typedarray(env, argv[0], &is_ta) != napi_ok || !is_ta) BAD_ARGS();
  napi_typedarray_type t; size_t len; void *data;
  NAPI_OK(napi_get_typedarray_info(env, argv[0], &t, &len, &data, NULL, NULL));
  if (t != napi_int32_array || len > 64) BAD_ARGS();
  pthread_mutex_lock(&g_lock);
  if (g_multi) { ntru_multi_destroy(g_multi); g_multi = NULL; }
  int rc = len ? ntru_multi_create((const int *)data, (int)len, &g_multi) : 0;
  pthread_mutex_unlock(&g_lock);
  if (rc) return throw_engine(env, rc);
  napi_value r; NAPI_OK(napi_create_int32(env, ntru_multi_engines(g_multi), &r)); return r;
}

static napi_value Supports(napi_env env, napi_callback_info info) {
  ARGS(2)
  int32_t N, mod;
  if (!get_i32(env, argv[0], &N) || !get_i32(env, argv[1], &mod)) BAD_ARGS();
  napi_value r; NAPI_OK(napi_get_boolean(env, ntru_engine_supports(N, mod) != 0, &r)); return r;
}

/* setSamplerRounds(rounds) -> rounds in force: 20 (ChaCha20, RFC 8439: the default), 12 or 8 for the draw stream of sampleTernary /
 * sampleTernaryDev / pipelineBatch (ntru_engine_set_sampler_rounds); setSamplerRounds(0) only reads the setting. */
static napi_value SetSamplerRounds(napi_env env, napi_callback_info info) {
  ARGS(1)
  int32_t rounds;
  if (!get_i32(env, argv[0], &rounds)) BAD_ARGS();
  if (!ensure_engine(env)) return NULL;
  pthread_mutex_lock(&g_lock);                       /* an Async pipeline job on a worker thread reads the setting */
  const int rc = rounds != 0 ? ntru_engine_set_sampler_rounds(g_engine, rounds) : 0;
  const int now = ntru_engine_get_sampler_rounds(g_engine);
  pthread_mutex_unlock(&g_lock);
  if (rc) return throw_engine(env, rc);
  napi_value r; NAPI_OK(napi_create_int32(env, now, &r)); return r;
}


/* packParams(maxVal, dataLen) -> [bits, perOutput, arrLen, outputSize] */
static napi_value PackParams(napi_env env, napi_callback_info info) {
  ARGS(2)
  int32_t mv, dl; int v[4];
  if (!get_i32(env, argv[0], &mv) || !get_i32(env, argv[1], &dl)) BAD_ARGS();
  int rc;
  ENGINE_CALL(rc, ntru_pack_params(mv, dl, &v[0], &v[1], &v[2], &v[3]));
  if (rc) return throw_engine(env, rc);
  napi_value arr; NAPI_OK(napi_create_array_with_length(env, 4, &arr));
  for (int i = 0; i < 4; i++) { napi_value n; NAPI_OK(napi_create_int32(env, v[i], &n)); NAPI_OK(napi_set_element(env, arr, i, n)); }
  return arr;
}

/* packBatch(maxVal, dataLen, data:Uint16Array[B*dataLen], B, out:BigUint64Array[B*outputSize*4]) */
static napi_value PackBatch(napi_env env, napi_callback_info info) {
  ARGS(5)
  int32_t mv, dl, B; void *data, *out; int v[4];
  if (!get_i32(env, argv[0], &mv) || !get_i32(env, argv[1], &dl) || !get_i32(env, argv[3], &B) || B < 0) BAD_ARGS();
  int rc;
  ENGINE_CALL(rc, ntru_pack_params(mv, dl, &v[0], &v[1], &v[2], &v[3]));
  if (rc) return throw_engine(env, rc);
  if (!get_buf(env, argv[2], napi_uint16_array, (size_t)dl * (size_t)B, 0, &data) ||
      !get_buf(env, argv[4], napi_biguint64_array, (size_t)v[3] * 4 * (size_t)B, 0, &out)) BAD_ARGS();
  if (!ensure_engine(env)) return NULL;
  ENGINE_CALL(rc, ntru_pack_batch(g_engine, mv, dl, data, B, out));
  return rc ? throw_engine(env, rc) : undefined(env);
}

/* unpackBatch(maxVal, packedBits, in:BigUint64Array[B*packedSize*4], packedSize, B, out:Uint16Array[B*packedSize*per]) */
static napi_value UnpackBatch(napi_env env, napi_callback_info info) {
  ARGS(6)
  int32_t mv, pb, ps, B; void *in, *out; int v[4];
  if (!get_i32(env, argv[0], &mv) || !get_i32(env, argv[1], &pb) || !get_i32(env, argv[3], &ps) ||
      !get_i32(env, argv[4], &B) || B < 0 || ps < 0) BAD_ARGS();
  int rc;
  ENGINE_CALL(rc, ntru_pack_params(mv, 0, &v[0], &v[1], &v[2], &v[3]));
  if (rc) return throw_engine(env, rc);
  const int per = pb / v[0];
  if (!get_buf(env, argv[2], napi_biguint64_array, (size_t)ps * 4 * (size_t)B, 0, &in) ||
      !get_buf(env, argv[5], napi_uint16_array, (size_t)ps * (size_t)(per > 0 ? per : 0) * (size_t)B, 0, &out)) BAD_ARGS();
  if (!ensure_engine(env)) return NULL;
  ENGINE_CALL(rc, ntru_unpack_batch(g_engine, mv, pb, in, ps, B, out));
  return rc ? throw_engine(env, rc) : undefined(env);
}

/* allocPinned(bytes) -> ArrayBuffer over page-locked memory (ntru_host_alloc): TypedArrays built on it are DMA'd in place
 * by the batch entry points instead of being staged.  Released when the ArrayBuffer is garbage collected. */
static void free_pinned(napi_env env, void *data, void *hint) { (void)env; (void)hint; ntru_host_free(data); }

static napi_value AllocPinned(napi_env env, napi_callback_info info) {
  ARGS(1)
  double bytes;
  if (napi_get_value_double(env, argv[0], &bytes) != napi_ok || bytes < 0 || bytes > 1e12) BAD_ARGS();
  if (!ensure_engine(env)) return NULL;
  void *p = ntru_host_alloc((size_t)bytes);
  if (!p) return throw_engine(env, NTRU_ERR_HIP);
  napi_value ab;
  if (napi_create_external_arraybuffer(env, p, (size_t)bytes, free_pinned, NULL, &ab) != napi_ok) {
    ntru_host_free(p);
    napi_throw_error(env, NULL, "napi_create_external_arraybuffer failed");
    return NULL;
  }
  return ab;
}

/* genericOp(op, a:Float64Array, b:Float64Array, mod, out0:Float64Array, out1:Float64Array|null) -> [status, len0, len1]
 * op: 0 multiplyPolynomials, 1 dividePolynomials, 2 extendedEuclideanAlgorithm, 3 polyInv (one item; the generic family of
 * include/ntru_engine.h).  JS Numbers cross as doubles and are converted to the int64 the C ABI takes; out0 / out1 need
 * ntru_generic_capacity(a.length, b.length) elements (genericCapacity). */
static napi_value GenericCapacity(napi_env env, napi_callback_info info) {
  ARGS(2)
  int32_t la, lb;
  if (!get_i32(env, argv[0], &la) || !get_i32(env, argv[1], &lb)) BAD_ARGS();
  napi_value r; NAPI_OK(napi_create_int32(env, ntru_generic_capacity(la, lb), &r)); return r;
}

static napi_value GenericOp(napi_env env, napi_callback_info info) {
  ARGS(6)
  int32_t op; double mod; void *a = NULL, *b = NULL, *o0 = NULL, *o1 = NULL;
  size_t la = 0, lb = 0;
  napi_typedarray_type t; bool is_ta = false;
  if (!get_i32(env, argv[0], &op) || op < 0 || op > 3 || napi_get_value_double(env, argv[3], &mod) != napi_ok ||
      !(mod >= 1.0 && mod <= 9007199254740992.0) || mod != (double)(int64_t)mod) BAD_ARGS();
  if (napi_is_typedarray(env, argv[1], &is_ta) != napi_ok || !is_ta ||
      napi_get_typedarray_info(env, argv[1], &t, &la, &a, NULL, NULL) != napi_ok || t != napi_float64_array) BAD_ARGS();
  if (napi_is_typedarray(env, argv[2], &is_ta) != napi_ok || !is_ta ||
      napi_get_typedarray_info(env, argv[2], &t, &lb, &b, NULL, NULL) != napi_ok || t != napi_float64_array) BAD_ARGS();
  const size_t cap = (size_t)ntru_generic_capacity((int)la, (int)lb);
  if (!get_buf(env, argv[4], napi_float64_array, cap, 0, &o0) || !get_buf(env, argv[5], napi_float64_array, cap, 1, &o1)) BAD_ARGS();
  if ((op == 1 || op == 2) && !o1) BAD_ARGS();
  if (!ensure_engine(env)) return NULL;
  int64_t *buf = (int64_t *)malloc((la + lb + 2 * cap + 2) * sizeof(int64_t));
  if (!buf) { napi_throw_error(env, NULL, "out of memory"); return NULL; }
  int64_t *ia = buf, *ib = ia + la + 1, *r0 = ib + lb + 1, *r1 = r0 + cap;
  for (size_t i = 0; i < la + lb; i++) {                      /* doubles -> int64: integers only, and only where the cast is defined */
    const double v = i < la ? ((double *)a)[i] : ((double *)b)[i - la];
    if (!(v >= -9007199254740992.0 && v <= 9007199254740992.0) || v != (double)(int64_t)v) {
      free(buf);
      napi_throw_type_error(env, NULL, "coefficients must be integers");
      return NULL;
    }
    if (i < la) ia[i] = (int64_t)v; else ib[i - la] = (int64_t)v;
  }
  int32_t len0 = 0, len1 = 0; uint8_t st = 0;
  int rc;
  if (op == 0) ENGINE_CALL(rc, ntru_generic_multiply(g_engine, (int)la, (int)lb, (int64_t)mod, ia, ib, 1, r0, &len0));
  else if (op == 1) ENGINE_CALL(rc, ntru_generic_divide(g_engine, (int)la, (int)lb, (int64_t)mod, ia, ib, 1, r0, &len0, r1, &len1, &st));
  else if (op == 2) ENGINE_CALL(rc, ntru_generic_eea(g_engine, (int)la, (int)lb, (int64_t)mod, ia, ib, 1, r0, &len0, r1, &len1, &st));
  else ENGINE_CALL(rc, ntru_generic_poly_inv(g_engine, (int)la, (int)lb, (int64_t)mod, ia, ib, 1, r0, &len0, &st));
  if (!rc) {
    for (int32_t i = 0; i < len0; i++) ((double *)o0)[i] = (double)r0[i];
    if (o1) for (int32_t i = 0; i < len1; i++) ((double *)o1)[i] = (double)r1[i];
  }
  free(buf);
  if (rc) return throw_engine(env, rc);
  napi_value arr; NAPI_OK(napi_create_array_with_length(env, 3, &arr));
  const int32_t v[3] = {st, len0, len1};
  for (int i = 0; i < 3; i++) { napi_value n; NAPI_OK(napi_create_int32(env, v[i], &n)); NAPI_OK(napi_set_element(env, arr, i, n)); }
  return arr;
}

/* ---- device buffers (additive): devAlloc / devUpload / devDownload / devFree hand out opaque handles for the engine's *_dev entry
 *      points, for callers that compose the stages themselves.  Every call on handles checks the byte size of each against what the
 *      kernel will touch before anything is launched. */
typedef struct DevBuf { void *p; size_t bytes; struct DevBuf *next; } DevBuf;
/* Every live handle of THIS addon.  An external value made by anybody else (another addon, a foreign napi_external) carries a data
 * pointer that is not in this list and is refused by get_dev without ever being dereferenced. */
static DevBuf *g_devs = NULL;
static pthread_mutex_t g_devs_lock = PTHREAD_MUTEX_INITIALIZER;
static void devs_add(DevBuf *b) { pthread_mutex_lock(&g_devs_lock); b->next = g_devs; g_devs = b; pthread_mutex_unlock(&g_devs_lock); }
static void devs_remove(DevBuf *b) {
  pthread_mutex_lock(&g_devs_lock);
  for (DevBuf **pp = &g_devs; *pp; pp = &(*pp)->next) if (*pp == b) { *pp = b->next; break; }
  pthread_mutex_unlock(&g_devs_lock);
}
static int devs_has(const void *data) {
  int found = 0;
  pthread_mutex_lock(&g_devs_lock);
  for (DevBuf *b = g_devs; b; b = b->next) if ((const void *)b == data) { found = 1; break; }
  pthread_mutex_unlock(&g_devs_lock);
  return found;
}

static void devbuf_finalize(napi_env env, void *data, void *hint) {
  (void)env; (void)hint;
  DevBuf *b = (DevBuf *)data;
  devs_remove(b);
  if (b->p) {                       /* not freed explicitly: release it with the handle (the engine may be gone already: then leak) */
    pthread_mutex_lock(&g_lock);
    if (g_engine) (void)ntru_dev_free(g_engine, b->p);
    pthread_mutex_unlock(&g_lock);
  }
  free(b);
}

static DevBuf *get_dev(napi_env env, napi_value v, size_t need, int optional, int *ok) {
  napi_valuetype vt;
  *ok = 0;
  if (napi_typeof(env, v, &vt) != napi_ok) return NULL;
  if (vt == napi_null || vt == napi_undefined) { *ok = optional; return NULL; }
  if (vt != napi_external) return NULL;
  void *data = NULL;
  if (napi_get_value_external(env, v, &data) != napi_ok || !data || !devs_has(data)) return NULL;   /* not one of ours: refused */
  DevBuf *b = (DevBuf *)data;
  if (!b->p || b->bytes < need) return NULL;
  *ok = 1;
  return b;
}

/* devAlloc(bytes) -> handle */
static napi_value DevAlloc(napi_env env, napi_callback_info info) {
  ARGS(1)
  double bytes;
  if (napi_get_value_double(env, argv[0], &bytes) != napi_ok || bytes < 0 || bytes > 281474976710656.0) BAD_ARGS();
  if (!ensure_engine(env)) return NULL;
  DevBuf *b = (DevBuf *)calloc(1, sizeof *b);
  if (!b) { napi_throw_error(env, NULL, "out of memory"); return NULL; }
  int rc;
  ENGINE_CALL(rc, ntru_dev_alloc(g_engine, (size_t)bytes, &b->p));
  if (rc) { free(b); return throw_engine(env, rc); }
  b->bytes = (size_t)bytes;
  devs_add(b);
  napi_value ext;
  if (napi_create_external(env, b, devbuf_finalize, NULL, &ext) != napi_ok) {
    devs_remove(b);
    ENGINE_CALL(rc, ntru_dev_free(g_engine, b->p)); free(b);
    napi_throw_error(env, NULL, "napi_create_external failed"); return NULL;
  }
  return ext;
}

/* devFree(handle) */
static napi_value DevFree(napi_env env, napi_callback_info info) {
  ARGS(1)
  int ok; DevBuf *b = get_dev(env, argv[0], 0, 0, &ok);
  if (!ok) BAD_ARGS();
  if (!ensure_engine(env)) return NULL;
  int rc;
  ENGINE_CALL(rc, ntru_dev_free(g_engine, b->p));
  b->p = NULL; b->bytes = 0;
  return rc ? throw_engine(env, rc) : undefined(env);
}

/* Bytes per element, by napi_typedarray_type (int8 .. biguint64) */
static const size_t elem_width[] = {1, 1, 1, 2, 2, 4, 4, 4, 8, 8, 8};

/* The bytes of any TypedArray. */
static int get_any(napi_env env, napi_value v, void **data, size_t *bytes) {
  bool is_ta = false;
  if (napi_is_typedarray(env, v, &is_ta) != napi_ok || !is_ta) return 0;
  napi_typedarray_type t; size_t len;
  if (napi_get_typedarray_info(env, v, &t, &len, data, NULL, NULL) != napi_ok) return 0;
  if ((int)t < 0 || (size_t)t >= sizeof elem_width / sizeof elem_width[0]) return 0;
  *bytes = len * elem_width[t];
  return 1;
}

/* devUpload(handle, src:TypedArray): the whole array to the start of the buffer */
static napi_value DevUpload(napi_env env, napi_callback_info info) {
  ARGS(2)
  void *src; size_t bytes;
  if (!get_any(env, argv[1], &src, &bytes)) BAD_ARGS();
  int ok; DevBuf *b = get_dev(env, argv[0], bytes, 0, &ok);
  if (!ok) BAD_ARGS();
  if (!ensure_engine(env)) return NULL;
  int rc;
  ENGINE_CALL(rc, ntru_dev_upload(g_engine, b->p, src, bytes));
  return rc ? throw_engine(env, rc) : undefined(env);
}

/* devDownload(dst:TypedArray, handle): the first dst.byteLength bytes of the buffer; waits for the engine's stream */
static napi_value DevDownload(napi_env env, napi_callback_info info) {
  ARGS(2)
  void *dst; size_t bytes;
  if (!get_any(env, argv[0], &dst, &bytes)) BAD_ARGS();
  int ok; DevBuf *b = get_dev(env, argv[1], bytes, 0, &ok);
  if (!ok) BAD_ARGS();
  if (!ensure_engine(env)) return NULL;
  int rc;
  ENGINE_CALL(rc, ntru_dev_download(g_engine, dst, b->p, bytes));
  return rc ? throw_engine(env, rc) : undefined(env);
}

/* packBatchDev(maxVal, dataLen, data:handle, B, out:handle[B*outputSize*32 bytes], bytes:boolean)   bytes: data holds uint8 values */
static napi_value PackBatchDev(napi_env env, napi_callback_info info) {
  ARGS(6)
  int32_t max_val, data_len, B; bool is_bytes; int ok_data, ok_out;
  if (!get_i32(env, argv[0], &max_val) || !get_i32(env, argv[1], &data_len) || !get_i32(env, argv[3], &B) || data_len < 0 || B < 0 ||
      napi_get_value_bool(env, argv[5], &is_bytes) != napi_ok) BAD_ARGS();
  int bits, per, al, os;
  if (ntru_pack_params(max_val, data_len, &bits, &per, &al, &os)) return throw_engine(env, NTRU_ERR_ARG);
  DevBuf *data = get_dev(env, argv[2], (size_t)B * (size_t)data_len * (is_bytes ? 1 : 2), 0, &ok_data);
  DevBuf *out = get_dev(env, argv[4], (size_t)B * (size_t)os * 32, 0, &ok_out);
  if (!ok_data || !ok_out) BAD_ARGS();
  if (!ensure_engine(env)) return NULL;
  int rc;
  ENGINE_CALL(rc, is_bytes ? ntru_pack_bytes_batch_dev(g_engine, max_val, data_len, data->p, B, out->p)
                           : ntru_pack_batch_dev(g_engine, max_val, data_len, data->p, B, out->p));
  return rc ? throw_engine(env, rc) : undefined(env);
}

/* keygenWorkspaceBytes(N, B) -> bytes of the workspace handle keygenBatchDev needs */
static napi_value KeygenWorkspaceBytes(napi_env env, napi_callback_info info) {
  ARGS(2)
  int32_t N, B;
  if (!get_i32(env, argv[0], &N) || !get_i32(env, argv[1], &B) || B < 0) BAD_ARGS();
  size_t bytes = 0;
  int rc = ntru_keygen_workspace_bytes(N, B, &bytes);
  if (rc) return throw_engine(env, rc);
  napi_value v;
  NAPI_OK(napi_create_double(env, (double)bytes, &v));
  return v;
}

/* ---- the batch calls.  Each engine operation is described ONCE, as a row of ops[] below: its JS arguments in order, and a run() that
 *      spells the engine call from the parsed arguments.  The JS forms are derived from the row by parse_call and three entry points:
 *        name(...)       on host TypedArrays;
 *        nameDev(...)    on device-buffer handles: every BUF becomes a handle of at least the same BYTES (elements * element width),
 *                        a HOSTBUF stays a TypedArray; checked before anything is launched;
 *        nameAsync(...)  the host form on a libuv worker thread, -> Promise<undefined>.
 *      A new call is one run function and one row. */
#define MAX_ARGS 17
#define MAX_BUFS 12

typedef struct {
  int32_t N, q, p, B, K, G, n1, n2, other, nq, np, df, dg, max_tries;   /* the int32 arguments, by name (a modulus of any name is q) */
  uint64_t first;                                                      /* firstItem */
  void *ptr[MAX_BUFS];                   /* the buffers in argument order: host pointers, device pointers in the Dev form; NULL = absent */
} Args;

enum { A_END, A_INT, A_FIRST, A_BUF };
/* How many elements a buffer needs.  SZ_PACKED_*: B rows of packOutput field elements, four uint64 limbs each. */
enum { SZ_N, SZ_B, SZ_NB, SZ_2NB, SZ_N1B, SZ_GN, SZ_G1, SZ_KEY, SZ_PACKED_Q, SZ_PACKED_PIPELINE, SZ_KEYGEN_WORK };
enum { OPTIONAL = 1, HOST_ALWAYS = 2, OFFSETS = 4 };
typedef struct { uint8_t kind, field, type, size, flags; } Arg;
#define INT(f) {A_INT, offsetof(Args, f), 0, 0, 0}                /* int32 */
#define FIRST {A_FIRST, 0, 0, 0, 0}                               /* Number, an integer 0 .. 2^53 - 1 */
#define BUF(t, sz) {A_BUF, 0, t, sz, 0}
#define OPT(t, sz) {A_BUF, 0, t, sz, OPTIONAL}                    /* may be null / undefined */
#define HOSTBUF(t, sz) {A_BUF, 0, t, sz, HOST_ALWAYS}
#define OFFS {A_BUF, 0, I64, SZ_G1, OPTIONAL | OFFSETS}           /* the offsets of a sum: groups_fit is applied after parsing */
#define I8 napi_int8_array
#define U8 napi_uint8_array
#define U16 napi_uint16_array
#define U32 napi_uint32_array
#define I64 napi_bigint64_array
#define U64 napi_biguint64_array

typedef struct {
  const char *name;                      /* of the host form; the others append Dev / Async */
  int forms;
  int (*run)(const Args *a, int dev);    /* called under g_lock, on the JS thread or on a worker */
  Arg args[MAX_ARGS + 1];
} Op;
enum { HOST = 1, DEV = 2, ASYNC = 4 };

/* The groups of a sum over B rows: offsets (BigInt64Array[G + 1], non-decreasing, 0 <= offsets[0], offsets[G] <= B) or uniform K with
 * G * K == B.  Only what keeps the engine inside the arrays is checked here; the engine reports the rest. */
static int groups_fit(const int64_t *off, int64_t K, int64_t G, int64_t B) {
  if (G < 0 || B < 0) return 0;
  if (!off) return K >= 1 && G <= B / K + 1 && G * K == B;
  if (off[0] < 0) return 0;
  for (int64_t g = 0; g < G; g++) if (off[g + 1] < off[g]) return 0;
  return off[G] <= B;
}

static size_t packed_elems(int max_val, const Args *a) {           /* 0 where ntru_pack_params refuses: the engine call reports it */
  int bits, per, al, os;
  return ntru_pack_params(max_val, a->N, &bits, &per, &al, &os) == 0 ? (size_t)a->B * (size_t)os * 4 : 0;
}

/* Throws the engine's error and returns 0 where the keygen workspace has no size (N out of range). */
static int elems(napi_env env, int rule, const Args *a, size_t *need) {
  const size_t N = (size_t)a->N, B = (size_t)a->B, G = (size_t)a->G;
  switch (rule) {
    case SZ_N: *need = N; break;
    case SZ_B: *need = B; break;
    case SZ_NB: *need = N * B; break;
    case SZ_2NB: *need = 2 * N * B; break;                        /* splitByI's dividends */
    case SZ_N1B: *need = (N + 1) * B; break;                      /* witness rows with the trailing [N]-th coefficient */
    case SZ_GN: *need = G * N; break;
    case SZ_G1: *need = G + 1; break;
    case SZ_KEY: *need = 8; break;
    case SZ_PACKED_Q: *need = packed_elems(a->q - 1, a); break;
    case SZ_PACKED_PIPELINE: *need = packed_elems(a->ptr[1] ? a->p - 1 : a->q - 1, a); break;   /* ptr[1] = f: value is packed, else e */
    default: {                                                    /* SZ_KEYGEN_WORK, in bytes */
      int rc = ntru_keygen_workspace_bytes(a->N, a->B, need);
      if (rc) { throw_engine(env, rc); return 0; }
    }
  }
  return 1;
}

/* Reads the arguments of a call as its row (the `data` of the property) describes them, into *a and argv[MAX_ARGS].  Validation first,
 * then the engine must exist; on any refusal throws and returns NULL. */
static const Op *parse_call(napi_env env, napi_callback_info info, int dev, Args *a, napi_value *argv) {
  size_t argc = MAX_ARGS, nargs = 0;
  void *data = NULL;
  NAPI_OK(napi_get_cb_info(env, info, &argc, argv, NULL, &data));
  const Op *op = (const Op *)data;
  while (op->args[nargs].kind != A_END) nargs++;
  if (argc < nargs) { napi_throw_type_error(env, NULL, "too few arguments"); return NULL; }
  memset(a, 0, sizeof *a);
  for (size_t i = 0; i < nargs; i++) {                            /* the scalars first: the sizes of the buffers depend on them */
    const Arg *g = &op->args[i];
    double first;
    if (g->kind == A_INT && !get_i32(env, argv[i], (int32_t *)((char *)a + g->field))) BAD_ARGS();
    if (g->kind != A_FIRST) continue;
    if (napi_get_value_double(env, argv[i], &first) != napi_ok || first < 0 || first > 9007199254740991.0) BAD_ARGS();
    a->first = (uint64_t)first;
  }
  if (a->N < 1 || a->B < 0 || a->G < 0) BAD_ARGS();
  int nbuf = 0, grouped = 0;
  const void *offsets = NULL;
  for (size_t i = 0; i < nargs; i++) {
    const Arg *g = &op->args[i];
    if (g->kind != A_BUF) continue;
    const int optional = g->flags & OPTIONAL;
    size_t need;
    if (!elems(env, g->size, a, &need)) return NULL;
    if (dev && !(g->flags & HOST_ALWAYS)) {
      int ok;
      DevBuf *b = get_dev(env, argv[i], need * elem_width[g->type], optional, &ok);
      if (!ok) BAD_ARGS();
      a->ptr[nbuf] = b ? b->p : NULL;
    } else if (!get_buf(env, argv[i], (napi_typedarray_type)g->type, need, optional, &a->ptr[nbuf])) BAD_ARGS();
    if (g->flags & OFFSETS) { grouped = 1; offsets = a->ptr[nbuf]; }
    nbuf++;
  }
  /* offsets on the device cannot be read here: the handle sizes were checked against the B the caller states, offsets[G] <= B is the
   * caller's promise */
  if (grouped && !(dev && offsets) && !groups_fit((const int64_t *)offsets, a->K, a->G, a->B)) BAD_ARGS();
  if (!ensure_engine(env)) return NULL;
  return op;
}

#define RUN(name) static int name(const Args *a, int dev)
#define P(i) a->ptr[i]
RUN(run_polymul_split) {
  return dev ? ntru_polymul_split_dev(g_engine, a->N, a->q, P(0), P(1), a->B, P(2), P(3))
             : ntru_polymul_split(g_engine, a->N, a->q, P(0), P(1), a->B, P(2), P(3));
}
RUN(run_split_by_I) { (void)dev; return ntru_split_by_I(g_engine, a->N, a->q, P(0), a->B, P(1), P(2)); }
RUN(run_add) { (void)dev; return ntru_add_batch(g_engine, a->N, a->q, P(0), P(1), a->B, P(2)); }
RUN(run_invert_key) {
  return dev ? ntru_invert_key_batch_dev(g_engine, a->N, a->q, a->p, P(0), a->B, P(1), P(2), P(3))
             : ntru_invert_key_batch(g_engine, a->N, a->q, a->p, P(0), a->B, P(1), P(2), P(3));
}
RUN(run_public_key) {
  return dev ? ntru_public_key_batch_dev(g_engine, a->N, a->q, a->p, P(0), P(1), a->B, P(2))
             : ntru_public_key_batch(g_engine, a->N, a->q, a->p, P(0), P(1), a->B, P(2));
}
/* useDevices([...]) shards the host forms of encrypt, decrypt and verifyKeys over its devices, synchronous or not */
RUN(run_encrypt) {
  if (dev) return ntru_encrypt_batch_dev(g_engine, a->N, a->q, P(0), P(1), P(2), a->B, P(3), P(4));
  return g_multi ? ntru_multi_encrypt_batch(g_multi, a->N, a->q, P(0), P(1), P(2), a->B, P(3), P(4))
                 : ntru_encrypt_batch(g_engine, a->N, a->q, P(0), P(1), P(2), a->B, P(3), P(4));
}
RUN(run_decrypt) {
  if (dev) return ntru_decrypt_batch_dev(g_engine, a->N, a->q, a->p, P(0), P(1), P(2), a->B, P(3), P(4), P(5), P(6));
  return g_multi ? ntru_multi_decrypt_batch(g_multi, a->N, a->q, a->p, P(0), P(1), P(2), a->B, P(3), P(4), P(5), P(6))
                 : ntru_decrypt_batch(g_engine, a->N, a->q, a->p, P(0), P(1), P(2), a->B, P(3), P(4), P(5), P(6));
}
RUN(run_encrypt_peritem) {
  return dev ? ntru_encrypt_peritem_batch_dev(g_engine, a->N, a->q, P(0), P(1), P(2), a->B, P(3), P(4))
             : ntru_encrypt_peritem_batch(g_engine, a->N, a->q, P(0), P(1), P(2), a->B, P(3), P(4));
}
RUN(run_decrypt_peritem) {
  return dev ? ntru_decrypt_peritem_batch_dev(g_engine, a->N, a->q, a->p, P(0), P(1), P(2), a->B, P(3), P(4), P(5), P(6))
             : ntru_decrypt_peritem_batch(g_engine, a->N, a->q, a->p, P(0), P(1), P(2), a->B, P(3), P(4), P(5), P(6));
}
RUN(run_verify_keys) {
  if (dev) return ntru_verify_keys_batch_dev(g_engine, a->N, a->q, a->p, P(0), P(1), P(2), P(3), P(4), a->B, P(5), P(6), P(7), P(8), P(9), P(10), P(11));
  return g_multi ? ntru_multi_verify_keys_batch(g_multi, a->N, a->q, a->p, P(0), P(1), P(2), P(3), P(4), a->B, P(5), P(6), P(7), P(8), P(9), P(10), P(11))
                 : ntru_verify_keys_batch(g_engine, a->N, a->q, a->p, P(0), P(1), P(2), P(3), P(4), a->B, P(5), P(6), P(7), P(8), P(9), P(10), P(11));
}
/* Witness checks: the signals in the order of the template's inputs (circuits/ntru.circom) */
RUN(run_check_encrypt) { (void)dev; return ntru_check_encrypt_batch(g_engine, a->N, a->q, a->nq, P(0), P(1), P(2), P(3), P(4), a->B, P(5)); }
RUN(run_check_decrypt) {
  (void)dev;
  return ntru_check_decrypt_batch(g_engine, a->N, a->q, a->nq, a->p, a->np, P(0), P(1), P(2), P(3), P(4), P(5), P(6), a->B, P(7));
}
RUN(run_check_inverse) { (void)dev; return ntru_check_inverse_batch(g_engine, a->N, a->q, a->nq, P(0), P(1), P(2), P(3), a->B, P(4)); }
RUN(run_sample_ternary) {
  return dev ? ntru_sample_ternary_dev(g_engine, a->N, a->n1, a->n2, a->other, P(0), a->first, a->B, P(1))
             : ntru_sample_ternary(g_engine, a->N, a->n1, a->n2, a->other, P(0), a->first, a->B, P(1));
}
/* sampler -> encryptBits -> decryptBits -> packOutput on the GPU for a batch of host plaintexts */
RUN(run_pipeline) {
  (void)dev;
  return ntru_pipeline_batch(g_engine, a->N, a->q, a->p, P(0), P(1), P(2), P(3), a->first, a->n1, a->n2, P(4), P(5), a->B, P(6), P(7), P(8), P(9));
}
RUN(run_sum_groups) {
  return dev ? ntru_sum_groups_dev(g_engine, a->N, a->q, P(0), P(1), P(2), a->K, a->G, P(3))
             : ntru_sum_groups(g_engine, a->N, a->q, P(0), P(1), P(2), a->K, a->G, P(3));
}
RUN(run_tally_decrypt) {
  return dev ? ntru_tally_decrypt_batch_dev(g_engine, a->N, a->q, a->p, P(0), P(1), P(2), P(3), P(4), a->K, a->G, P(5), P(6), P(7), P(8), P(9))
             : ntru_tally_decrypt_batch(g_engine, a->N, a->q, a->p, P(0), P(1), P(2), P(3), P(4), a->K, a->G, P(5), P(6), P(7), P(8), P(9));
}
/* generatePrivateKeyF + generateNewPublicKeyGH for B items, non-units redrawn on the device.  The Dev form has a list of its own: a
 * workspace handle of keygenWorkspaceBytes(N, B), every output but tries needed, no packedH; it waits for the engine's stream once per
 * call and once per redraw pass (a 4-byte count). */
RUN(run_keygen) {
  (void)dev;
  return ntru_keygen_batch(g_engine, a->N, a->q, a->p, a->df, a->dg, P(0), a->first, a->max_tries, a->B, P(1), P(2), P(3), P(4), P(5), P(6), P(7), P(8));
}
RUN(run_keygen_dev) {
  (void)dev;
  return ntru_keygen_batch_dev(g_engine, a->N, a->q, a->p, a->df, a->dg, P(0), a->first, a->max_tries, a->B, P(1), P(2), P(3), P(4), P(5), P(6), P(7), P(8));
}

/* The JS argument lists.  Rows are [B][N] unless the size says otherwise; BUF / OPT name the element type of the host form. */
static const Op ops[] = {
  /* (N, mod, a, b, B, quot, rem) */
  {"polymulSplit", HOST | DEV, run_polymul_split, {INT(N), INT(q), BUF(U16, SZ_NB), BUF(U16, SZ_NB), INT(B), BUF(U16, SZ_NB), BUF(U16, SZ_NB)}},
  /* (N, mod, a[B][2N], B, quot, rem) */
  {"splitByI", HOST, run_split_by_I, {INT(N), INT(q), BUF(U16, SZ_2NB), INT(B), BUF(U16, SZ_NB), BUF(U16, SZ_NB)}},
  /* (N, mod, a, b, B, out) */
  {"addBatch", HOST, run_add, {INT(N), INT(q), BUF(U16, SZ_NB), BUF(U16, SZ_NB), INT(B), BUF(U16, SZ_NB)}},
  /* (N, q, p, f, B, fq|null, fp|null, flags[B]) */
  {"invertKeyBatch", HOST | DEV, run_invert_key,
   {INT(N), INT(q), INT(p), BUF(I8, SZ_NB), INT(B), OPT(U16, SZ_NB), OPT(U8, SZ_NB), BUF(U8, SZ_B)}},
  /* (N, q, p, fq, g, B, h) */
  {"publicKeyBatch", HOST | DEV, run_public_key, {INT(N), INT(q), INT(p), BUF(U16, SZ_NB), BUF(I8, SZ_NB), INT(B), BUF(U16, SZ_NB)}},
  /* (N, q, h[N], r, m, B, e, quotE|null) */
  {"encryptBatch", HOST | DEV | ASYNC, run_encrypt,
   {INT(N), INT(q), BUF(U16, SZ_N), BUF(U8, SZ_NB), BUF(U8, SZ_NB), INT(B), BUF(U16, SZ_NB), OPT(U16, SZ_NB)}},
  /* (N, q, p, f[N], fp[N], e, B, value, quot1|null, rem1|null, quot2|null) */
  {"decryptBatch", HOST | DEV | ASYNC, run_decrypt,
   {INT(N), INT(q), INT(p), BUF(I8, SZ_N), BUF(U8, SZ_N), BUF(U16, SZ_NB), INT(B), BUF(U8, SZ_NB), OPT(U16, SZ_NB), OPT(U16, SZ_NB), OPT(U8, SZ_NB)}},
  /* the same two with row b under key b: h, f, fp are [B][N] */
  {"encryptPeritemBatch", HOST | DEV, run_encrypt_peritem,
   {INT(N), INT(q), BUF(U16, SZ_NB), BUF(U8, SZ_NB), BUF(U8, SZ_NB), INT(B), BUF(U16, SZ_NB), OPT(U16, SZ_NB)}},
  {"decryptPeritemBatch", HOST | DEV, run_decrypt_peritem,
   {INT(N), INT(q), INT(p), BUF(I8, SZ_NB), BUF(U8, SZ_NB), BUF(U16, SZ_NB), INT(B), BUF(U8, SZ_NB), OPT(U16, SZ_NB), OPT(U16, SZ_NB), OPT(U8, SZ_NB)}},
  /* (N, q, p, f, g, fq, fp, h, B, quotFq, remFq, quotFp, remFp, quotH, remH, flags[B]) */
  {"verifyKeysBatch", HOST | DEV, run_verify_keys,
   {INT(N), INT(q), INT(p), BUF(I8, SZ_NB), BUF(I8, SZ_NB), BUF(U16, SZ_NB), BUF(U8, SZ_NB), BUF(U16, SZ_NB), INT(B), BUF(U16, SZ_NB), BUF(U16, SZ_NB),
    BUF(U8, SZ_NB), BUF(U8, SZ_NB), BUF(U16, SZ_NB), BUF(U16, SZ_NB), BUF(U8, SZ_B)}},
  /* (N, q, nq, r, m, h, quotientE[B][N+1], remainderE[B][N+1], B, flags[B]) */
  {"checkEncryptBatch", HOST, run_check_encrypt,
   {INT(N), INT(q), INT(nq), BUF(U16, SZ_NB), BUF(U16, SZ_NB), BUF(U16, SZ_NB), BUF(U16, SZ_N1B), BUF(U16, SZ_N1B), INT(B), BUF(U8, SZ_B)}},
  /* (N, q, nq, p, np, f, fp, e, quotient1, remainder1, quotient2, remainder2 (the last four [B][N+1]), B, flags[B]) */
  {"checkDecryptBatch", HOST, run_check_decrypt,
   {INT(N), INT(q), INT(nq), INT(p), INT(np), BUF(U16, SZ_NB), BUF(U16, SZ_NB), BUF(U16, SZ_NB), BUF(U16, SZ_N1B), BUF(U16, SZ_N1B), BUF(U16, SZ_N1B),
    BUF(U16, SZ_N1B), INT(B), BUF(U8, SZ_B)}},
  /* (N, M, n, f, fq, quotientI[B][N+1], remainderI[B][N+1], B, flags[B]) */
  {"checkInverseBatch", HOST, run_check_inverse,
   {INT(N), INT(q), INT(nq), BUF(U16, SZ_NB), BUF(U16, SZ_NB), BUF(U16, SZ_N1B), BUF(U16, SZ_N1B), INT(B), BUF(U8, SZ_B)}},
  /* (N, n1, n2, other, key:Uint32Array[8], firstItem, B, out) */
  {"sampleTernary", HOST | DEV, run_sample_ternary,
   {INT(N), INT(n1), INT(n2), INT(other), HOSTBUF(U32, SZ_KEY), FIRST, INT(B), BUF(U8, SZ_NB)}},
  /* (N, q, p, h[N], f[N]|null, fp[N]|null, key[8]|null, firstItem, n1, n2, r|null, m, B, rOut|null, e|null, value|null,
   *  packed:BigUint64Array[B][outputSize][4]|null) */
  {"pipelineBatch", HOST | ASYNC, run_pipeline,
   {INT(N), INT(q), INT(p), BUF(U16, SZ_N), OPT(I8, SZ_N), OPT(U8, SZ_N), OPT(U32, SZ_KEY), FIRST, INT(n1), INT(n2), OPT(U8, SZ_NB), BUF(U8, SZ_NB),
    INT(B), OPT(U8, SZ_NB), OPT(U16, SZ_NB), OPT(U8, SZ_NB), OPT(U64, SZ_PACKED_PIPELINE)}},
  /* (N, mod, rows, weights[B]|null, offsets:BigInt64Array[G+1]|null, K, G, B, out[G][N]) */
  {"sumGroups", HOST | DEV, run_sum_groups,
   {INT(N), INT(q), BUF(U16, SZ_NB), OPT(U16, SZ_B), OFFS, INT(K), INT(G), INT(B), BUF(U16, SZ_GN)}},
  /* (N, q, p, f[N], fp[N], rows, weights[B]|null, offsets[G+1]|null, K, G, B, sum[G][N], value[G][N], quot1|null, rem1|null, quot2|null) */
  {"tallyDecryptBatch", HOST | DEV | ASYNC, run_tally_decrypt,
   {INT(N), INT(q), INT(p), BUF(I8, SZ_N), BUF(U8, SZ_N), BUF(U16, SZ_NB), OPT(U16, SZ_B), OFFS, INT(K), INT(G), INT(B), BUF(U16, SZ_GN),
    BUF(U8, SZ_GN), OPT(U16, SZ_GN), OPT(U16, SZ_GN), OPT(U8, SZ_GN)}},
  /* (N, q, p, df, dg, key[8], firstItem, maxTries, B, f|null, g|null, fq|null, fp|null, h|null, tries[B]|null, flags[B],
   *  packedH:BigUint64Array[B][outputSize][4]|null) */
  {"keygenBatch", HOST | ASYNC, run_keygen,
   {INT(N), INT(q), INT(p), INT(df), INT(dg), BUF(U32, SZ_KEY), FIRST, INT(max_tries), INT(B), OPT(I8, SZ_NB), OPT(I8, SZ_NB), OPT(U16, SZ_NB),
    OPT(U8, SZ_NB), OPT(U16, SZ_NB), OPT(U8, SZ_B), BUF(U8, SZ_B), OPT(U64, SZ_PACKED_Q)}},
  /* keygenBatchDev(N, q, p, df, dg, key[8], firstItem, maxTries, B, work, f, g, fq, fp, h, tries[B]|null, flags[B]) */
  {"keygenBatch", DEV, run_keygen_dev,
   {INT(N), INT(q), INT(p), INT(df), INT(dg), HOSTBUF(U32, SZ_KEY), FIRST, INT(max_tries), INT(B), BUF(U8, SZ_KEYGEN_WORK), BUF(I8, SZ_NB),
    BUF(I8, SZ_NB), BUF(U16, SZ_NB), BUF(U8, SZ_NB), BUF(U16, SZ_NB), OPT(U8, SZ_B), BUF(U8, SZ_B)}},
};

static napi_value call_sync(napi_env env, napi_callback_info info, int dev) {
  napi_value argv[MAX_ARGS];
  Args a;
  const Op *op = parse_call(env, info, dev, &a, argv);
  if (!op) return NULL;
  int rc;
  ENGINE_CALL(rc, op->run(&a, dev));
  return rc ? throw_engine(env, rc) : undefined(env);
}
static napi_value CallHost(napi_env env, napi_callback_info info) { return call_sync(env, info, 0); }
static napi_value CallDev(napi_env env, napi_callback_info info) { return call_sync(env, info, 1); }

/* ---- the Async form (additive; the reference API stays synchronous): the engine call runs on a libuv worker thread, so the event loop
 *      keeps turning while a 2^18-item batch (tens of milliseconds of PCIe) is in flight.  The typed arrays are pinned by references
 *      until the Promise settles; the caller must not touch the output arrays before that. */
typedef struct {
  napi_async_work work;
  napi_deferred deferred;
  napi_ref keep[MAX_ARGS];
  int n_keep;
  const Op *op;
  Args a;
  int rc;
  char err[400];
} AsyncJob;

static void async_execute(napi_env env, void *data) {
  (void)env;
  AsyncJob *j = (AsyncJob *)data;
  pthread_mutex_lock(&g_lock);
  if (!g_engine) { j->rc = NTRU_ERR_ARG; snprintf(j->err, sizeof j->err, "ntru engine not created"); }
  else if ((j->rc = j->op->run(&j->a, 0)) != 0)
    snprintf(j->err, sizeof j->err, "ntru engine error %d: %s", j->rc, ntru_last_error());   /* per thread: read it here */
  pthread_mutex_unlock(&g_lock);
}

static void async_complete(napi_env env, napi_status status, void *data) {
  AsyncJob *j = (AsyncJob *)data;
  napi_value v;
  if (status == napi_ok && j->rc == 0) {
    napi_get_undefined(env, &v);
    napi_resolve_deferred(env, j->deferred, v);
  } else {
    napi_value msg;
    napi_create_string_utf8(env, status == napi_ok ? j->err : "ntru engine: asynchronous work was cancelled", NAPI_AUTO_LENGTH, &msg);
    napi_create_error(env, NULL, msg, &v);
    napi_reject_deferred(env, j->deferred, v);
  }
  for (int i = 0; i < j->n_keep; i++) napi_delete_reference(env, j->keep[i]);
  napi_delete_async_work(env, j->work);
  free(j);
}

static napi_value CallAsync(napi_env env, napi_callback_info info) {
  napi_value argv[MAX_ARGS], promise, rname;
  Args a;
  const Op *op = parse_call(env, info, 0, &a, argv);
  if (!op) return NULL;
  AsyncJob *j = (AsyncJob *)calloc(1, sizeof *j);
  if (!j) { napi_throw_error(env, NULL, "out of memory"); return NULL; }
  j->op = op; j->a = a;
  if (napi_create_promise(env, &j->deferred, &promise) != napi_ok) { free(j); napi_throw_error(env, NULL, "napi_create_promise failed"); return NULL; }
  for (int i = 0; i < MAX_ARGS; i++) {                            /* every argument that is an object: the arrays */
    napi_valuetype vt;
    if (napi_typeof(env, argv[i], &vt) == napi_ok && vt == napi_object &&
        napi_create_reference(env, argv[i], 1, &j->keep[j->n_keep]) == napi_ok) j->n_keep++;
  }
  char name[64];
  snprintf(name, sizeof name, "ntru.%sAsync", op->name);
  napi_create_string_utf8(env, name, NAPI_AUTO_LENGTH, &rname);
  if (napi_create_async_work(env, NULL, rname, async_execute, async_complete, j, &j->work) != napi_ok ||
      napi_queue_async_work(env, j->work) != napi_ok) {
    for (int i = 0; i < j->n_keep; i++) napi_delete_reference(env, j->keep[i]);
    free(j);
    napi_throw_error(env, NULL, "could not queue asynchronous work");
    return NULL;
  }
  return promise;
}

static napi_value Init(napi_env env, napi_value exports) {
  static const struct { const char *name; napi_callback fn; } by_hand[] = {
    {"deviceCount", DeviceCount}, {"create", Create}, {"destroy", Destroy}, {"useDevices", UseDevices}, {"supports", Supports},
    {"setSamplerRounds", SetSamplerRounds}, {"packParams", PackParams}, {"packBatch", PackBatch}, {"unpackBatch", UnpackBatch},
    {"packBatchDev", PackBatchDev}, {"allocPinned", AllocPinned}, {"genericCapacity", GenericCapacity}, {"genericOp", GenericOp},
    {"devAlloc", DevAlloc}, {"devFree", DevFree}, {"devUpload", DevUpload}, {"devDownload", DevDownload},
    {"keygenWorkspaceBytes", KeygenWorkspaceBytes},
  };
  static const struct { int form; const char *suffix; napi_callback fn; } forms[] = {{HOST, "", CallHost}, {DEV, "Dev", CallDev}, {ASYNC, "Async", CallAsync}};
  enum { N_HAND = sizeof by_hand / sizeof by_hand[0], N_OPS = sizeof ops / sizeof ops[0] };
  napi_property_descriptor props[N_HAND + 3 * N_OPS];
  char names[3 * N_OPS][48];
  size_t n = 0, m = 0;
  for (size_t i = 0; i < N_HAND; i++)
    props[n++] = (napi_property_descriptor){by_hand[i].name, NULL, by_hand[i].fn, NULL, NULL, NULL, napi_default, NULL};
  for (size_t i = 0; i < N_OPS; i++)
    for (size_t k = 0; k < 3; k++) {
      if (!(ops[i].forms & forms[k].form)) continue;
      snprintf(names[m], sizeof names[m], "%s%s", ops[i].name, forms[k].suffix);
      props[n++] = (napi_property_descriptor){names[m++], NULL, forms[k].fn, NULL, NULL, NULL, napi_default, (void *)&ops[i]};
    }
  if (napi_define_properties(env, exports, n, props) != napi_ok) return NULL;
  return exports;
}

NAPI_MODULE(NODE_GYP_MODULE_NAME, Init)
