// Host-side sanitizer driver: the real abi.hip + ntru_host.hip, compiled as plain C++ against the fake HIP runtime and the fake
// device (fake_hip.cpp, fake_device.cpp), run under AddressSanitizer + UBSan and under ThreadSanitizer.  What is exercised: engine
// life cycle, the three-stage chunk pipeline (pinned and pageable buffers, single chunk / many chunks / ragged last chunk / empty batch),
// optional outputs, every regular host form, the shared scratch buffer across two user streams, ntru_multi_* (one host thread per
// shard, unequal and empty shards), two engines driven from two threads, error paths, and the small host helpers of engine_internal.h
// that the kernel files' host forms carve and hold buffers with.  Expected values come from the same formulas applied to the whole batch.
#include <hip/hip_runtime.h>

#include <atomic>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <thread>
#include <vector>

#include "fake_formulas.h"
#include "ntru_engine.h"
#include "engine_internal.h"

static int g_fail = 0;
static std::atomic<int> g_checks{0};          // (CHECK runs on two threads at once in one case)
#define CHECK(cond, ...) do { g_checks++; if (!(cond)) { g_fail++; fprintf(stderr, "FAIL %s:%d: ", __FILE__, __LINE__); fprintf(stderr, __VA_ARGS__); fprintf(stderr, "\n"); } } while (0)
#define OK(call) do { int rc_ = (call); CHECK(rc_ == 0, "%s -> %d (%s)", #call, rc_, ntru_last_error()); } while (0)

static thread_local uint32_t rng_state = 12345;
static uint32_t rnd() { rng_state = rng_state * 1664525u + 1013904223u; return rng_state >> 8; }

template <class T>
struct Buf {                 // pageable (std::vector) or pinned (ntru_host_alloc) host array
  std::vector<T> v;
  T *p = nullptr;
  size_t n = 0;
  bool pinned = false;
  Buf(size_t count, bool pin) : n(count), pinned(pin) {
    if (pin) p = (T *)ntru_host_alloc((count ? count : 1) * sizeof(T)); else { v.resize(count ? count : 1); p = v.data(); }
  }
  ~Buf() { if (pinned) ntru_host_free(p); }
  Buf(const Buf &) = delete;
};

static void round_trip(ntru_engine_t *eng, int N, int q, int64_t B, bool pin, bool witness) {
  const int p = 3;
  Buf<uint16_t> h(N, false), e(B * N, pin), quot(B * N, pin), e_want(B * N, false), quot_want(B * N, false);
  Buf<uint8_t> r(B * N, pin), m(B * N, pin);
  for (int i = 0; i < N; i++) h.p[i] = (uint16_t)(rnd() % q);
  for (int64_t i = 0; i < B * N; i++) { r.p[i] = (uint8_t)(rnd() % 3); m.p[i] = (uint8_t)(rnd() % 2); }
  OK(ntru_encrypt_batch(eng, N, q, h.p, r.p, m.p, B, e.p, witness ? quot.p : nullptr));
  fake_encrypt(N, q, h.p, r.p, m.p, B, e_want.p, quot_want.p);
  CHECK(memcmp(e.p, e_want.p, B * N * 2) == 0, "encrypt e, B=%ld pin=%d", (long)B, pin);
  if (witness) CHECK(memcmp(quot.p, quot_want.p, B * N * 2) == 0, "encrypt quot, B=%ld", (long)B);
  Buf<int8_t> f(N, false);
  Buf<uint8_t> fp(N, false), value(B * N, pin), q2(B * N, pin), value_want(B * N, false), q2_want(B * N, false);
  Buf<uint16_t> q1(B * N, pin), r1(B * N, pin), q1_want(B * N, false), r1_want(B * N, false);
  for (int i = 0; i < N; i++) { f.p[i] = (int8_t)((int)(rnd() % 3) - 1); fp.p[i] = (uint8_t)(rnd() % 3); }
  OK(ntru_decrypt_batch(eng, N, q, p, f.p, fp.p, e.p, B, value.p, witness ? q1.p : nullptr, witness ? r1.p : nullptr, witness ? q2.p : nullptr));
  fake_decrypt(N, q, p, f.p, fp.p, e.p, B, value_want.p, q1_want.p, r1_want.p, q2_want.p);
  CHECK(memcmp(value.p, value_want.p, B * N) == 0, "decrypt value, B=%ld pin=%d", (long)B, pin);
  if (witness) {
    CHECK(memcmp(q1.p, q1_want.p, B * N * 2) == 0 && memcmp(r1.p, r1_want.p, B * N * 2) == 0 && memcmp(q2.p, q2_want.p, B * N) == 0,
          "decrypt witness arrays, B=%ld", (long)B);
  }
}

static void per_item(ntru_engine_t *eng, int N, int q, int64_t B, bool pin) {
  const int p = 3;
  Buf<int8_t> f(B * N, pin), g(B * N, pin);
  Buf<uint16_t> fq(B * N, pin), h(B * N, pin), a(B * N, pin);
  Buf<uint8_t> fp(B * N, pin);
  for (int64_t i = 0; i < B * N; i++) { f.p[i] = (int8_t)((int)(rnd() % 3) - 1); g.p[i] = (int8_t)((int)(rnd() % 3) - 1); fq.p[i] = (uint16_t)(rnd() % q);
                                         h.p[i] = (uint16_t)(rnd() % q); a.p[i] = (uint16_t)(rnd() % q); fp.p[i] = (uint8_t)(rnd() % 3); }
  Buf<uint16_t> o1(B * N, pin), o2(B * N, pin), o5(B * N, pin), o6(B * N, pin), w1(B * N, false), w2(B * N, false), w5(B * N, false), w6(B * N, false);
  Buf<uint8_t> o3(B * N, pin), o4(B * N, pin), fl(B, pin), w3(B * N, false), w4(B * N, false), wf(B, false);
  OK(ntru_verify_keys_batch(eng, N, q, p, f.p, g.p, fq.p, fp.p, h.p, B, o1.p, o2.p, o3.p, o4.p, o5.p, o6.p, fl.p));
  fake_verify(N, q, p, f.p, g.p, fq.p, fp.p, h.p, B, w1.p, w2.p, w3.p, w4.p, w5.p, w6.p, wf.p);
  CHECK(!memcmp(o1.p, w1.p, B * N * 2) && !memcmp(o2.p, w2.p, B * N * 2) && !memcmp(o3.p, w3.p, B * N) && !memcmp(o4.p, w4.p, B * N) &&
        !memcmp(o5.p, w5.p, B * N * 2) && !memcmp(o6.p, w6.p, B * N * 2) && !memcmp(fl.p, wf.p, B), "verify_keys, B=%ld pin=%d", (long)B, pin);
  OK(ntru_polymul_split(eng, N, q, a.p, fq.p, B, o1.p, o2.p));
  fake_polymul(N, q, a.p, fq.p, B, w1.p, w2.p);
  CHECK(!memcmp(o1.p, w1.p, B * N * 2) && !memcmp(o2.p, w2.p, B * N * 2), "polymul_split, B=%ld", (long)B);
  OK(ntru_public_key_batch(eng, N, q, p, fq.p, g.p, B, o1.p));
  fake_public_key(N, q, p, fq.p, g.p, B, w1.p);
  CHECK(!memcmp(o1.p, w1.p, B * N * 2), "public_key, B=%ld", (long)B);
  OK(ntru_invert_key_batch(eng, N, q, p, f.p, B, o1.p, o3.p, fl.p));
  bool same = true;
  for (int64_t i = 0; i < B * N && same; i++) same = o1.p[i] == (uint16_t)((((f.p[i] + 3) & (q - 1)) * 5 + 1) & (q - 1)) && o3.p[i] == (uint8_t)((f.p[i] + 4) % p);
  for (int64_t b = 0; b < B && same; b++) same = fl.p[b] == (uint8_t)(f.p[b * N] & 1);
  CHECK(same, "invert_key (scratch buffer per slot), B=%ld", (long)B);
  OK(ntru_add_batch(eng, N, q, a.p, h.p, B, o1.p));
  same = true;
  for (int64_t i = 0; i < B * N && same; i++) same = o1.p[i] == (uint16_t)((a.p[i] + h.p[i]) % q);
  CHECK(same, "add_batch, B=%ld", (long)B);
  uint32_t key[8] = {9, 8, 7, 6, 5, 4, 3, 2};
  OK(ntru_sample_ternary(eng, N, 3, 3, 2, key, 1000, B, o3.p));
  same = true;
  for (int64_t b = 0; b < B && same; b++) for (int i = 0; i < N && same; i++) same = o3.p[b * N + i] == (uint8_t)((1000 + b) * 7 + i * 3 + 9 + 3 + 3 + 2);
  CHECK(same, "sample_ternary (item offsets across chunks), B=%ld", (long)B);
}

// The regular host forms that round_trip and per_item do not reach: per-item keys, byte messages, witness checks, split_by_I, pack and
// unpack.  Each goes through the same runner (one description per call, ntru_host.hip); optional outputs asked for or not.
template <class T>
static void fill(Buf<T> &b, uint32_t mod, int bias = 0) { for (size_t i = 0; i < b.n; i++) b.p[i] = (T)((int)(rnd() % mod) + bias); }
template <class T>
static bool same(const Buf<T> &a, const Buf<T> &b) { return memcmp(a.p, b.p, a.n * sizeof(T)) == 0; }

static void regular_forms(ntru_engine_t *eng, int N, int q, int64_t B, bool pin, bool opt) {
  const int p = 3, nbytes = N / 8;
  {   // per-item keys
    Buf<uint16_t> h(B * N, pin), e(B * N, pin), quot(B * N, pin), e_want(B * N, false), quot_want(B * N, false);
    Buf<uint8_t> r(B * N, pin), m(B * N, pin);
    fill(h, q); fill(r, 3); fill(m, 2);
    OK(ntru_encrypt_peritem_batch(eng, N, q, h.p, r.p, m.p, B, e.p, opt ? quot.p : nullptr));
    fake_encrypt_peritem(N, q, h.p, r.p, m.p, B, e_want.p, quot_want.p);
    CHECK(same(e, e_want) && (!opt || same(quot, quot_want)), "encrypt_peritem, B=%ld pin=%d opt=%d", (long)B, pin, opt);
    Buf<int8_t> f(B * N, pin);
    Buf<uint8_t> fp(B * N, pin), value(B * N, pin), q2(B * N, pin), value_want(B * N, false), q2_want(B * N, false);
    Buf<uint16_t> q1(B * N, pin), r1(B * N, pin), q1_want(B * N, false), r1_want(B * N, false);
    fill(f, 3, -1); fill(fp, 3);
    OK(ntru_decrypt_peritem_batch(eng, N, q, p, f.p, fp.p, e.p, B, value.p, opt ? q1.p : nullptr, opt ? r1.p : nullptr, opt ? q2.p : nullptr));
    fake_decrypt_peritem(N, q, p, f.p, fp.p, e.p, B, value_want.p, q1_want.p, r1_want.p, q2_want.p);
    CHECK(same(value, value_want) && (!opt || (same(q1, q1_want) && same(r1, r1_want) && same(q2, q2_want))), "decrypt_peritem, B=%ld pin=%d opt=%d",
          (long)B, pin, opt);
  }
  {   // byte messages
    Buf<uint8_t> bytes(B * nbytes, pin), m(B * N, pin), m_want(B * N, false), back(B * nbytes, pin), back_want(B * nbytes, false), fl(B, pin), fl_want(B, false);
    fill(bytes, 256);
    OK(ntru_bytes_to_rows(eng, N, nbytes, bytes.p, B, m.p));
    fake_bytes_to_rows(N, nbytes, bytes.p, B, m_want.p);
    CHECK(same(m, m_want), "bytes_to_rows, B=%ld pin=%d", (long)B, pin);
    OK(ntru_rows_to_bytes(eng, N, nbytes, m.p, B, back.p, opt ? fl.p : nullptr));
    fake_rows_to_bytes(N, nbytes, m.p, B, back_want.p, fl_want.p);
    CHECK(same(back, back_want) && (!opt || same(fl, fl_want)), "rows_to_bytes, B=%ld pin=%d opt=%d", (long)B, pin, opt);
    Buf<uint16_t> h(N, false), e(B * N, pin), quot(B * N, pin), e_want(B * N, false), quot_want(B * N, false);
    Buf<uint8_t> r(B * N, pin), fp(N, false);
    Buf<int8_t> f(N, false);
    fill(h, q); fill(r, 3); fill(f, 3, -1); fill(fp, 3);
    OK(ntru_encrypt_bytes_batch(eng, N, q, nbytes, h.p, r.p, bytes.p, B, e.p, opt ? quot.p : nullptr));
    fake_encrypt_bytes(N, q, nbytes, h.p, r.p, bytes.p, B, e_want.p, quot_want.p);
    CHECK(same(e, e_want) && (!opt || same(quot, quot_want)), "encrypt_bytes, B=%ld pin=%d opt=%d", (long)B, pin, opt);
    OK(ntru_decrypt_bytes_batch(eng, N, q, p, nbytes, f.p, fp.p, e.p, B, back.p, opt ? fl.p : nullptr));
    fake_decrypt_bytes(N, q, p, nbytes, f.p, fp.p, e.p, B, back_want.p, fl_want.p);
    CHECK(same(back, back_want) && (!opt || same(fl, fl_want)), "decrypt_bytes, B=%ld pin=%d opt=%d", (long)B, pin, opt);
  }
  if (opt) {   // witness checks (no optional arrays): three or two rows of N entries, four or two of N + 1
    Buf<uint16_t> a0(B * N, pin), a1(B * N, pin), a2(B * N, pin), b0(B * (N + 1), pin), b1(B * (N + 1), pin), b2(B * (N + 1), pin), b3(B * (N + 1), pin);
    Buf<uint8_t> fl(B, pin), fl_want(B, false);
    for (Buf<uint16_t> *x : {&a0, &a1, &a2, &b0, &b1, &b2, &b3}) fill(*x, q);
    const uint16_t *enc[] = {a0.p, a1.p, a2.p, b0.p, b1.p}, *dec[] = {a0.p, a1.p, a2.p, b0.p, b1.p, b2.p, b3.p}, *inv[] = {a0.p, a1.p, b0.p, b1.p};
    OK(ntru_check_encrypt_batch(eng, N, q, 11, a0.p, a1.p, a2.p, b0.p, b1.p, B, fl.p));
    fake_check(N, q + 11, enc, 3, 2, B, fl_want.p);
    CHECK(same(fl, fl_want), "check_encrypt, B=%ld pin=%d", (long)B, pin);
    OK(ntru_check_decrypt_batch(eng, N, q, 11, p, 2, a0.p, a1.p, a2.p, b0.p, b1.p, b2.p, b3.p, B, fl.p));
    fake_check(N, q + 11 + p + 2, dec, 3, 4, B, fl_want.p);
    CHECK(same(fl, fl_want), "check_decrypt, B=%ld pin=%d", (long)B, pin);
    OK(ntru_check_inverse_batch(eng, N, q, 11, a0.p, a1.p, b0.p, b1.p, B, fl.p));
    fake_check(N, q + 11, inv, 2, 2, B, fl_want.p);
    CHECK(same(fl, fl_want), "check_inverse, B=%ld pin=%d", (long)B, pin);
    CHECK(ntru_check_inverse_batch(eng, N, q, 11, a0.p, a1.p, b0.p, b1.p, -1, fl.p) != 0 && strstr(ntru_last_error(), "witness check: negative batch size"),
          "the witness checks' own batch-size message");
    // split_by_I: rows of 2 N in; pack: rows of os field elements out; unpack: row lengths from the bit width
    Buf<uint16_t> wide(B * 2 * N, pin), lo(B * N, pin), hi(B * N, pin);
    fill(wide, q);
    OK(ntru_split_by_I(eng, N, q, wide.p, B, lo.p, hi.p));
    bool ok = true;
    for (int64_t i = 0; i < B * N && ok; i++) ok = lo.p[i] == (uint16_t)((wide.p[2 * i] + 1) % q) && hi.p[i] == (uint16_t)((wide.p[2 * i + 1] + 2) % q);
    CHECK(ok, "split_by_I, B=%ld pin=%d", (long)B, pin);
    int bits, per, al, os;
    OK(ntru_pack_params(q - 1, N, &bits, &per, &al, &os));
    Buf<uint64_t> packed(B * os * 4, pin);
    OK(ntru_pack_batch(eng, q - 1, N, a0.p, B, packed.p));
    ok = true;
    for (int64_t b = 0; b < B && ok; b++) for (int j = 0; j < os * 4 && ok; j++) ok = packed.p[b * os * 4 + j] == (uint64_t)a0.p[b * N + j % N] * 0x10001ull + j;
    CHECK(ok, "pack_batch, B=%ld pin=%d", (long)B, pin);
    Buf<uint16_t> unpacked(B * os * per, pin);
    OK(ntru_unpack_batch(eng, q - 1, per * bits, packed.p, os, B, unpacked.p));
    ok = true;
    for (int64_t b = 0; b < B && ok; b++) for (int j = 0; j < os * per && ok; j++) ok = unpacked.p[b * os * per + j] == (uint16_t)(packed.p[(b * os + j / per) * 4] + j);
    CHECK(ok, "unpack_batch, B=%ld pin=%d", (long)B, pin);
    OK(ntru_unpack_batch(eng, q - 1, per * bits, nullptr, 0, B, nullptr));       // packed_size == 0: nothing to move
    OK(ntru_pack_batch(eng, q - 1, N, nullptr, 0, nullptr));
    CHECK(ntru_pack_batch(eng, q - 1, N, nullptr, B, packed.p) != 0 && strstr(ntru_last_error(), "ntru_pack_batch: NULL buffer"), "pack without data");
  }
}

// ntru_pipeline_batch: device-only intermediates (r, e), optional outputs, several chunks
static void pipeline(ntru_engine_t *eng, int N, int q, int64_t B, bool pin) {
  const int p = 3;
  Buf<uint16_t> h(N, false), e(B * N, pin), e_want(B * N, false);
  Buf<int8_t> f(N, false);
  Buf<uint8_t> fp(N, false), m(B * N, pin), r(B * N, false), value(B * N, pin), value_want(B * N, false), r_back(B * N, pin);
  for (int i = 0; i < N; i++) { h.p[i] = (uint16_t)(rnd() % q); f.p[i] = (int8_t)((int)(rnd() % 3) - 1); fp.p[i] = (uint8_t)(rnd() % 3); }
  for (int64_t i = 0; i < B * N; i++) m.p[i] = (uint8_t)(rnd() % 2);
  uint32_t key[8] = {5, 4, 3, 2, 1, 0, 9, 8};
  for (int64_t b = 0; b < B; b++) for (int i = 0; i < N; i++) r.p[b * N + i] = (uint8_t)((77 + b) * 7 + i * 3 + 5 + 4 + 4 + 2);   // what the fake sampler draws
  fake_encrypt(N, q, h.p, r.p, m.p, B, e_want.p, nullptr);
  std::vector<uint16_t> d1(B * N ? B * N : 1), d2(B * N ? B * N : 1);
  std::vector<uint8_t> d3(B * N ? B * N : 1);
  fake_decrypt(N, q, p, f.p, fp.p, e_want.p, B, value_want.p, d1.data(), d2.data(), d3.data());
  OK(ntru_pipeline_batch(eng, N, q, p, h.p, f.p, fp.p, key, 77, 4, 4, nullptr, m.p, B, r_back.p, e.p, value.p, nullptr));
  CHECK(!memcmp(r_back.p, r.p, B * N) && !memcmp(e.p, e_want.p, B * N * 2) && !memcmp(value.p, value_want.p, B * N), "pipeline r / e / value, B=%ld pin=%d", (long)B, pin);
  memset(value.p, 0xEE, B * N);
  OK(ntru_pipeline_batch(eng, N, q, p, h.p, f.p, fp.p, key, 77, 4, 4, nullptr, m.p, B, nullptr, nullptr, value.p, nullptr));   // only m up, only value down
  CHECK(!memcmp(value.p, value_want.p, B * N), "lean pipeline, B=%ld", (long)B);
  OK(ntru_pipeline_batch(eng, N, q, p, h.p, nullptr, nullptr, nullptr, 0, 0, 0, r.p, m.p, B, nullptr, e.p, nullptr, nullptr));   // encrypt only, r given
  CHECK(!memcmp(e.p, e_want.p, B * N * 2), "encrypt-only pipeline, B=%ld", (long)B);
  CHECK(ntru_pipeline_batch(eng, N, q, p, h.p, f.p, fp.p, key, 0, 4, 4, r.p, m.p, B, nullptr, e.p, nullptr, nullptr) != 0, "key AND r must be refused");
  CHECK(ntru_pipeline_batch(eng, N, q, p, h.p, nullptr, nullptr, key, 0, 4, 4, nullptr, m.p, B, nullptr, nullptr, value.p, nullptr) != 0, "value without f, fp must be refused");
}

static void two_streams_share_the_scratch(ntru_engine_t *eng, int N, int q) {
  hipStream_t sa, sb;
  hipStreamCreateWithFlags(&sa, 0); hipStreamCreateWithFlags(&sb, 0);
  const int64_t B = 300;
  std::vector<int8_t> f1(B * N), f2(B * N);
  std::vector<uint16_t> o1(B * N), o2(B * N);
  std::vector<uint8_t> p1(B * N), p2(B * N), l1(B), l2(B);
  for (auto &x : f1) x = (int8_t)((int)(rnd() % 3) - 1);
  for (auto &x : f2) x = (int8_t)((int)(rnd() % 3) - 1);
  OK(ntru_engine_set_stream(eng, sa));
  OK(ntru_invert_key_batch_dev(eng, N, q, 3, f1.data(), B, o1.data(), p1.data(), l1.data()));   // ("device" memory is the heap here)
  OK(ntru_engine_set_stream(eng, sb));
  OK(ntru_invert_key_batch_dev(eng, N, q, 3, f2.data(), B, o2.data(), p2.data(), l2.data()));   // must wait for stream a's use of the scratch
  hipStreamSynchronize(sa); hipStreamSynchronize(sb);
  bool same = true;
  for (int64_t i = 0; i < B * N && same; i++)
    same = o1[i] == (uint16_t)((((f1[i] + 3) & (q - 1)) * 5 + 1) & (q - 1)) && o2[i] == (uint16_t)((((f2[i] + 3) & (q - 1)) * 5 + 1) & (q - 1));
  CHECK(same, "two *_dev calls on two streams sharing the engine's scratch buffer");
  OK(ntru_engine_set_stream(eng, nullptr));
  hipStreamDestroy(sa); hipStreamDestroy(sb);
}

// eng->shared_dev through ResidentHold: one holder at a time; a second hold fails without growing (growing frees what the first
// holder still points at, which AddressSanitizer would see at the reads below).
static void resident_hold(ntru_engine_t *eng) {
  const size_t small = 1000, large = (size_t)3 << 20;
  {
    ResidentHold first(eng, "first_form", small);
    CHECK(first.rc == NTRU_OK && first.p != nullptr && first.p == (char *)eng->shared_dev.p, "a hold hands out the engine's buffer");
    if (first.rc != NTRU_OK) return;
    memset(first.p, 0x5A, small);
    const size_t cap = eng->shared_dev.cap;
    {
      ResidentHold second(eng, "second_form", large);
      CHECK(second.rc == NTRU_ERR_ARG && second.p == nullptr, "a second hold while one is live must be refused");
      CHECK(strstr(ntru_last_error(), "first_form") && strstr(ntru_last_error(), "second_form"), "the refusal names both holders: %s", ntru_last_error());
    }
    CHECK(eng->shared_dev.p == first.p && eng->shared_dev.cap == cap, "the refused hold did not grow the buffer");
    CHECK(eng->shared_holder && !strcmp(eng->shared_holder, "first_form"), "the refused hold left the first holder's mark");
    bool intact = true;
    for (size_t i = 0; i < small && intact; i++) intact = first.p[i] == 0x5A;
    CHECK(intact, "the first holder's bytes after the refused hold");
  }
  CHECK(eng->shared_holder == nullptr, "leaving scope releases the hold");
  ResidentHold third(eng, "third_form", large);
  CHECK(third.rc == NTRU_OK && third.p != nullptr && eng->shared_dev.cap >= large, "a larger hold after the first has left scope");
  if (third.rc == NTRU_OK) memset(third.p, 0, large);
}

// Carve against the offset chain scan_flow wrote by hand (one pass of 1000 packed rows, N = 61, 7 message bytes, 4 blocks), and
// ntru_ranges_overlap.
static void carve_and_overlap() {
  auto up = [](size_t v) { return (v + 255) / 256 * 256; };
  const size_t pass = 1000, N = 61, nbytes = 7, max_blocks = 4;
  const size_t at_value = up(pass * N * 2), at_bytes = at_value + up(pass * N), at_flags = at_bytes + up(pass * nbytes), at_counts = at_flags + up(pass),
               at_offsets = at_counts + up(max_blocks * 4), total = at_offsets + up(max_blocks * 8);
  Carve c;
  const size_t got[6] = {c.take(pass * N * 2), c.take(pass * N), c.take(pass * nbytes), c.take(pass), c.take(max_blocks * 4), c.take(max_blocks * 8)};
  const size_t want[6] = {0, at_value, at_bytes, at_flags, at_counts, at_offsets};
  for (int i = 0; i < 6; i++) CHECK(got[i] == want[i] && got[i] % 256 == 0, "Carve offset %d: %zu, by hand %zu", i, got[i], want[i]);
  CHECK(c.total == total && total % 256 == 0, "Carve total %zu, by hand %zu", c.total, total);
  Carve e;
  CHECK(e.take(0) == 0 && e.take(1) == 0 && e.take(256) == 256 && e.take(257) == 512 && e.total == 1024, "empty arrays take no room, every other one whole granules");
  char buf[64];
  CHECK(!ntru_ranges_overlap(buf, 16, buf + 16, 16) && !ntru_ranges_overlap(buf + 16, 16, buf, 16), "touching ranges do not overlap");
  CHECK(ntru_ranges_overlap(buf, 17, buf + 16, 16) && ntru_ranges_overlap(buf + 16, 16, buf, 17), "one shared byte overlaps");
  CHECK(ntru_ranges_overlap(buf, 64, buf + 8, 4) && ntru_ranges_overlap(buf + 8, 4, buf, 64) && ntru_ranges_overlap(buf, 8, buf, 8), "a range inside another, and a range and itself");
  CHECK(!ntru_ranges_overlap(buf + 8, 0, buf, 64) && !ntru_ranges_overlap(buf, 64, buf + 8, 0) && !ntru_ranges_overlap(buf, 0, buf, 0), "an empty range overlaps nothing");
  CHECK(!ntru_ranges_overlap(nullptr, 64, buf, 64) && !ntru_ranges_overlap(buf, 64, nullptr, 64) && !ntru_ranges_overlap(nullptr, 8, nullptr, 8), "NULL overlaps nothing");
}

static void multi(int N, int q) {
  const int ids[3] = {0, 1, 2};
  ntru_multi_t *mu = nullptr;
  OK(ntru_multi_create(ids, 3, &mu));
  CHECK(ntru_multi_engines(mu) == 3, "three engines");
  for (int64_t B : {(int64_t)2, (int64_t)1000, (int64_t)70001}) {       // 2 items on 3 engines: an empty shard
    std::vector<uint16_t> h(N), e(B * N), quot(B * N), ew(B * N), qw(B * N);
    std::vector<uint8_t> r(B * N), m(B * N);
    for (auto &x : h) x = (uint16_t)(rnd() % q);
    for (int64_t i = 0; i < B * N; i++) { r[i] = (uint8_t)(rnd() % 3); m[i] = (uint8_t)(rnd() % 2); }
    OK(ntru_multi_encrypt_batch(mu, N, q, h.data(), r.data(), m.data(), B, e.data(), quot.data()));
    fake_encrypt(N, q, h.data(), r.data(), m.data(), B, ew.data(), qw.data());
    CHECK(e == ew && quot == qw, "multi encrypt, B=%ld", (long)B);
    std::vector<int8_t> f(N);
    std::vector<uint8_t> fp(N), v(B * N), vw(B * N);
    for (int i = 0; i < N; i++) { f[i] = (int8_t)((int)(rnd() % 3) - 1); fp[i] = (uint8_t)(rnd() % 3); }
    OK(ntru_multi_decrypt_batch(mu, N, q, 3, f.data(), fp.data(), e.data(), B, v.data(), nullptr, nullptr, nullptr));
    std::vector<uint16_t> d1(B * N), d2(B * N);
    std::vector<uint8_t> d3(B * N);
    fake_decrypt(N, q, 3, f.data(), fp.data(), e.data(), B, vw.data(), d1.data(), d2.data(), d3.data());
    CHECK(v == vw, "multi decrypt (value only), B=%ld", (long)B);
    if (B > 1000) continue;
    // the per-item calls: every array moves with its shard, flags by one byte per item
    std::vector<int8_t> fi(B * N), g(B * N);
    std::vector<uint16_t> fq(B * N), hh(B * N), o1(B * N), o2(B * N), o5(B * N), o6(B * N), w1(B * N), w2(B * N), w5(B * N), w6(B * N);
    std::vector<uint8_t> fpi(B * N), o3(B * N), o4(B * N), fl(B), w3(B * N), w4(B * N), wf(B);
    for (int64_t i = 0; i < B * N; i++) { fi[i] = (int8_t)((int)(rnd() % 3) - 1); g[i] = (int8_t)((int)(rnd() % 3) - 1); fq[i] = (uint16_t)(rnd() % q);
                                           hh[i] = (uint16_t)(rnd() % q); fpi[i] = (uint8_t)(rnd() % 3); }
    OK(ntru_multi_verify_keys_batch(mu, N, q, 3, fi.data(), g.data(), fq.data(), fpi.data(), hh.data(), B, o1.data(), o2.data(), o3.data(), o4.data(),
                                    o5.data(), o6.data(), fl.data()));
    fake_verify(N, q, 3, fi.data(), g.data(), fq.data(), fpi.data(), hh.data(), B, w1.data(), w2.data(), w3.data(), w4.data(), w5.data(), w6.data(), wf.data());
    CHECK(o1 == w1 && o2 == w2 && o3 == w3 && o4 == w4 && o5 == w5 && o6 == w6 && fl == wf, "multi verify_keys, B=%ld", (long)B);
    OK(ntru_multi_polymul_split(mu, N, q, fq.data(), hh.data(), B, o1.data(), o2.data()));
    fake_polymul(N, q, fq.data(), hh.data(), B, w1.data(), w2.data());
    CHECK(o1 == w1 && o2 == w2, "multi polymul_split, B=%ld", (long)B);
    OK(ntru_multi_public_key_batch(mu, N, q, 3, fq.data(), g.data(), B, o1.data()));
    fake_public_key(N, q, 3, fq.data(), g.data(), B, w1.data());
    CHECK(o1 == w1, "multi public_key, B=%ld", (long)B);
    OK(ntru_multi_invert_key_batch(mu, N, q, 3, fi.data(), B, nullptr, o3.data(), fl.data()));       // fp only
    bool same_fp = true;
    for (int64_t i = 0; i < B * N && same_fp; i++) same_fp = o3[i] == (uint8_t)((fi[i] + 4) % 3);
    for (int64_t b = 0; b < B && same_fp; b++) same_fp = fl[b] == (uint8_t)(fi[b * N] & 1);
    CHECK(same_fp, "multi invert_key (fp only), B=%ld", (long)B);
    CHECK(ntru_multi_invert_key_batch(mu, N, q, 3, fi.data(), B, nullptr, nullptr, fl.data()) != 0 &&
          strstr(ntru_last_error(), "device shard 0: ntru_invert_key_batch: NULL buffer"), "multi invert_key without fq and fp");
    CHECK(ntru_multi_public_key_batch(mu, N, q, 3, fq.data(), nullptr, B, o1.data()) != 0 &&
          strstr(ntru_last_error(), "ntru_multi_public_key_batch: NULL buffer"), "the multi forms' own NULL check");
  }
  ntru_multi_destroy(mu);
}

int main() {
  CHECK(ntru_engine_device_count() == 4, "fake device count");
  ntru_engine_t *eng = nullptr;
  OK(ntru_engine_create(0, &eng));
  ntru_engine_t *e2 = nullptr;
  CHECK(ntru_engine_create(9, &e2) != 0 && e2 == nullptr && strlen(ntru_last_error()) > 0, "device id out of range must fail with a message");
  OK(ntru_engine_create(1, &e2));
  CHECK(ntru_engine_set_kernel_path(eng, 77) != 0, "bad kernel path must be refused");
  {   // the occupancy query is corrected for the 1280-byte pieces LDS is handed out in (profiles/r03_wg_residency.txt)
    struct { int threads; size_t lds; int want; } cases[] = {{64, 13312, 11}, {64, 12800, 12}, {64, 12801, 11}, {64, 10241, 14},
                                                             {256, 81920, 2}, {256, 81921, 1}, {256, 0, 2}, {64, 5121, 25}};
    for (auto &c : cases) {
      int n = 0;
      OK(ntru_blocks_per_cu(eng, (const void *)&cases, c.threads, c.lds, &n));
      CHECK(n == c.want, "workgroups per CU after the LDS-piece correction");
    }
  }
  const int N = 61, q = 2048;
  for (bool pin : {false, true})
    for (int64_t B : {(int64_t)0, (int64_t)1, (int64_t)1000, (int64_t)(1 << 15) + 7, (int64_t)3 * (1 << 15) + 5}) {
      round_trip(eng, N, q, B, pin, true);
#ifndef HOSTCHECK_QUICK                                      // (the ThreadSanitizer build runs ~20x slower: fewer repetitions, same paths)
      round_trip(eng, N, q, B, pin, false);
#endif
    }
  for (bool pin : {false, true})
#ifdef HOSTCHECK_QUICK
    for (int64_t B : {(int64_t)1, (int64_t)(1 << 15) + 9}) per_item(eng, N, q, B, pin);
#else
    for (int64_t B : {(int64_t)1, (int64_t)(1 << 15) + 9, (int64_t)2 * (1 << 15) + 1}) per_item(eng, N, q, B, pin);
#endif
  round_trip(eng, N, q, 1000, false, false);
  // B = 1, one chunk, four even chunks, four chunks with a ragged last one (8197 = 3 * 2050 + 2047)
  for (bool pin : {false, true})
#ifdef HOSTCHECK_QUICK
    for (int64_t B : {(int64_t)1, (int64_t)8197}) regular_forms(eng, N, q, B, pin, B == 1 ? !pin : pin);
#else
    for (int64_t B : {(int64_t)1, (int64_t)1000, (int64_t)8200, (int64_t)8197})
      for (bool opt : {true, false}) regular_forms(eng, N, q, B, pin, opt);
#endif
  for (bool pin : {false, true})
    for (int64_t B : {(int64_t)1, (int64_t)9001, (int64_t)4 * (1 << 15) + 3}) pipeline(eng, N, q, B, pin);
  {   // plain device buffers
    void *d = nullptr;
    OK(ntru_dev_alloc(eng, 4096, &d));
    std::vector<uint8_t> a(4096), b(4096);
    for (auto &x : a) x = (uint8_t)rnd();
    OK(ntru_dev_upload(eng, d, a.data(), a.size()));
    OK(ntru_dev_download(eng, b.data(), d, b.size()));
    CHECK(a == b, "dev_upload / dev_download");
    OK(ntru_dev_free(eng, d));
  }
  two_streams_share_the_scratch(eng, N, q);
  resident_hold(eng);
  carve_and_overlap();
  {   // two engines from two host threads at once (thread-local error strings, nothing shared between engines)
    std::thread t1([&] { round_trip(eng, N, q, (1 << 15) + 11, false, true); });
    std::thread t2([&] { round_trip(e2, N, q, (1 << 15) + 13, true, true); });
    t1.join(); t2.join();
  }
  multi(N, q);
  CHECK(ntru_encrypt_batch(eng, N, 1000, nullptr, nullptr, nullptr, 4, nullptr, nullptr) != 0, "q that is no power of two must be refused");
  ntru_engine_destroy(e2);
  ntru_engine_destroy(eng);
  if (g_fail) { fprintf(stderr, "hostcheck: %d failure(s)\n", g_fail); return 1; }
  printf("hostcheck ok (%d checks)\n", g_checks.load());
  return 0;
}
