// valu_families.hip -- MI355X (gfx950): the vector-ALU kernel families 1-3 of the NTRU polynomial-ring engine ("one ciphertext per
// wavefront", the decomposition BASELINE.json's north_star describes) and the host functions that launch them.
//
// Hot path of numtel/ntru-circom re-designed for CDNA4 (reference: index.js):
//   multiplyPolynomials (index.js:319-355)  -> exact integer schoolbook in Z/2^16 (q | 2^16, so natural u16
//                                              wrap-around IS the mod-q residue; mod-p sums stay < 2^16)
//   dividePolynomials by I=1-x^N (:358-401) -> closed form fused into the product's epilogue
//   addPolynomials (:235-244), lift (:117)  -> fused into the same epilogue
//
// Work decomposition ("one ciphertext per wavefront"):
//   * an item (one polynomial product) is owned by nl = ceil(N / 2K) consecutive lanes of a wave; lane s owns
//     the 2K outputs k in [2K s, 2K s + 2K) as K packed u16 pairs (v_pk_mad_u16: 2 MACs per lane-instruction).
//     For small N several items share a wave (G = 64 / nl).
//   * the "window" operand b lives in LDS as EO[u] = { E[u] = (bc[2u], bc[2u+1]), O[u] = (bc[2u-1], bc[2u]) },
//     bc = b extended cyclically with period N, so that for step i the K pairs a lane needs are K consecutive
//     8-byte entries, and going from step i to i+2 slides that window by exactly one entry: one ds_read_b64 per
//     lane per two steps, lane stride K entries (K odd => conflict-free, profiles/archive/r01_microbench_valu_lds.txt).
//   * the "broadcast" operand a is read from LDS two coefficients at a time and applied with op_sel splats.
//   * T[k] = sum_i a[i] bc[k-i] is the cyclic product = remainder; the low half c[k] of the LINEAR product (needed
//     for the quotient) is T's value just before the lane's own block of i plus an in-block
//     triangle; high = T - low; quotient = -high.  (tools/lane_model.py is the executable spec of this indexing.)
//
// Layout of the file: operand functors and staging; then what the families share, each stated once (window policies, triangle,
// finish_pair, lift_pair, lane bookkeeping, the verifyKeysInputs flag helpers, the per-item-window LDS layout); the MAC family (1);
// the ternary-stepping "add path" families (2: per-item stepping, 3: shared-key stepping, with the dot8 second product); the
// launchers.  Two store forms stay: the MAC kernels' per-element predicates (store_pairs) and the add path's whole-block / tail
// plan (StorePlan); the second in the MAC kernels costs a fifth more instructions and an occupancy step (EXPERIMENTS.md).
//
// No CPU fallback exists in this file: every entry point needs a HIP device.
#include "kernels_common.h"

struct Geom {
  int N;       // ring size
  int nl;      // lanes per item = ceil(N / 2K)
  int G;       // items per wave = 64 / nl
  int off;     // K*nl: position of logical entry u = 0 inside an EO array
  int eo_len;  // 2*K*nl 8-byte entries per EO array
  int a_len;   // K*nl dwords (2K*nl u16) per staged a-operand
};

// ---- operand value functors: coefficient j of an operand, already mapped into its u16 representation ----------
struct ValU16 {            // e, h, fq, generic a/b
  const u16 *p;
  __device__ __forceinline__ u32 operator()(int j) const { return p[j]; }
};
struct ValU16x3 {          // fqp = p*fq left unreduced (index.js:155); 3*8191 < 2^16
  const u16 *p; u32 mul;
  __device__ __forceinline__ u32 operator()(int j) const { return (u32)p[j] * mul; }
};
struct ValU16x3m {         // (p*fq) mod q: the same window reduced, for the add path's 16-bit field budget
  const u16 *p; u32 mul, mask;
  __device__ __forceinline__ u32 operator()(int j) const { return ((u32)p[j] * mul) & mask; }
};
struct ValU8 {             // r, fp, m
  const uint8_t *p;
  __device__ __forceinline__ u32 operator()(int j) const { return p[j]; }
};
struct ValTernary {        // f, g in {-1,0,1}: -1 -> mod-1 (index.js:112,151,152,156)
  const int8_t *p; u32 neg;
  __device__ __forceinline__ u32 operator()(int j) const { int v = p[j]; return v < 0 ? neg : (u32)v; }
};

struct ValLds {            // an operand staged as u16 in LDS (per-item windows: coalesced global loads first)
  const u16 *p;
  __device__ __forceinline__ u32 operator()(int j) const { return p[j]; }
};

// Coefficients k, k + 1 of an operand row as a packed u16 pair, zero beyond N.  CLAMP: every lane loads, from a clamped index (no
// branch, but an address of its own per element); otherwise only lanes inside the row load (one address per lane, immediate offsets).
template <bool CLAMP = true, class F>
static __device__ __forceinline__ u32 pair_at(F val, int k, int N) {
  const int k0 = !CLAMP || k < N ? k : N - 1, k1 = !CLAMP || k + 1 < N ? k + 1 : N - 1;
  const u32 v0 = k < N ? (val(k0) & 0xFFFFu) : 0u, v1 = k + 1 < N ? (val(k1) & 0xFFFFu) : 0u;
  return v0 | (v1 << 16);
}

// Stage N coefficients of a per-item operand into LDS as u16 (lane `sub` of the item's `nl` lanes; coalesced).
template <class F>
static __device__ __forceinline__ void stage_raw(u16 *raw, int N, int nl, F val, int sub, bool active) {
  if (!active) return;
  for (int i = sub; i < N; i += nl) raw[i] = (u16)val(i);
}

// Build one EO array (see header) from `val`; executed by `nthr` cooperating threads, this one being `tid`.
template <class F>
static __device__ __forceinline__ void build_eo(uint2 *eo, const Geom &g, F val, int tid, int nthr) {
  const int N = g.N;
  for (int x = tid; x < g.eo_len; x += nthr) {
    int j = 2 * (x - g.off);                 // |j| < 2*off <= N + 2K <= 2N
    j += j < 0 ? N : 0; j += j < 0 ? N : 0;
    j -= j >= N ? N : 0; j -= j >= N ? N : 0;
    int jm = j == 0 ? N - 1 : j - 1;
    int jp = j + 1 == N ? 0 : j + 1;
    u32 c0 = val(j) & 0xFFFFu, cm = val(jm) & 0xFFFFu, cp = val(jp) & 0xFFFFu;
    eo[x] = make_uint2(c0 | (cp << 16), cm | (c0 << 16));
  }
}

// Stage the broadcast operand as zero-padded u16s: a16[i] = i < N ? val(i) : 0 for i < 2*a_len.
template <class F>
static __device__ __forceinline__ void stage_a(u16 *a16, const Geom &g, F val, int sub, bool active) {
  if (!active) return;
  const int n2 = 2 * g.a_len;
  for (int i = sub; i < n2; i += g.nl) a16[i] = i < g.N ? (u16)val(i) : (u16)0;
}

// ---- what the families share: window policies, triangle, finish, lift, stores, lane bookkeeping, key flags ----------------------
static __device__ __forceinline__ u32 odd_pair(u32 e_u, u32 e_um1) { return __builtin_amdgcn_alignbit(e_u, e_um1, 16); }

// The two window layouts and, for the add path (described further down), the two ways of holding step bits.  The MAC kernels
// read PerItemWin's entries; per-item stepping (k_encrypt_t, k_decrypt_t, k_verify_keys_t) uses all of PerItemWin, shared-key
// stepping (k_decrypt_s, described at build_cyclic_pairs below) all of SharedWin.  Everything in which they differ is stated here:
//   1. window (Entry, even, odd, extra, stored_odd): LDS entries {E[u], O[u]} -- against entries E[u] alone with
//      O[u] = odd_pair(E[u], E[u-1]), so that the refill of one block needs K + 1 next-window entries, not K.
//   2. step bits (Code, bit2, put, hold, fetch): one code dword per block, step j tests its bits j and 16+j -- against two
//      mask words per block (x: "into S1", y: "into S2") that each use bit j.  The block loop holds the current block's
//      Code and looks one block ahead; each family keeps its own order of loads and readfirstlanes: the dword is made
//      scalar when it becomes the held one -- against the held uint2 staying in VGPRs until its block begins.
//   3. remainder (masks_rem): a power-of-two remainder is left to the caller, who adds to it first and then masks --
//      against masked in the finish.  (Small moduli are reduced exactly in both.)
struct PerItemWin {
  using Entry = uint2;
  using Code = u32;
  static constexpr int extra = 0;                       // next-window entries a block pre-loads beyond K
  static constexpr bool stored_odd = true;              // O[0] = (b[-1], b[0]) is stored: the linear product cuts b[-1]
  static constexpr bool masks_rem = false;
  static constexpr bool clamps_loads = true;            // of a block of the stepping operand (pair_at): loaded per item, in every lane
  static constexpr int bit2(int J) { return 16 + J; }
  static __device__ __forceinline__ u32 even(Entry v) { return v.x; }
  static __device__ __forceinline__ u32 odd(Entry v, Entry before) { return v.y; }
  static __device__ __forceinline__ void put(Code &c, u32 is1, u32 is2, int j) { c |= (is1 << j) | (is2 << (16 + j)); }
  static __device__ __forceinline__ Code hold(Code c) { return __builtin_amdgcn_readfirstlane(c); }
  // the held block's two step words, and the look-ahead load of block m + 1's Code (clamped at the last block)
  static __device__ __forceinline__ Code fetch(const Code *codes, int m, int nblk, Code held, u32 &w1, u32 &w2) {
    w1 = held; w2 = held;
    return codes[m + 1 < nblk ? m + 1 : m];
  }
};
struct SharedWin {
  using Entry = u32;
  using Code = uint2;
  static constexpr int extra = 1;
  static constexpr bool stored_odd = false;             // derived from the entry before; none before index 0
  static constexpr bool masks_rem = true;
  static constexpr bool clamps_loads = false;           // loaded once per workgroup
  static constexpr int bit2(int J) { return J; }
  static __device__ __forceinline__ u32 even(Entry v) { return v; }
  static __device__ __forceinline__ u32 odd(Entry v, Entry before) { return odd_pair(v, before); }
  static __device__ __forceinline__ void put(Code &c, u32 is1, u32 is2, int j) { c.x |= is1 << j; c.y |= is2 << j; }
  static __device__ __forceinline__ Code hold(Code c) { return c; }
  static __device__ __forceinline__ Code fetch(const Code *codes, int m, int nblk, Code held, u32 &w1, u32 &w2) {
    w1 = __builtin_amdgcn_readfirstlane(held.x); w2 = __builtin_amdgcn_readfirstlane(held.y);
    return codes[m + 1 < nblk ? m + 1 : m];
  }
};

// In-block triangle of the LINEAR product: low[t] += the pairs of sum_{u<=j} a[k0+u] * b[j-u], j = 2t, 2t+1, for the lane's own
// 2K outputs (k0 = 2K*sub).  win: the item's window array, av(s): the lane's s-th pair of a.  No coefficient exists before b[0].
template <class Win, int K, class AV>
static __device__ __forceinline__ void triangle(const typename Win::Entry *win, const Geom &g, AV av, u16x2 (&low)[K]) {
  u32 ZE[K], ZO[K];
  typename Win::Entry prev = {};
#pragma unroll
  for (int x = 0; x < K; x++) {
    const typename Win::Entry v = win[g.off + x];
    ZE[x] = Win::even(v); ZO[x] = Win::odd(v, prev); prev = v;
  }
  if constexpr (Win::stored_odd) ZO[0] &= 0xFFFF0000u;
#pragma unroll
  for (int s = 0; s < K; s++) {
    const u16x2 ap = as_pair(av(s));
#pragma unroll
    for (int t = s; t < K; t++) {
      low[t] = ap.xx * as_pair(ZE[t - s]) + low[t];
      low[t] = ap.yy * as_pair(ZO[t - s]) + low[t];
    }
  }
}

// The finish of one output pair.  T: the cyclic product = remainder, low: the low half of the linear product, so high = T - low:
//   rem = T mod `mod`      quot = (-high) mod `mod`  (0 if not wanted)
// POW2: mod is a power of two (mask arithmetic on the wrapped u16 sums); otherwise sums are exact and `mod` small.
// MASK_REM: whether a power-of-two remainder is masked here or left to a caller that adds to it first.
template <bool POW2, bool MASK_REM>
static __device__ __forceinline__ void finish_pair(u16x2 T, u16x2 low, bool want_quot, u32 mod, u16x2 &rem, u16x2 &quot) {
  quot = (u16x2){0, 0};
  if (want_quot) {
    const u16x2 hi = T - low;
    if (POW2) {
      quot = ((u16x2){0, 0} - hi) & (u16)(mod - 1);
    } else {
      const u32 h0 = mod_small(hi.x, mod), h1 = mod_small(hi.y, mod);
      quot = (u16x2){(u16)(h0 ? mod - h0 : 0), (u16)(h1 ? mod - h1 : 0)};
    }
  }
  rem = POW2 ? (MASK_REM ? (T & (u16)(mod - 1)) : T) : (u16x2){(u16)mod_small(T.x, mod), (u16)mod_small(T.y, mod)};
}

// The centred lift of the finished pair at outputs k, k + 1 as a packed pair of the next product's operand; zero beyond N so that
// the padding stays zero.
static __device__ __forceinline__ u32 lift_pair(u16x2 rv, int k, int N, u32 q, u32 p, u32 add) {
  const u32 b0 = lift_value(rv.x, q, p, add), b1 = lift_value(rv.y, q, p, add);    // unconditional: no branch around the division
  return (k < N ? b0 : 0u) | ((k + 1 < N ? b1 : 0u) << 16);
}

// ---- MAC family (1) ---------------------------------------------------------------------------------------------------------------
// The O(N^2) accumulate.  eo: this item's EO array, a32: its staged a-operand (packed pairs), sub: lane's index in item.
template <int K>
static __device__ __forceinline__ void mac_core(const uint2 *__restrict__ eo, const u32 *__restrict__ a32,
                                                const Geom &g, int sub, bool want_low,
                                                u16x2 (&T)[K], u16x2 (&low)[K]) {
  u32 WE[K], WO[K];
  const uint2 *nb = eo + (K * sub + g.off);     // logical entry K*sub - K*m, m = 0
#pragma unroll
  for (int x = 0; x < K; x++) { uint2 v = nb[x]; WE[x] = v.x; WO[x] = v.y; }
#pragma unroll
  for (int t = 0; t < K; t++) { T[t] = (u16x2){0, 0}; low[t] = (u16x2){0, 0}; }
  const int nblk = g.nl;
  for (int m = 0; m < nblk; m++) {
    if (want_low && m == sub) {                 // snapshot: everything accumulated so far has i < 2K*sub <= k
#pragma unroll
      for (int t = 0; t < K; t++) low[t] = T[t];
    }
    uint2 nw[K]; u32 av[K];
#pragma unroll
    for (int s = 0; s < K; s++) nw[s] = nb[-1 - s];
#pragma unroll
    for (int s = 0; s < K; s++) av[s] = a32[K * m + s];
#pragma unroll
    for (int s = 0; s < K; s++) {
      const u16x2 ap = as_pair(av[s]);
#pragma unroll
      for (int t = 0; t < K; t++) T[t] = ap.xx * as_pair(WE[(t - s + K) % K]) + T[t];   // i = 2(Km+s)
#pragma unroll
      for (int t = 0; t < K; t++) T[t] = ap.yy * as_pair(WO[(t - s + K) % K]) + T[t];   // i + 1
      WE[K - 1 - s] = nw[s].x; WO[K - 1 - s] = nw[s].y;
    }
    nb -= K;
  }
}

// One product a*b with split by 1-x^N, results left in registers as K pairs per lane; the remainder of a power of two is left
// unmasked for a caller that adds to it first (finish_pair).
template <int K, bool POW2>
static __device__ __forceinline__ void product_split(const uint2 *eo, const u32 *a32, const Geom &g, int sub,
                                                     bool want_quot, u32 mod, u16x2 (&rem)[K], u16x2 (&quot)[K]) {
  u16x2 T[K], low[K];
  mac_core<K>(eo, a32, g, sub, want_quot, T, low);
  if (want_quot) triangle<PerItemWin, K>(eo, g, [&](int s) { return a32[K * sub + s]; }, low);
#pragma unroll
  for (int t = 0; t < K; t++) finish_pair<POW2, false>(T[t], low[t], want_quot, mod, rem[t], quot[t]);
}

// Store the lane's K output pairs into its item's row, element by element inside the row.
template <int K, class OutT>
static __device__ __forceinline__ void store_pairs(OutT *row, const Geom &g, int sub, const u16x2 (&v)[K]) {
#pragma unroll
  for (int t = 0; t < K; t++) {
    int k = 2 * K * sub + 2 * t;
    if (k < g.N) row[k] = (OutT)v[t].x;
    if (k + 1 < g.N) row[k + 1] = (OutT)v[t].y;
  }
}

struct LaneId {
  int wave, lane, grp, sub; bool active;
};
static __device__ __forceinline__ LaneId lane_id(const Geom &g) {
  LaneId L;
  L.wave = threadIdx.x >> 6;     // (readfirstlane here saves 5 VGPRs in k_encrypt_t but measured 11% slower)
  L.lane = threadIdx.x & 63;
  L.active = L.lane < g.G * g.nl;
  L.grp = L.active ? L.lane / g.nl : 0;
  L.sub = L.active ? L.lane - L.grp * g.nl : 0;
  return L;
}

// This lane's item's part of a wave-wide ballot of `pred` (items occupy nl consecutive lanes of the wave).
static __device__ __forceinline__ unsigned long long item_ballot(bool pred, const Geom &g, const LaneId &L) {
  const unsigned long long msk = (g.nl >= 64 ? ~0ull : ((1ull << g.nl) - 1)) << (L.grp * g.nl);
  return __ballot(pred && L.active) & msk;
}
// Does any active lane of this lane's item have `pred` set?
static __device__ __forceinline__ bool item_any(bool pred, const Geom &g, const LaneId &L) { return item_ballot(pred, g, L) != 0; }

// verifyKeysInputs' inverse check (index.js:159,162) on a remainder that arrives pair by pair: invalid iff
// "length != 1 && [0] != 1".
template <int K>
struct InverseCheck {
  bool nz_hi = false, first_not_one = false;          // some coefficient beyond index 0 is non-zero; coefficient 0 is not 1
  __device__ __forceinline__ void note(int sub, int t, int N, u16x2 rv) {
    const int k = 2 * K * sub + 2 * t;
    nz_hi |= (k >= 1 && k < N && rv.x != 0) || (k + 1 < N && rv.y != 0);
    if (t == 0) first_not_one = sub == 0 && rv.x != 1;
  }
  __device__ __forceinline__ bool invalid(const Geom &g, const LaneId &L) const {
    return item_any(nz_hi, g, L) && item_any(first_not_one, g, L);
  }
};
// 'invalid h' iff some index below h's TRIMMED length differs from the remainder (index.js:165).  hp: h's pair at outputs k, k + 1
// (pair_at: zero beyond N).  Each lane notes its highest non-zero index (-1: none); over the item's lanes the highest lane that
// holds one wins, and the zero polynomial has length 1.
static __device__ __forceinline__ void note_top(int &top, int k, u32 hp) {
  if (hp & 0xFFFFu) top = k;
  if (hp >> 16) top = k + 1;
}
static __device__ __forceinline__ int item_trimmed_len(int top, const Geom &g, const LaneId &L) {
  const unsigned long long bal = item_ballot(top >= 0, g, L);
  const int src = bal ? 63 - __builtin_clzll(bal) : (int)L.lane;
  const int top_src = __shfl(top, src);
  return bal ? top_src + 1 : 1;
}
static __device__ __forceinline__ bool differs_below(int hl, int k, u32 hp, u16x2 rv) {
  return (k < hl && (hp & 0xFFFFu) != rv.x) || (k + 1 < hl && (hp >> 16) != rv.y);
}

// The per-wave LDS region of the kernels whose window belongs to the item (k_polymul_split, k_verify_keys): G EO arrays, G staged
// a-operands, G raw u16 rows.  Byte offsets inside the region and its size; the launcher sizes what the kernels carve up.
struct PerItemLds { size_t a32, raw, raw_len, per_wave; };     // the EO arrays sit at offset 0; raw_len in u16 slots
static __host__ __device__ __forceinline__ PerItemLds per_item_lds(const Geom &g) {
  PerItemLds l;
  l.raw_len = ((size_t)g.N + 1) & ~(size_t)1;                  // dword aligned
  l.a32 = (size_t)g.G * g.eo_len * 8;
  l.raw = l.a32 + (size_t)g.G * g.a_len * 4;
  l.per_wave = l.raw + (size_t)g.G * l.raw_len * 2;
  return l;
}
struct PerItemBufs { uint2 *eo; u32 *a32; u16 *raw; };         // this lane's item's three arrays
static __device__ __forceinline__ PerItemBufs per_item_bufs(unsigned char *lds, const Geom &g, const LaneId &L) {
  const PerItemLds l = per_item_lds(g);
  unsigned char *wbase = lds + (size_t)L.wave * l.per_wave;
  return {(uint2 *)wbase + (size_t)L.grp * g.eo_len, (u32 *)(wbase + l.a32) + (size_t)L.grp * g.a_len,
          (u16 *)(wbase + l.raw) + (size_t)L.grp * l.raw_len};
}

// ---- kernels ------------------------------------------------------------------------------------------------
// dynamic LDS: [shared EO arrays][per-wave regions]; per-wave = G a-operands (+ G EO arrays for per-item windows)

// encryptBits, index.js:87-110: e = (m + r*h) mod q split by I.
template <int K>
__global__ __launch_bounds__(BLOCK_THREADS) void k_encrypt(Geom g, u32 q, const u16 *__restrict__ h,
                                                           const uint8_t *__restrict__ r,
                                                           const uint8_t *__restrict__ m, long B,
                                                           u16 *__restrict__ e, u16 *__restrict__ quotE) {
  extern __shared__ __attribute__((aligned(16))) unsigned char lds[];
  uint2 *eo_h = (uint2 *)lds;
  const LaneId L = lane_id(g);
  u32 *a_wave = (u32 *)(lds + (size_t)g.eo_len * 8) + (size_t)L.wave * g.G * g.a_len;
  u32 *a32 = a_wave + (size_t)L.grp * g.a_len;
  build_eo(eo_h, g, ValU16{h}, threadIdx.x, BLOCK_THREADS);
  __syncthreads();
  const long ngroups = (B + g.G - 1) / g.G;
  const bool want_quot = quotE != nullptr;
  for (long grp = (long)blockIdx.x * WAVES_PER_BLOCK + L.wave; grp < ngroups; grp += (long)gridDim.x * WAVES_PER_BLOCK) {
    const long item = grp * g.G + L.grp;
    const bool valid = L.active && item < B;
    const long row = (valid ? item : 0) * g.N;
    stage_a((u16 *)a32, g, ValU8{r + row}, L.sub, L.active);
    wave_lds_fence();
    u16x2 rem[K], quot[K];
    product_split<K, true>(eo_h, a32, g, L.sub, want_quot, q, rem, quot);
#pragma unroll
    for (int t = 0; t < K; t++) {
      int k = 2 * K * L.sub + 2 * t;
      u16x2 add = {(u16)(k < g.N ? m[row + k] : 0), (u16)(k + 1 < g.N ? m[row + k + 1] : 0)};
      rem[t] = (rem[t] + add) & (u16)(q - 1);
    }
    if (valid) {
      store_pairs<K>(e + row, g, L.sub, rem);
      if (want_quot) store_pairs<K>(quotE + row, g, L.sub, quot);
    }
    wave_lds_fence();
  }
}

// decryptBits, index.js:111-140: a = f*e mod q; split; lift; c = fp*b mod p; split.
template <int K>
__global__ __launch_bounds__(BLOCK_THREADS) void k_decrypt(Geom g, u32 q, u32 p, u32 lift_add, const int8_t *__restrict__ f,
                                                           const uint8_t *__restrict__ fp,
                                                           const u16 *__restrict__ e, long B,
                                                           uint8_t *__restrict__ value, u16 *__restrict__ quot1,
                                                           u16 *__restrict__ rem1, uint8_t *__restrict__ quot2) {
  extern __shared__ __attribute__((aligned(16))) unsigned char lds[];
  uint2 *eo_f = (uint2 *)lds;
  uint2 *eo_fp = eo_f + g.eo_len;
  const LaneId L = lane_id(g);
  u32 *a_wave = (u32 *)(lds + (size_t)g.eo_len * 16) + (size_t)L.wave * g.G * g.a_len;
  u32 *a32 = a_wave + (size_t)L.grp * g.a_len;
  build_eo(eo_f, g, ValTernary{f, q - 1}, threadIdx.x, BLOCK_THREADS);
  build_eo(eo_fp, g, ValU8{fp}, threadIdx.x, BLOCK_THREADS);
  __syncthreads();
  const long ngroups = (B + g.G - 1) / g.G;
  const bool want_q1 = quot1 != nullptr, want_q2 = quot2 != nullptr;
  for (long grp = (long)blockIdx.x * WAVES_PER_BLOCK + L.wave; grp < ngroups; grp += (long)gridDim.x * WAVES_PER_BLOCK) {
    const long item = grp * g.G + L.grp;
    const bool valid = L.active && item < B;
    const long row = (valid ? item : 0) * g.N;
    stage_a((u16 *)a32, g, ValU16{e + row}, L.sub, L.active);
    wave_lds_fence();
    u16x2 r1[K], q1[K];
    product_split<K, true>(eo_f, a32, g, L.sub, want_q1, q, r1, q1);
#pragma unroll
    for (int t = 0; t < K; t++) r1[t] = r1[t] & (u16)(q - 1);
    if (valid) {
      if (rem1) store_pairs<K>(rem1 + row, g, L.sub, r1);
      if (want_q1) store_pairs<K>(quot1 + row, g, L.sub, q1);
    }
    wave_lds_fence();
    if (L.active) {                                   // the lifted message is the second product's broadcast operand
#pragma unroll
      for (int t = 0; t < K; t++) a32[K * L.sub + t] = lift_pair(r1[t], 2 * K * L.sub + 2 * t, g.N, q, p, lift_add);
    }
    wave_lds_fence();
    u16x2 r2[K], q2[K];
    product_split<K, false>(eo_fp, a32, g, L.sub, want_q2, p, r2, q2);
    if (valid) {
      store_pairs<K>(value + row, g, L.sub, r2);
      if (want_q2) store_pairs<K>(quot2 + row, g, L.sub, q2);
    }
    wave_lds_fence();
  }
}

// generic a*b mod `mod` split by I with per-item operands (multiplyPolynomials + dividePolynomials(.,I,.)).
// PUBKEY: generatePublicKeyH (index.js:72-79) for per-item keys: a = g in {-1,0,1} (int8, passed through `a`),
// b = p*fq reduced mod q (scale = p), only the remainder (= h before trimming) is stored.
template <int K, bool PUBKEY = false>
__global__ __launch_bounds__(BLOCK_THREADS) void k_polymul_split(Geom g, u32 mod, int pow2,
                                                                 const u16 *__restrict__ a, const u16 *__restrict__ b,
                                                                 long B, u16 *__restrict__ quot, u16 *__restrict__ rem,
                                                                 u32 scale = 1) {
  extern __shared__ __attribute__((aligned(16))) unsigned char lds[];
  const LaneId L = lane_id(g);
  const auto [eo, a32, raw] = per_item_bufs(lds, g, L);
  const long ngroups = (B + g.G - 1) / g.G;
  for (long grp = (long)blockIdx.x * WAVES_PER_BLOCK + L.wave; grp < ngroups; grp += (long)gridDim.x * WAVES_PER_BLOCK) {
    const long item = grp * g.G + L.grp;
    const bool valid = L.active && item < B;
    const long row = (valid ? item : 0) * g.N;
    if (PUBKEY) {
      stage_raw(raw, g.N, g.nl, ValU16x3m{b + row, scale, mod - 1}, L.sub, L.active);
      stage_a((u16 *)a32, g, ValTernary{(const int8_t *)a + row, mod - 1}, L.sub, L.active);
    } else {
      stage_raw(raw, g.N, g.nl, ValU16{b + row}, L.sub, L.active);
      stage_a((u16 *)a32, g, ValU16{a + row}, L.sub, L.active);
    }
    wave_lds_fence();
    if (L.active) build_eo(eo, g, ValLds{raw}, L.sub, g.nl);
    wave_lds_fence();
    u16x2 r[K], qv[K];
    if (pow2) {
      product_split<K, true>(eo, a32, g, L.sub, !PUBKEY, mod, r, qv);
#pragma unroll
      for (int t = 0; t < K; t++) r[t] = r[t] & (u16)(mod - 1);
    } else {
      product_split<K, false>(eo, a32, g, L.sub, true, mod, r, qv);
    }
    if (valid) {
      store_pairs<K>(rem + row, g, L.sub, r);
      if (!PUBKEY) store_pairs<K>(quot + row, g, L.sub, qv);
    }
    wave_lds_fence();
  }
}

// ================================================================================================================
// Ternary-stepping kernels ("add path").
//
// Every product on the hot path has one TERNARY operand (r, f, g, the lifted message), and on gfx950 every packed /
// multiply VALU op issues at 4 cycles per wave while a plain v_add_u32 issues at 2 (profiles/archive/r01_microbench_valu_lds.txt).
// So the ternary operand becomes the stepping operand: each coefficient is one step (0 skip, 1 "+w into S1", otherwise
// "+w into S2"; the other symbol c = 2 or -1 is applied once at the end, T = S1 + c*S2), the step bits of one block of
// 2K steps live in wave-uniform scalar words, zero steps are skipped by a scalar branch, and the windowed operand is
// accumulated with v_add_u32 on two packed 16-bit fields.  A field may only hold `limit` additions of values < q on
// top of a masked value before it could carry into its neighbour, so the accumulators are masked (mod q is free:
// q | 2^16) every ME steps, ME <= limit chosen by the launcher; products with exact small sums never mask (ME = 0).
//
// Two families use this machinery, written once below (step_code, load_block, TernOps, add_steps, add_core,
// add_product_split) over the policy types PerItemWin / SharedWin above, which state what differs between them; triangle,
// finish_pair, lift_pair and the stores are the ones the MAC kernels use:
//   per-item stepping (k_encrypt_t, k_decrypt_t, k_verify_keys_t): the stepping operand belongs to the item; one item
//     per wave (nl > 32), K <= 7 (2K step bits in half a dword) and (K+1)*(q-1) <= 65535;
//   shared-key stepping (k_decrypt_s): every wave steps over the same key; two items per wave, K = 9 / 11 / 13.
// Otherwise the MAC kernels above are used.
// ================================================================================================================

// Enter step j of a block, with coefficient v, into the block's code: "adds into S1" (v = 1) or "adds into S2" (the other non-zero
// symbol), at the bits Win::put states.  Written with 0/1 flags and immediate shifts so that no per-bit constant has to live in a
// VGPR (a select between two literal masks would: 2 x 2K constants hoisted for the whole kernel).
template <class Win>
static __device__ __forceinline__ void step_code(typename Win::Code &code, u32 v, int j) {
  u32 is1 = v == 1u ? 1u : 0u, is2 = v > 1u ? 1u : 0u;
  asm volatile("" : "+v"(is1), "+v"(is2));              // opaque: keeps the optimiser from folding this back into selects
  Win::put(code, is1, is2, j);
}

// The lane's block of a stepping operand: numeric u16 pairs for the triangle + the block's code.
template <class Win, int K, class F>
static __device__ __forceinline__ typename Win::Code load_block(F val, int N, int sub, u32 (&av)[K]) {
  typename Win::Code code = {};
#pragma unroll
  for (int t = 0; t < K; t++) {
    av[t] = pair_at<Win::clamps_loads>(val, 2 * K * sub + 2 * t, N);
    step_code<Win>(code, av[t] & 0xFFFFu, 2 * t); step_code<Win>(code, av[t] >> 16, 2 * t + 1);
  }
  return code;
}

// Lane-conditional snapshot L1 <- S1, L2 <- S2 as an exec-masked block of in-place full-rate v_mov (hipcc would turn
// plain assignments into v_cndmask, which is far slower on gfx950: profiles/archive/r01_microbench_exec_rate.txt).
template <int K>
static __device__ __forceinline__ void snapshot_if(bool take, u32 (&L1)[K], u32 (&L2)[K], const u32 (&S1)[K],
                                                   const u32 (&S2)[K]) {
  if (take) {
#pragma unroll
    for (int t = 0; t < K; t++) {
      asm volatile("v_mov_b32 %0, %1" : "+v"(L1[t]) : "v"(S1[t]));
      asm volatile("v_mov_b32 %0, %1" : "+v"(L2[t]) : "v"(S2[t]));
    }
  }
}

// TernOps<K>::step<B1, B2>: bit B1 of w1 set: S1[t] += W[t]; else bit B2 of w2 set: S2[t] += W[t]; else nothing.
// Wave-uniform scalar tests, exactly one taken branch per step, in-place full-rate adds.  One asm block per K (the
// operand lists must be spelled out), all seven generated from the one definition below: TERN_Rk(M) repeats M(i) for
// i = 1 .. k-1; element 0 is written out so that every further list element can carry its leading comma.
template <int K> struct TernOps;
#define TERN_R1(M)
#define TERN_R3(M) M(1) M(2)
#define TERN_R5(M) TERN_R3(M) M(3) M(4)
#define TERN_R7(M) TERN_R5(M) M(5) M(6)
#define TERN_R9(M) TERN_R7(M) M(7) M(8)
#define TERN_R11(M) TERN_R9(M) M(9) M(10)
#define TERN_R13(M) TERN_R11(M) M(11) M(12)
#define TERN_ADD_A(i) "v_add_u32 %[a" #i "], %[a" #i "], %[w" #i "]\n\t"
#define TERN_ADD_B(i) "v_add_u32 %[b" #i "], %[b" #i "], %[w" #i "]\n\t"
#define TERN_ACC_A(i) , [a##i] "+v"(S1[i])
#define TERN_ACC_B(i) , [b##i] "+v"(S2[i])
#define TERN_WIN(i) , [w##i] "v"(W[i])
#define TERN_OPS(K)                                                                                                  \
  template <>                                                                                                        \
  struct TernOps<K> {                                                                                                \
    template <int B1, int B2>                                                                                        \
    static __device__ __forceinline__ void step(u32 (&S1)[K], u32 (&S2)[K], const u32 (&W)[K], u32 w1, u32 w2) {     \
      asm volatile("s_bitcmp1_b32 %[wd1], %[bit1]\n\t"                                                               \
                   "s_cbranch_scc1 2f\n\t"                                                                           \
                   "s_bitcmp1_b32 %[wd2], %[bit2]\n\t"                                                               \
                   "s_cbranch_scc0 3f\n\t"                                                                           \
                   TERN_ADD_B(0) TERN_R##K(TERN_ADD_B)                                                               \
                   "s_branch 3f\n"                                                                                   \
                   "2:\n\t"                                                                                          \
                   TERN_ADD_A(0) TERN_R##K(TERN_ADD_A)                                                               \
                   "3:\n"                                                                                            \
                   : [a0] "+v"(S1[0]) TERN_R##K(TERN_ACC_A), [b0] "+v"(S2[0]) TERN_R##K(TERN_ACC_B)                  \
                   : [wd1] "s"(w1), [wd2] "s"(w2), [bit1] "i"(B1), [bit2] "i"(B2), [w0] "v"(W[0]) TERN_R##K(TERN_WIN) \
                   : "scc");                                                                                         \
    }                                                                                                                \
  };
TERN_OPS(1)
TERN_OPS(3)
TERN_OPS(5)
TERN_OPS(7)
TERN_OPS(9)
TERN_OPS(11)
TERN_OPS(13)
#undef TERN_OPS

// Steps J .. 2K-1 of one block (compile-time recursion so every bit index / register index is an immediate).
// Step j adds into S1 if bit j of w1 is set, else into S2 if bit Win::bit2(j) of w2 is.  ME: mask both sets every ME
// steps (0 = never: exact small sums).  At most ME additions of values < q land on a masked field between masks.
template <class Win, int K, int ME, int J>
static __device__ __forceinline__ void add_steps(u32 (&S1)[K], u32 (&S2)[K], u32 (&WE)[K], u32 (&WO)[K],
                                                 const typename Win::Entry (&nw)[K + Win::extra], u32 w1, u32 w2,
                                                 u32 fmask) {
  if constexpr (J < 2 * K) {
    if constexpr (ME > 0 && J % (ME > 0 ? ME : 1) == 0) {
#pragma unroll
      for (int t = 0; t < K; t++) { S1[t] &= fmask; S2[t] &= fmask; }
    }
    constexpr int s = J >> 1;
    u32 W[K];
#pragma unroll
    for (int t = 0; t < K; t++) W[t] = (J & 1) ? WO[(t - s + K) % K] : WE[(t - s + K) % K];
    TernOps<K>::template step<J, Win::bit2(J)>(S1, S2, W, w1, w2);
    if constexpr ((J & 1) != 0) { WE[K - 1 - s] = Win::even(nw[s]); WO[K - 1 - s] = Win::odd(nw[s], nw[s + Win::extra]); }
    add_steps<Win, K, ME, J + 1>(S1, S2, WE, WO, nw, w1, w2, fmask);
  }
}

// The block loop.  win: the item's window array in LDS, codes: one Win::Code per block of 2K steps, sub: the lane's
// index in the item.  WL: snapshot the accumulators before the lane's own block (the low half, for the quotient).
template <class Win, int K, int ME, bool WL>
static __device__ __forceinline__ void add_core(const typename Win::Entry *__restrict__ win,
                                                const typename Win::Code *__restrict__ codes, const Geom &g, int sub,
                                                u32 fmask, u32 (&S1)[K], u32 (&S2)[K], u32 (&L1)[K], u32 (&L2)[K]) {
  u32 WE[K], WO[K];
  const typename Win::Entry *nb = win + (K * sub + g.off);
  {
    typename Win::Entry prev = nb[-1];
#pragma unroll
    for (int x = 0; x < K; x++) { const typename Win::Entry v = nb[x]; WE[x] = Win::even(v); WO[x] = Win::odd(v, prev); prev = v; }
  }
#pragma unroll
  for (int t = 0; t < K; t++) { S1[t] = 0; S2[t] = 0; L1[t] = 0; L2[t] = 0; }
  const int nblk = g.nl;
  typename Win::Code held = Win::hold(codes[0]);
  for (int m = 0; m < nblk; m++) {
    u32 w1 = 0, w2 = 0;
    const typename Win::Code next = Win::fetch(codes, m, nblk, held, w1, w2);
    if constexpr (WL) snapshot_if<K>(m == sub, L1, L2, S1, S2);
    typename Win::Entry nw[K + Win::extra];
#pragma unroll
    for (int s = 0; s < K + Win::extra; s++) nw[s] = nb[-1 - s];
    add_steps<Win, K, ME, 0>(S1, S2, WE, WO, nw, w1, w2, fmask);
    held = Win::hold(next);
    nb -= K;
  }
}

// T = S1 + c*S2 per 16-bit field, as a u16 pair (mod 2^16 from here on).  NEG: c = -1 (mod q), else c = 2.
// c = 2 adds as u16 pairs: at q = 32768 a field's S1 + 2 S2 reaches 3 (q - 1) > 65535, and a 32-bit add would carry
// into the odd coefficient's field.  S1 + q - S2 <= 2q - 1 never does.
template <bool NEG>
static __device__ __forceinline__ u16x2 tern_combine(u32 s1, u32 s2, u32 fmask, u32 qq) {
  s1 &= fmask; s2 &= fmask;
  if constexpr (NEG) return as_pair(s1 + (qq - s2));
  else return as_pair(s1) + as_pair(s2) + as_pair(s2);
}

// Which lanes may store a whole block of 2K outputs without bounds checks, and which one holds the row's tail.
struct StorePlan {
  bool full, tail; int nv;      // nv: number of valid outputs in the tail lane (wave-uniform)
};
template <int K>
static __device__ __forceinline__ StorePlan store_plan(const Geom &g, int sub, bool valid) {
  StorePlan sp;
  sp.nv = g.N - 2 * K * (g.nl - 1);
  sp.full = valid && (sub < g.nl - 1 || sp.nv == 2 * K);
  sp.tail = valid && !sp.full;
  return sp;
}
// Store output pair t of this lane into its row (`lane_row` already points at the lane's first output).
template <class OutT>
static __device__ __forceinline__ void store_pair(OutT *lane_row, const StorePlan &sp, int t, u16x2 v) {
  if (sp.full) {
    lane_row[2 * t] = (OutT)v.x; lane_row[2 * t + 1] = (OutT)v.y;
  } else if (sp.tail) {
    if (2 * t < sp.nv) lane_row[2 * t] = (OutT)v.x;        // wave-uniform tests
    if (2 * t + 1 < sp.nv) lane_row[2 * t + 1] = (OutT)v.y;
  }
}

// Runs one stepped product and hands each finished pair to `emit(t, rem_pair, quot_pair)` right away (so no result
// arrays stay live: register pressure is what limits k_decrypt_s's occupancy).  Remainder / quotient as finish_pair states.
// av(s): the lane's s-th pair of the stepping operand (numeric), only evaluated for the triangle after the main loop.
// The per-item kernels call this with PerItemWin themselves: a forwarding tern_product_split in between changes the
// register allocation of k_decrypt_t and k_verify_keys_t.  k_decrypt_s goes through shared_product_split below.
template <class Win, int K, int ME, bool NEG, class AV, class Emit>
static __device__ __forceinline__ void add_product_split(const typename Win::Entry *win, const typename Win::Code *codes,
                                                         AV av, const Geom &g, int sub, bool want_quot, u32 mod,
                                                         Emit emit) {
  constexpr bool POW2 = ME > 0;
  const u32 fmask = POW2 ? (mod - 1) * 0x00010001u : 0xFFFFFFFFu;
  const u32 qq = mod * 0x00010001u;
  u32 S1[K], S2[K], L1[K], L2[K];
  if (want_quot) add_core<Win, K, ME, true>(win, codes, g, sub, fmask, S1, S2, L1, L2);
  else add_core<Win, K, ME, false>(win, codes, g, sub, fmask, S1, S2, L1, L2);
  // fold the snapshots into "low" right away (frees L2), then add the in-block triangle
  u16x2 low[K];
#pragma unroll
  for (int t = 0; t < K; t++) low[t] = tern_combine<NEG>(L1[t], L2[t], fmask, qq);
  if (want_quot) triangle<Win, K>(win, g, av, low);
#pragma unroll
  for (int t = 0; t < K; t++) {
    u16x2 rv, qv;
    finish_pair<POW2, Win::masks_rem>(tern_combine<NEG>(S1[t], S2[t], fmask, qq), low[t], want_quot, mod, rv, qv);
    emit(t, rv, qv);
  }
}

// encryptBits on the add path: stepping operand r in {0,1,2}, window h (shared).
template <int K, int ME>
__global__ __launch_bounds__(BLOCK_THREADS, 7) void k_encrypt_t(Geom g, u32 q, const u16 *__restrict__ h,
                                                             const uint8_t *__restrict__ r,
                                                             const uint8_t *__restrict__ m, long B,
                                                             u16 *__restrict__ e, u16 *__restrict__ quotE) {
  extern __shared__ __attribute__((aligned(16))) unsigned char lds[];
  uint2 *eo_h = (uint2 *)lds;
  const LaneId L = lane_id(g);
  u32 *codes = (u32 *)(lds + (size_t)g.eo_len * 8) + (size_t)L.wave * g.nl;
  build_eo(eo_h, g, ValU16{h}, threadIdx.x, BLOCK_THREADS);
  __syncthreads();
  const bool want_quot = quotE != nullptr;
  for (long item = (long)blockIdx.x * WAVES_PER_BLOCK + L.wave; item < B; item += (long)gridDim.x * WAVES_PER_BLOCK) {
    int sub = L.sub, N = g.N;                            // re-materialised per iteration: keeps the glue out of LICM's reach
    asm volatile("" : "+v"(sub), "+s"(N));
    const long row = item * N;
    {
      u32 av[K];
      const u32 word = load_block<PerItemWin, K>(ValU8{r + row}, N, sub, av);
      if (L.active) codes[sub] = word;
    }
    wave_lds_fence();
    // everything below runs behind the hot loop; `sub2` is a fresh opaque copy so that none of its index arithmetic
    // is CSE'd with the pre-loop block load and kept live (spilled) across the loop
    auto r_pair = [&](int t) -> u32 {                                     // reloaded behind the hot loop (L1/L2 hit)
      int sub2 = sub;
      asm volatile("" : "+v"(sub2));
      return pair_at(ValU8{r + row}, 2 * K * sub2 + 2 * t, N);
    };
    add_product_split<PerItemWin, K, ME, false>(eo_h, codes, r_pair, g, sub, want_quot, q, [&](int t, u16x2 rv, u16x2 qv) {
      int sub2 = sub;
      asm volatile("" : "+v"(sub2));
      const StorePlan sp = store_plan<K>(g, sub2, L.active);
      const long lane0 = row + 2 * K * sub2;
      const int k = 2 * K * sub2 + 2 * t;
      const int k0 = k < N ? k : N - 1, k1 = k + 1 < N ? k + 1 : N - 1;
      const uint8_t *mr = m + row;
      const u16x2 add = {(u16)mr[k0], (u16)mr[k1]};                         // out-of-row lanes never store
      store_pair(e + lane0, sp, t, (rv + add) & (u16)(q - 1));
      if (want_quot) store_pair(quotE + lane0, sp, t, qv);
    });
    wave_lds_fence();
  }
}

// decryptBits on the add path: product 1 steps over f (shared, codes built once) with a per-item window of e;
// product 2 steps over the lifted message (per item, in registers) with the shared window of fp.  Needs p == 3.
template <int K, int ME>
__global__ __launch_bounds__(BLOCK_THREADS) void k_decrypt_t(Geom g, u32 q, u32 p, u32 lift_add,
                                                             const int8_t *__restrict__ f,
                                                             const uint8_t *__restrict__ fp,
                                                             const u16 *__restrict__ e, long B,
                                                             uint8_t *__restrict__ value, u16 *__restrict__ quot1,
                                                             u16 *__restrict__ rem1, uint8_t *__restrict__ quot2) {
  extern __shared__ __attribute__((aligned(16))) unsigned char lds[];
  uint2 *eo_fp = (uint2 *)lds;
  u32 *codes_f = (u32 *)(lds + (size_t)g.eo_len * 8);
  const LaneId L = lane_id(g);
  const size_t per_wave = (size_t)g.eo_len * 8 + (size_t)g.nl * 4;
  unsigned char *wbase = lds + (size_t)g.eo_len * 8 + (size_t)g.nl * 4 + (size_t)L.wave * per_wave;
  uint2 *eo_e = (uint2 *)wbase;
  u32 *codes_b = (u32 *)(wbase + (size_t)g.eo_len * 8);
  build_eo(eo_fp, g, ValU8{fp}, threadIdx.x, BLOCK_THREADS);
  u32 av_f[K];                                           // this lane's block of f, the same for every item
  {
    const u32 wf = load_block<PerItemWin, K>(ValTernary{f, q - 1}, g.N, L.sub, av_f);
    if (L.wave == 0 && L.active) codes_f[L.sub] = wf;
  }
  __syncthreads();
  const bool want_q1 = quot1 != nullptr, want_q2 = quot2 != nullptr;
  for (long item = (long)blockIdx.x * WAVES_PER_BLOCK + L.wave; item < B; item += (long)gridDim.x * WAVES_PER_BLOCK) {
    const long row = item * g.N;
    if (L.active) build_eo(eo_e, g, ValU16{e + row}, L.sub, g.nl);
    wave_lds_fence();
    const StorePlan sp = store_plan<K>(g, L.sub, L.active);
    const long lane0 = row + 2 * K * L.sub;
    u32 av_b[K], wb = 0;
    // remainder1 / quotient1 stored pair by pair; the lifted pair is the second stepping operand
    add_product_split<PerItemWin, K, ME, true>(eo_e, codes_f, [&](int t) { return av_f[t]; }, g, L.sub, want_q1, q, [&](int t, u16x2 rv, u16x2 qv) {
      rv = rv & (u16)(q - 1);
      if (rem1) store_pair(rem1 + lane0, sp, t, rv);
      if (want_q1) store_pair(quot1 + lane0, sp, t, qv);
      av_b[t] = lift_pair(rv, 2 * K * L.sub + 2 * t, g.N, q, p, lift_add);
      step_code<PerItemWin>(wb, av_b[t] & 0xFFFFu, 2 * t); step_code<PerItemWin>(wb, av_b[t] >> 16, 2 * t + 1);
    });
    if (L.active) codes_b[L.sub] = wb;
    wave_lds_fence();
    add_product_split<PerItemWin, K, 0, false>(eo_fp, codes_b, [&](int t) { return av_b[t]; }, g, L.sub, want_q2, p, [&](int t, u16x2 rv, u16x2 qv) {
      store_pair(value + lane0, sp, t, rv);
      if (want_q2) store_pair(quot2 + lane0, sp, t, qv);
    });
    wave_lds_fence();
  }
}

// ================================================================================================================
// Shared-stepping add path (decrypt).  Both products of decryptBits can step over a SHARED key operand (f, then fp),
// so every wave of the launch follows the same step masks.  That allows two items per wave (32 lanes x K pairs each,
// K = 9 / 11 / 13) under one scalar control stream -- the scalar unit, not the VALU, is what limits the add path
// (profiles/archive/r01_microbench_step_rate.txt).  The per-item operand (e, then the lifted message) is the window; it is kept
// in LDS as ONE cyclic array of aligned pairs E[u] = (bc[2u], bc[2u+1]); the odd-aligned pairs are derived on the fly,
// O[u] = alignbit(E[u], E[u-1], 16).  N must be odd (so that the cyclic wrap turns aligned pairs into odd-aligned ones).
// ================================================================================================================

// Fill this item's cyclic pair array from the K aligned pairs P[t] = (x[2v], x[(2v+1) mod N]), v = K*sub + t, held in
// registers by the item's lanes.  E points at logical entry u = -off (one spare entry sits in front of it, one dummy
// slot behind the array absorbs writes of lanes that have nothing to contribute -- no per-element predication).
//   phase 1: E[u] = P[u] for u in [0, H), H = (N+1)/2 (the aligned pairs, the last one wrapping to x[0])
//   phase 2: every other entry is either another aligned pair (2u mod N even) or the odd-aligned pair
//            (x[j], x[j+1]) = (hi(P[(j-1)/2]), lo(P[(j+1)/2])), j = 2u mod N, read back from phase 1's region
template <int K>
static __device__ __forceinline__ void build_cyclic_pairs(u32 *E, const Geom &g, int sub, bool active, const u32 (&P)[K],
                                                          bool patch_wrap, u32 x0) {
  const int N = g.N, H = (N + 1) >> 1, off = g.off, top = K * g.nl;
  const int dummy = top + off;                          // one slot past the last real entry
#pragma unroll
  for (int t = 0; t < K; t++) {
    const int v = K * sub + t;
    E[(active && v < H) ? v + off : dummy] = P[t];
  }
  wave_lds_fence();
  if (patch_wrap && active && sub == 0) ((u16 *)E)[2 * (H - 1 + off) + 1] = (u16)x0;   // P[H-1] = (x[N-1], x[0])
  wave_lds_fence();
  const int below = off + 1, total = below + (top - H);  // entries u in [-off-1, -1] and [H, top)
  for (int idx = sub; idx < total; idx += g.nl) {
    const int u = idx < below ? idx - below : H + (idx - below);
    int j = 2 * u;                                       // reduce 2u into [0, N)
    j += j < 0 ? N : 0; j += j < 0 ? N : 0; j -= j >= N ? N : 0;
    const int hi_src = (j + 1) >> 1, lo_src = j >> 1;    // j even: both = j/2 (aligned pair); j odd: neighbours
    const u32 a = E[hi_src + off], b = E[lo_src + off];
    const u32 val = (j & 1) ? odd_pair(a, b) : a;
    E[active ? u + off : dummy] = val;
  }
  wave_lds_fence();
}

// add_product_split for shared-key stepping: E is the item's cyclic pair array, masks one uint2 per block (x: steps
// adding into S1, y: steps adding into S2), identical for every item; av the lane's block of the stepping operand.
template <int K, int ME, bool NEG, class Emit>
static __device__ __forceinline__ void shared_product_split(const u32 *E, const uint2 *masks, const u32 *av,
                                                            const Geom &g, int sub, bool want_quot, u32 mod, Emit emit) {
  add_product_split<SharedWin, K, ME, NEG>(E, masks, [&](int s) { return av[s]; }, g, sub, want_quot, mod, emit);
}

// ---- ternary x ternary product on v_dot8_u32_u4 (decrypt's c = fp * b mod 3) ---------------------------------------
// Both operands are in {0,1,2}: 8 multiply-accumulates per instruction, no branches, exact sums (<= 4N).  Layout for
// this phase: lane l owns the 32 outputs k = 32 l + t.  A8r[I] (shared, built once per workgroup) packs fp[8I+7-i] in
// nibble i; the per-item operand b is a nibble stream in LDS (coefficient j at nibble j + 8*nblk, extended cyclically
// below 0), and FB(t, I) = the forward window b[k-8I-7 .. k-8I] is cut out of two stream dwords with v_alignbit; going
// to the next block shifts all windows by 8 slots, so only 8 of the 32 are recomputed.  The low half for the quotient
// is the accumulator snapshot before block 4 l plus a 4-block correction against the zero-extended stream.
// tools/dot8_model.py is the executable specification (checked against a direct convolution).
static __device__ __forceinline__ u32 funnel(u32 hi, u32 lo, int sh) { return __builtin_amdgcn_alignbit(hi, lo, sh); }

// nibble stream of b from the K pairs per lane of the 32-lane product-1 layout (P[t] = (b[2v], b[2v+1]), v = K sub + t)
template <int K>
static __device__ __forceinline__ void build_nibble_stream(u32 *dwp, int N, int nblk, int sub, bool active,
                                                           const u32 (&P)[K]) {
  if (active) {
    unsigned char *by = (unsigned char *)dwp + 4 * nblk + K * sub;       // coefficient 0 sits at dword nblk
#pragma unroll
    for (int t = 0; t < K; t++) by[t] = (unsigned char)((P[t] & 0xFu) | (((P[t] >> 16) & 0xFu) << 4));
  }
  wave_lds_fence();
  const int a = N >> 3, r4 = 4 * (N & 7);                                 // N nibbles = a dwords + r nibbles
  for (int w = sub; w < nblk; w += 32) {                                 // coefficient j < 0 is b[j + N]
    const u32 lo = dwp[w + a], hi = dwp[w + a + 1];
    if (active) dwp[w] = r4 ? funnel(hi, lo, r4) : lo;
  }
  wave_lds_fence();
}

template <bool WL>
static __device__ __forceinline__ void dot8_core(const u32 *__restrict__ dwp, const u32 *__restrict__ a8, int nblk, int l,
                                                 u32 (&acc)[32], u32 (&snap)[32]) {
  u32 S[32];
  const u32 *base = dwp + 4 * l + nblk - 1;
  u32 Y;
  {
    u32 D[5];
#pragma unroll
    for (int g = 0; g < 5; g++) D[g] = base[g];
#pragma unroll
    for (int t = 0; t < 32; t++) {
      const int g = (t + 1) >> 3, ph = (t + 1) & 7;
      S[t] = ph ? funnel(D[g + 1 < 5 ? g + 1 : 4], D[g], 4 * ph) : D[g];
    }
    Y = D[0];
  }
#pragma unroll
  for (int t = 0; t < 32; t++) { acc[t] = 0; snap[t] = 0; }
  const u32 *xp = base - 1;                                               // block I reads xp[-I]
  for (int u = 0; u < (nblk >> 2); u++) {
    if constexpr (WL) {
      if (u == l) {
#pragma unroll
        for (int t = 0; t < 32; t++) asm volatile("v_mov_b32 %0, %1" : "+v"(snap[t]) : "v"(acc[t]));
      }
    }
    const uint4 av = *(const uint4 *)(a8 + 4 * u);
    const u32 A[4] = {av.x, av.y, av.z, av.w};
    u32 X[4];
#pragma unroll
    for (int v = 0; v < 4; v++) X[v] = xp[-(4 * u + v)];
#pragma unroll
    for (int v = 0; v < 4; v++) {
#pragma unroll
      for (int t = 0; t < 32; t++) acc[t] = __builtin_amdgcn_udot8(A[v], S[(t - 8 * v) & 31], acc[t], false);
#pragma unroll
      for (int tp = 0; tp < 7; tp++) S[(tp - 8 * (v + 1)) & 31] = funnel(Y, X[v], 4 * (tp + 1));
      S[(7 - 8 * (v + 1)) & 31] = Y;
      Y = X[v];
    }
  }
}

// c = fp * b mod 3 for one item per 32-lane half: value / quotient2 rows stored directly.
template <bool WQ>
static __device__ __forceinline__ void dot8_product_mod3(const u32 *dwp, const u32 *a8, int N, int nblk, int l, bool valid,
                                                         int lanes, uint8_t *__restrict__ value_row,
                                                         uint8_t *__restrict__ quot_row) {
  u32 acc[32], low[32];
  dot8_core<WQ>(dwp, a8, nblk, l, acc, low);
  if (WQ) {                                             // low += in-block part, against the zero-extended stream
    u32 ZD[9];
#pragma unroll
    for (int g = 0; g < 4; g++) ZD[g] = 0;
#pragma unroll
    for (int g = 0; g < 5; g++) ZD[4 + g] = dwp[nblk + g];
#pragma unroll
    for (int d = 0; d < 4; d++) {
      const u32 a = a8[4 * l + d];
#pragma unroll
      for (int t = 0; t < 32; t++) {
        const int g = ((t + 1) >> 3) + 3 - d, ph = (t + 1) & 7;
        const u32 w = ph ? funnel(ZD[g + 1], ZD[g], 4 * ph) : ZD[g];
        low[t] = __builtin_amdgcn_udot8(a, w, low[t], false);
      }
    }
  }
  const int nv = N - 32 * (lanes - 1);                  // valid outputs of the last lane (wave-uniform)
  const bool full = valid && l < lanes - 1, tail = valid && l == lanes - 1;
  uint8_t *vr = value_row + 32 * l, *qr = quot_row + 32 * l;
#pragma unroll
  for (int t = 0; t < 32; t++) {
    const u32 T = acc[t];
    const u32 rv = T % 3u;
    u32 qv = 0;
    if (WQ) { const u32 h = (T - low[t]) % 3u; qv = h ? 3u - h : 0u; }
    if (full || (tail && t < nv)) {
      vr[t] = (uint8_t)rv;
      if (WQ) qr[t] = (uint8_t)qv;
    }
  }
}

// decryptBits with both products stepping over the shared key (f, then fp); two items per wave.  p must be 3.
template <int K, int ME, bool D8>
__global__ __launch_bounds__(BLOCK_THREADS, 4) void k_decrypt_s(Geom g, u32 q, u32 lift_add, const int8_t *__restrict__ f,
                                                             const uint8_t *__restrict__ fp,
                                                             const u16 *__restrict__ e, long B,
                                                             uint8_t *__restrict__ value, u16 *__restrict__ quot1,
                                                             u16 *__restrict__ rem1, uint8_t *__restrict__ quot2) {
  constexpr u32 p = 3u;                                                 // the launcher's precondition; lift_add has taken its argument's place
  extern __shared__ __attribute__((aligned(16))) unsigned char lds[];
  uint2 *masks_f = (uint2 *)lds;
  uint2 *masks_fp = masks_f + g.nl;
  u32 *blk_f = (u32 *)(masks_fp + g.nl);                                // [nl][K] numeric pairs of f (for the triangles)
  u32 *blk_fp = blk_f + (size_t)g.nl * K;
  const LaneId L = lane_id(g);
  const int nblk = ((g.N + 31) >> 5) << 2;                              // dot8 phase: 8-step blocks, multiple of 4
  u32 *a8fp = blk_fp + (size_t)g.nl * K;                                // [nblk] reversed-nibble words of fp (16-byte aligned)
  const int e_alloc = g.eo_len + 2;                                     // dwords per item incl. spare front entry + dummy slot
  const int e_off0 = nblk + (L.wave * g.G + L.grp) * e_alloc + 1;
  if (L.wave == 0 && L.active && L.grp == 0) {                          // key-dependent tables, once per workgroup
    u32 av[K];
    masks_f[L.sub] = load_block<SharedWin, K>(ValTernary{f, q - 1}, g.N, L.sub, av);
#pragma unroll
    for (int t = 0; t < K; t++) blk_f[K * L.sub + t] = av[t];
    masks_fp[L.sub] = load_block<SharedWin, K>(ValU8{fp}, g.N, L.sub, av);
#pragma unroll
    for (int t = 0; t < K; t++) blk_fp[K * L.sub + t] = av[t];
  }
  if (D8 && L.wave == 1) {                                              // A8r[I]: nibble i = fp[8I + 7 - i]
    for (int I = L.lane; I < nblk; I += 64) {
      u32 w = 0;
#pragma unroll
      for (int i = 0; i < 8; i++) { const int j = 8 * I + 7 - i; w |= (j < g.N ? (u32)fp[j] & 0xFu : 0u) << (4 * i); }
      a8fp[I] = w;
    }
  }
  const u32 *av_f = blk_f + K * L.sub, *av_fp = blk_fp + K * L.sub;
  __syncthreads();
  const long ngroups = (B + g.G - 1) / g.G;
  const bool want_q1 = quot1 != nullptr, want_q2 = quot2 != nullptr;
  for (long grp = (long)blockIdx.x * WAVES_PER_BLOCK + L.wave; grp < ngroups; grp += (long)gridDim.x * WAVES_PER_BLOCK) {
    // Re-materialise the lane index and N every iteration: otherwise the compiler hoists all per-lane address /
    // predicate arithmetic of the glue below out of this loop and keeps ~100 registers live (and spilled) across
    // both hot loops.
    int sub = L.sub, N = g.N, e_off = e_off0;
    asm volatile("" : "+v"(sub), "+s"(N), "+v"(e_off));
    u32 *E = a8fp + e_off;
    const long item = grp * g.G + L.grp;
    const bool valid = L.active && item < B;
    const long row = (valid ? item : 0) * N;
    // ---- product 1: a = f * e mod q, window = this item's ciphertext
    u32 P[K];
    {
      const u16 *er = e + row;
#pragma unroll
      for (int t = 0; t < K; t++) {                       // clamped indices: lanes past the end load something harmless
        const int j = 2 * (K * sub + t);
        const int j0 = j < N ? j : N - 1;
        const int j1 = j + 1 < N ? j + 1 : (j + 1 == N ? 0 : N - 1);
        P[t] = (u32)er[j0] | ((u32)er[j1] << 16);
      }
    }
    build_cyclic_pairs<K>(E, g, sub, L.active, P, false, 0u);
    // remainder1 / quotient1 are stored and the centred lift is applied pair by pair; the lifted
    // message replaces P: it is the window of product 2
    const StorePlan sp = store_plan<K>(g, sub, valid);
    const long lane0 = row + 2 * K * sub;                              // this lane's first output
    shared_product_split<K, ME, true>(E, masks_f, av_f, g, sub, want_q1, q, [&](int t, u16x2 rv, u16x2 qv) {
      if (rem1) store_pair(rem1 + lane0, sp, t, rv);
      if (want_q1) store_pair(quot1 + lane0, sp, t, qv);
      P[t] = lift_pair(rv, 2 * (K * sub + t), N, q, p, lift_add);
    });
    wave_lds_fence();                                                   // everyone is done reading E(e)
    if constexpr (D8) {
      // ---- product 2 on v_dot8: the item's buffer now holds the nibble stream of the lifted message
      int d_off = e_off - 1, l8 = L.lane & 31;                          // 16-byte aligned start of the item's buffer
      asm volatile("" : "+v"(d_off), "+v"(l8));                         // keep this phase's addresses out of product 1
      u32 *dwp = a8fp + d_off;
      build_nibble_stream<K>(dwp, N, nblk, sub, L.active, P);
      const int lanes8 = (N + 31) >> 5;
      const bool act8 = l8 < lanes8 && L.active;
      l8 = act8 ? l8 : 0;
      if (want_q2) dot8_product_mod3<true>(dwp, a8fp, N, nblk, l8, valid && act8, lanes8, value + row, quot2 + row);
      else dot8_product_mod3<false>(dwp, a8fp, N, nblk, l8, valid && act8, lanes8, value + row, value + row);
    } else {
      build_cyclic_pairs<K>(E, g, sub, L.active, P, true, P[0] & 0xFFFFu);
      // ---- product 2: c = fp * b mod p (exact small sums, no masking)
      shared_product_split<K, 0, false>(E, masks_fp, av_fp, g, sub, want_q2, p, [&](int t, u16x2 rv, u16x2 qv) {
        store_pair(value + lane0, sp, t, rv);
        if (want_q2) store_pair(quot2 + lane0, sp, t, qv);
      });
    }
    wave_lds_fence();
  }
}

// verifyKeysInputs, index.js:141-197, per-item key material; three products per item.
template <int K>
__global__ __launch_bounds__(BLOCK_THREADS) void k_verify_keys(
    Geom g, u32 q, u32 p, const int8_t *__restrict__ f, const int8_t *__restrict__ gg, const u16 *__restrict__ fq,
    const uint8_t *__restrict__ fp, const u16 *__restrict__ h, long B, u16 *__restrict__ quot_fq,
    u16 *__restrict__ rem_fq, uint8_t *__restrict__ quot_fp, uint8_t *__restrict__ rem_fp, u16 *__restrict__ quot_h,
    u16 *__restrict__ rem_h, uint8_t *__restrict__ flags) {
  extern __shared__ __attribute__((aligned(16))) unsigned char lds[];
  const LaneId L = lane_id(g);
  const auto [eo, a32, raw] = per_item_bufs(lds, g, L);
  const long ngroups = (B + g.G - 1) / g.G;
  for (long grp = (long)blockIdx.x * WAVES_PER_BLOCK + L.wave; grp < ngroups; grp += (long)gridDim.x * WAVES_PER_BLOCK) {
    const long item = grp * g.G + L.grp;
    const bool valid = L.active && item < B;
    const long row = (valid ? item : 0) * g.N;
    u32 fl = 0;
    u16x2 r[K], qv[K];
    // ---- fq * f mod q (index.js:158-160)
    stage_raw(raw, g.N, g.nl, ValTernary{f + row, q - 1}, L.sub, L.active);
    stage_a((u16 *)a32, g, ValU16{fq + row}, L.sub, L.active);
    wave_lds_fence();
    if (L.active) build_eo(eo, g, ValLds{raw}, L.sub, g.nl);
    wave_lds_fence();
    product_split<K, true>(eo, a32, g, L.sub, true, q, r, qv);
    {
      InverseCheck<K> inv;
#pragma unroll
      for (int t = 0; t < K; t++) { r[t] = r[t] & (u16)(q - 1); inv.note(L.sub, t, g.N, r[t]); }
      if (inv.invalid(g, L)) fl |= NTRU_FLAG_INVALID_FQ;
    }
    if (valid) { store_pairs<K>(rem_fq + row, g, L.sub, r); store_pairs<K>(quot_fq + row, g, L.sub, qv); }
    wave_lds_fence();
    // ---- fp * f mod p (index.js:161-163)
    // the staged f only differs in what -1 maps to: patch q-1 -> p-1 in place instead of re-reading it
    if (q > 2) {
      if (L.active) for (int i = L.sub; i < g.N; i += g.nl) { const u16 v = raw[i]; raw[i] = v == (u16)(q - 1) ? (u16)(p - 1) : v; }
    } else {                                              // q = 2: -1 and +1 coincide mod q, so re-stage from the source
      stage_raw(raw, g.N, g.nl, ValTernary{f + row, p - 1}, L.sub, L.active);
    }
    stage_a((u16 *)a32, g, ValU8{fp + row}, L.sub, L.active);
    wave_lds_fence();
    if (L.active) build_eo(eo, g, ValLds{raw}, L.sub, g.nl);
    wave_lds_fence();
    product_split<K, false>(eo, a32, g, L.sub, true, p, r, qv);
    {
      InverseCheck<K> inv;
#pragma unroll
      for (int t = 0; t < K; t++) inv.note(L.sub, t, g.N, r[t]);
      if (inv.invalid(g, L)) fl |= NTRU_FLAG_INVALID_FP;
    }
    if (valid) { store_pairs<K>(rem_fp + row, g, L.sub, r); store_pairs<K>(quot_fp + row, g, L.sub, qv); }
    wave_lds_fence();
    // ---- (p*fq) * g mod q (index.js:155,164-166)
    stage_raw(raw, g.N, g.nl, ValTernary{gg + row, q - 1}, L.sub, L.active);
    stage_a((u16 *)a32, g, ValU16x3{fq + row, p}, L.sub, L.active);
    wave_lds_fence();
    if (L.active) build_eo(eo, g, ValLds{raw}, L.sub, g.nl);
    wave_lds_fence();
    product_split<K, true>(eo, a32, g, L.sub, true, q, r, qv);
    {
      u32 hp[K]; int top = -1;
#pragma unroll
      for (int t = 0; t < K; t++) {
        r[t] = r[t] & (u16)(q - 1);
        hp[t] = pair_at<false>(ValU16{h + row}, 2 * K * L.sub + 2 * t, g.N);
        note_top(top, 2 * K * L.sub + 2 * t, hp[t]);
      }
      const int hl = item_trimmed_len(top, g, L);
      bool bad = false;
#pragma unroll
      for (int t = 0; t < K; t++) bad |= differs_below(hl, 2 * K * L.sub + 2 * t, hp[t], r[t]);
      if (item_any(bad, g, L)) fl |= NTRU_FLAG_INVALID_H;
    }
    if (valid) {
      store_pairs<K>(rem_h + row, g, L.sub, r); store_pairs<K>(quot_h + row, g, L.sub, qv);
      if (L.sub == 0) flags[item] = (uint8_t)fl;
    }
    wave_lds_fence();
  }
}

// verifyKeysInputs on the add path: every product steps over a per-item ternary operand (f, f, g) with a per-item
// window (fq, fp, 3*fq mod q), one item per wave.  Needs p == 3 (so that -1 = 2 mod p is the "other" symbol).
template <int K, int ME>
__global__ __launch_bounds__(BLOCK_THREADS) void k_verify_keys_t(
    Geom g, u32 q, u32 p, const int8_t *__restrict__ f, const int8_t *__restrict__ gg, const u16 *__restrict__ fq,
    const uint8_t *__restrict__ fp, const u16 *__restrict__ h, long B, u16 *__restrict__ quot_fq,
    u16 *__restrict__ rem_fq, uint8_t *__restrict__ quot_fp, uint8_t *__restrict__ rem_fp, u16 *__restrict__ quot_h,
    u16 *__restrict__ rem_h, uint8_t *__restrict__ flags) {
  extern __shared__ __attribute__((aligned(16))) unsigned char lds[];
  const LaneId L = lane_id(g);
  const size_t raw_len = ((size_t)g.N + 1) & ~(size_t)1;
  const size_t per_wave = (size_t)g.eo_len * 8 + (size_t)g.nl * 4 + raw_len * 2;
  unsigned char *wbase = lds + (size_t)L.wave * per_wave;
  uint2 *eo = (uint2 *)wbase;
  u32 *codes = (u32 *)(wbase + (size_t)g.eo_len * 8);
  u16 *raw = (u16 *)(wbase + (size_t)g.eo_len * 8 + (size_t)g.nl * 4);
  for (long item = (long)blockIdx.x * WAVES_PER_BLOCK + L.wave; item < B; item += (long)gridDim.x * WAVES_PER_BLOCK) {
    int sub = L.sub, N = g.N;
    asm volatile("" : "+v"(sub), "+s"(N));
    const long row = item * N;
    u32 fl = 0;
    // one product: window `win` (already mapped into [0, mod)), stepping operand `step` (ternary, -1 -> neg)
    auto product = [&](auto win, const int8_t *step, u32 neg, auto split, auto emit) {
      asm volatile("" : "+v"(sub));                      // fresh lane index: no load of this product is CSE'd with another's
      stage_raw(raw, N, g.nl, win, sub, L.active);
      {
        u32 av[K];
        const u32 word = load_block<PerItemWin, K>(ValTernary{step + row, neg}, N, sub, av);
        if (L.active) codes[sub] = word;
      }
      wave_lds_fence();
      if (L.active) build_eo(eo, g, ValLds{raw}, sub, g.nl);
      wave_lds_fence();
      auto s_pair = [&](int t) -> u32 {                                   // reloaded behind the hot loop
        int sub2 = sub;
        asm volatile("" : "+v"(sub2));
        return pair_at(ValTernary{step + row, neg}, 2 * K * sub2 + 2 * t, N);
      };
      split(s_pair, emit);
      wave_lds_fence();
    };
    InverseCheck<K> inv;
    // ---- fq * f mod q
    product(ValU16{fq + row}, f, q - 1,
            [&](auto s_pair, auto emit) { add_product_split<PerItemWin, K, ME, true>(eo, codes, s_pair, g, sub, true, q, emit); },
            [&](int t, u16x2 rv, u16x2 qv) {
              int sub2 = sub; asm volatile("" : "+v"(sub2));
              rv = rv & (u16)(q - 1);
              const StorePlan sp = store_plan<K>(g, sub2, L.active);
              const long lane0 = row + 2 * K * sub2;
              store_pair(rem_fq + lane0, sp, t, rv);
              store_pair(quot_fq + lane0, sp, t, qv);
              inv.note(sub2, t, N, rv);
            });
    if (inv.invalid(g, L)) fl |= NTRU_FLAG_INVALID_FQ;
    // ---- fp * f mod p
    inv = InverseCheck<K>();
    product(ValU8{fp + row}, f, p - 1,
            [&](auto s_pair, auto emit) { add_product_split<PerItemWin, K, 0, false>(eo, codes, s_pair, g, sub, true, p, emit); },
            [&](int t, u16x2 rv, u16x2 qv) {
              int sub2 = sub; asm volatile("" : "+v"(sub2));
              const StorePlan sp = store_plan<K>(g, sub2, L.active);
              const long lane0 = row + 2 * K * sub2;
              store_pair(rem_fp + lane0, sp, t, rv);
              store_pair(quot_fp + lane0, sp, t, qv);
              inv.note(sub2, t, N, rv);
            });
    if (inv.invalid(g, L)) fl |= NTRU_FLAG_INVALID_FP;
    // ---- (p*fq) * g mod q: the window is reduced mod q (same product; the unreduced p*fq of index.js:155 is host glue)
    int top = -1;                                                  // h's trimmed length first: the product's emit compares below it
#pragma unroll
    for (int t = 0; t < K; t++) note_top(top, 2 * K * sub + 2 * t, pair_at(ValU16{h + row}, 2 * K * sub + 2 * t, N));
    const int hl = item_trimmed_len(top, g, L);
    bool bad = false;
    product(ValU16x3m{fq + row, p, q - 1}, gg, q - 1,
            [&](auto s_pair, auto emit) { add_product_split<PerItemWin, K, ME, true>(eo, codes, s_pair, g, sub, true, q, emit); },
            [&](int t, u16x2 rv, u16x2 qv) {
              int sub2 = sub; asm volatile("" : "+v"(sub2));
              rv = rv & (u16)(q - 1);
              const StorePlan sp = store_plan<K>(g, sub2, L.active);
              const long lane0 = row + 2 * K * sub2;
              store_pair(rem_h + lane0, sp, t, rv);
              store_pair(quot_h + lane0, sp, t, qv);
              bad |= differs_below(hl, 2 * K * sub2 + 2 * t, pair_at(ValU16{h + row}, 2 * K * sub2 + 2 * t, N), rv);
            });
    if (item_any(bad, g, L)) fl |= NTRU_FLAG_INVALID_H;
    if (L.active && sub == 0) flags[item] = (uint8_t)fl;
  }
}

// ---- host side: launchers of the vector-ALU families ---------------------------------------------------------------------------

static int pick_K(int N) {
  for (int K = 1; K <= 15; K += 2)
    if ((N + 2 * K - 1) / (2 * K) <= 64) return K;
  return 0;
}

static Geom make_geom(int N, int K) {
  Geom g;
  g.N = N;
  g.nl = (N + 2 * K - 1) / (2 * K);
  g.G = 64 / g.nl;
  g.off = K * g.nl;
  g.eo_len = 2 * K * g.nl;
  g.a_len = K * g.nl;
  return g;
}

struct Launch { Geom g; int K; long blocks; size_t lds; };   // blocks: work blocks, capped to residency by launch_resident()

// shared_eo: number of EO arrays shared by the workgroup; per_item_eo: whether each item also needs its own EO array.
static int plan(const ntru_engine *eng, int N, long B, int shared_eo, bool per_item_eo, Launch *L) {
  int K = pick_K(N);
  if (!K) return fail(NTRU_ERR_UNSUPPORTED, "N too large");
  L->K = K;
  L->g = make_geom(N, K);
  const size_t per_wave = per_item_eo ? per_item_lds(L->g).per_wave : (size_t)L->g.G * L->g.a_len * 4;
  L->lds = (size_t)shared_eo * L->g.eo_len * 8 + WAVES_PER_BLOCK * per_wave;
  if (L->lds > 160 * 1024) return fail(NTRU_ERR_UNSUPPORTED, "parameter set needs more than 160 KiB of LDS");
  const long ngroups = (B + L->g.G - 1) / L->g.G;
  L->blocks = (ngroups + WAVES_PER_BLOCK - 1) / WAVES_PER_BLOCK;
  return NTRU_OK;
}

// The add path needs one item per wave, 2K step bits in half a dword (K <= 7) and at least K values below q fitting
// a 16-bit field on top of a masked one.  Returns the mask interval ME (2K: once per block, K: twice) or 0.  Leaves
// the launch geometry in L->K and L->g: the caller sizes its LDS from it and hands the byte counts to plan_add().
static int add_path_me(const ntru_engine *eng, int N, int q, Launch *L) {
  if (eng->path == 1) return 0;
  int K = pick_K(N);
  if (!K || K > 7) return 0;
  L->K = K;
  L->g = make_geom(N, K);
  if (L->g.G != 1) return 0;
  long limit = 65535 / (q - 1) - 1;          // additions of values < q allowed on a masked field
  if (limit >= 2 * K) return 2 * K;
  if (limit >= K) return K;
  return 0;
}

static int plan_add(long B, size_t shared_bytes, size_t per_wave_bytes, Launch *L) {
  L->lds = shared_bytes + WAVES_PER_BLOCK * per_wave_bytes;
  if (L->lds > 160 * 1024) return fail(NTRU_ERR_UNSUPPORTED, "parameter set needs more than 160 KiB of LDS");
  L->blocks = (B + WAVES_PER_BLOCK - 1) / WAVES_PER_BLOCK;
  return NTRU_OK;
}

// Shared-stepping decrypt: two items per wave, K pairs per lane.  Returns K (9/11/13) and the mask interval, or 0.
static int shared_path_K(const ntru_engine *eng, int N, int q, int p, int *me) {
  if (eng->path == 1 || p != 3 || (N & 1) == 0) return 0;
  int K = (N + 63) / 64;
  if ((K & 1) == 0) K++;
  if (K < 9 || K > 13) return 0;
  if ((long)N * 4 >= 65536) return 0;
  long limit = 65535 / (q - 1) - 1;
  if (limit >= K) *me = K; else if (limit >= 7) *me = 7; else return 0;
  if (K == 13 && *me == 7) return 0;      // that variant does not fit 128 VGPRs without spilling: use the MAC kernels
  return K;
}

// The admitted (K, mask interval, dot8) tuples, one list per template family: VARIANT binds the constants KK, MM, DD for the
// statement and the three switches below differ in the tuples they hold and the message of their default.
#define VARIANT(Kc, Mc, Dc, ...)                                                                                           \
  case (Kc) * 1000 + (Mc) * 10 + (Dc): {                                                                                   \
    [[maybe_unused]] constexpr int KK = Kc, MM = Mc; [[maybe_unused]] constexpr bool DD = Dc; __VA_ARGS__;                 \
  } break;
#define DISPATCH_K_SHARED(Kv, MEv, D8v, ...)                                                                               \
  switch ((Kv) * 1000 + (MEv) * 10 + (D8v)) {                                                                              \
    VARIANT(13, 13, 1, __VA_ARGS__) VARIANT(13, 13, 0, __VA_ARGS__) VARIANT(11, 11, 1, __VA_ARGS__)                        \
    VARIANT(11, 11, 0, __VA_ARGS__) VARIANT(11, 7, 1, __VA_ARGS__) VARIANT(11, 7, 0, __VA_ARGS__)                          \
    VARIANT(9, 9, 0, __VA_ARGS__) VARIANT(9, 7, 0, __VA_ARGS__)                                                            \
    default: return fail(NTRU_ERR_UNSUPPORTED, "no shared-step kernel for this (K, mask interval)");                       \
  }
#define DISPATCH_K_ADD(Kv, MEv, ...)                                                                                       \
  switch ((Kv) * 1000 + (MEv) * 10) {                                                                                      \
    VARIANT(7, 14, 0, __VA_ARGS__) VARIANT(7, 7, 0, __VA_ARGS__) VARIANT(5, 10, 0, __VA_ARGS__) VARIANT(5, 5, 0, __VA_ARGS__) \
    VARIANT(3, 6, 0, __VA_ARGS__) VARIANT(3, 3, 0, __VA_ARGS__) VARIANT(1, 2, 0, __VA_ARGS__) VARIANT(1, 1, 0, __VA_ARGS__) \
    default: return fail(NTRU_ERR_UNSUPPORTED, "no add-path kernel for this (K, mask interval)");                          \
  }
#define DISPATCH_K(Kv, ...)                                                                                                \
  switch ((Kv) * 1000) {                                                                                                   \
    VARIANT(1, 0, 0, __VA_ARGS__) VARIANT(3, 0, 0, __VA_ARGS__) VARIANT(5, 0, 0, __VA_ARGS__) VARIANT(7, 0, 0, __VA_ARGS__) \
    VARIANT(9, 0, 0, __VA_ARGS__) VARIANT(11, 0, 0, __VA_ARGS__) VARIANT(13, 0, 0, __VA_ARGS__) VARIANT(15, 0, 0, __VA_ARGS__) \
    default: return fail(NTRU_ERR_UNSUPPORTED, "no kernel for this K");                                                    \
  }

int ntru_launch_encrypt_valu(ntru_engine *eng, int N, int q, const uint16_t *d_h, const uint8_t *d_r, const uint8_t *d_m, int64_t B,
                             uint16_t *d_e, uint16_t *d_quotE) {
  Launch L;
  if (const int me = add_path_me(eng, N, q, &L)) {
    if (int rc = plan_add(B, (size_t)L.g.eo_len * 8, (size_t)L.g.nl * 4, &L)) return rc;
    DISPATCH_K_ADD(L.K, me, {
      note_kernel(eng, "k_encrypt_t", KK, MM);
      return launch_resident(eng, k_encrypt_t<KK, MM>, L.blocks, BLOCK_THREADS, L.lds, L.g, (u32)q, d_h, d_r, d_m, (long)B, d_e, d_quotE);
    });
  }
  if (int rc = plan(eng, N, B, 1, false, &L)) return rc;
  DISPATCH_K(L.K, {
    note_kernel(eng, "k_encrypt", KK, -1);
    return launch_resident(eng, k_encrypt<KK>, L.blocks, BLOCK_THREADS, L.lds, L.g, (u32)q, d_h, d_r, d_m, (long)B, d_e, d_quotE);
  });
}

int ntru_launch_decrypt_valu(ntru_engine *eng, int N, int q, int p, const int8_t *d_f, const uint8_t *d_fp, const uint16_t *d_e,
                             int64_t B, uint8_t *d_value, uint16_t *d_quot1, uint16_t *d_rem1, uint8_t *d_quot2) {
  Launch L;
  {
    int me = 0;
    if (const int KS = shared_path_K(eng, N, q, p, &me)) {
      L.K = KS;
      L.g = make_geom(N, KS);
      const size_t per_wave = (size_t)L.g.G * (L.g.eo_len + 2) * 4;
      const int nblk8 = ((N + 31) >> 5) << 2;
      L.lds = (size_t)L.g.nl * 16 + (size_t)L.g.nl * KS * 8 + (size_t)nblk8 * 4 + WAVES_PER_BLOCK * per_wave;
      // product 2 on v_dot8 needs the 32-lane item layout (and is skipped when the MAC/add families are forced apart); it is
      // instantiated for K >= 11 only, so K = 9 at nl == 32 (odd N 559..575) keeps the plain second product
      const int d8 = (L.g.nl == 32 && KS >= 11 && eng->path != 3) ? 1 : 0;
      const long ngroups = (B + L.g.G - 1) / L.g.G;
      L.blocks = (ngroups + WAVES_PER_BLOCK - 1) / WAVES_PER_BLOCK;
      DISPATCH_K_SHARED(KS, me, d8, {
        note_kernel(eng, DD ? "k_decrypt_s+dot8" : "k_decrypt_s", KK, MM);
        return launch_resident(eng, k_decrypt_s<KK, MM, DD>, L.blocks, BLOCK_THREADS, L.lds, L.g, (u32)q, ntru_lift_addend(eng, q, p), d_f, d_fp, d_e, (long)B,
                               d_value, d_quot1, d_rem1, d_quot2);
      });
    }
  }
  if (const int me = (p == 3 && eng->path == 2) ? add_path_me(eng, N, q, &L) : 0) {   // per-item stepping: only when forced
    if (int rc = plan_add(B, (size_t)L.g.eo_len * 8 + (size_t)L.g.nl * 4,
                          (size_t)L.g.eo_len * 8 + (size_t)L.g.nl * 4, &L)) return rc;
    DISPATCH_K_ADD(L.K, me, {
      note_kernel(eng, "k_decrypt_t", KK, MM);
      return launch_resident(eng, k_decrypt_t<KK, MM>, L.blocks, BLOCK_THREADS, L.lds, L.g, (u32)q, (u32)p, ntru_lift_addend(eng, q, p), d_f, d_fp, d_e, (long)B, d_value,
                             d_quot1, d_rem1, d_quot2);
    });
  }
  if (int rc = plan(eng, N, B, 2, false, &L)) return rc;
  DISPATCH_K(L.K, {
    note_kernel(eng, "k_decrypt", KK, -1);
    return launch_resident(eng, k_decrypt<KK>, L.blocks, BLOCK_THREADS, L.lds, L.g, (u32)q, (u32)p, ntru_lift_addend(eng, q, p), d_f, d_fp, d_e, (long)B, d_value, d_quot1,
                           d_rem1, d_quot2);
  });
}

int ntru_launch_polymul_valu(ntru_engine *eng, int N, int mod, const uint16_t *d_a, const uint16_t *d_b, int64_t B, uint16_t *d_quot,
                             uint16_t *d_rem) {
  Launch L;
  if (int rc = plan(eng, N, B, 0, true, &L)) return rc;
  DISPATCH_K(L.K, {
    note_kernel(eng, "k_polymul_split", KK, -1);
    return launch_resident(eng, k_polymul_split<KK>, L.blocks, BLOCK_THREADS, L.lds, L.g, (u32)mod, (int)is_pow2(mod), d_a, d_b, (long)B,
                           d_quot, d_rem, 1u);
  });
}

int ntru_launch_public_key_valu(ntru_engine *eng, int N, int q, int p, const uint16_t *d_fq, const int8_t *d_g, int64_t B,
                                uint16_t *d_h) {
  Launch L;
  if (int rc = plan(eng, N, B, 0, true, &L)) return rc;
  DISPATCH_K(L.K, {
    note_kernel(eng, "k_public_key", KK, -1);
    return launch_resident(eng, k_polymul_split<KK, true>, L.blocks, BLOCK_THREADS, L.lds, L.g, (u32)q, 1, (const u16 *)d_g, d_fq, (long)B,
                           (u16 *)nullptr, d_h, (u32)p);
  });
}

int ntru_launch_verify_keys_valu(ntru_engine *eng, int N, int q, int p, const int8_t *d_f, const int8_t *d_g, const uint16_t *d_fq,
                                 const uint8_t *d_fp, const uint16_t *d_h, int64_t B, uint16_t *d_quot_fq, uint16_t *d_rem_fq,
                                 uint8_t *d_quot_fp, uint8_t *d_rem_fp, uint16_t *d_quot_h, uint16_t *d_rem_h, uint8_t *d_flags) {
  Launch L;
  if (const int me = p == 3 ? add_path_me(eng, N, q, &L) : 0) {
    const size_t raw_len = ((size_t)N + 1) & ~(size_t)1;
    if (int rc = plan_add(B, 0, (size_t)L.g.eo_len * 8 + (size_t)L.g.nl * 4 + raw_len * 2, &L)) return rc;
    DISPATCH_K_ADD(L.K, me, {
      note_kernel(eng, "k_verify_keys_t", KK, MM);
      return launch_resident(eng, k_verify_keys_t<KK, MM>, L.blocks, BLOCK_THREADS, L.lds, L.g, (u32)q, (u32)p, d_f, d_g, d_fq, d_fp, d_h,
                             (long)B, d_quot_fq, d_rem_fq, d_quot_fp, d_rem_fp, d_quot_h, d_rem_h, d_flags);
    });
  }
  if (int rc = plan(eng, N, B, 0, true, &L)) return rc;
  DISPATCH_K(L.K, {
    note_kernel(eng, "k_verify_keys", KK, -1);
    return launch_resident(eng, k_verify_keys<KK>, L.blocks, BLOCK_THREADS, L.lds, L.g, (u32)q, (u32)p, d_f, d_g, d_fq, d_fp, d_h, (long)B,
                           d_quot_fq, d_rem_fq, d_quot_fp, d_rem_fp, d_quot_h, d_rem_h, d_flags);
  });
}

