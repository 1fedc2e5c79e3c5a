// ES-module shim: the hot-path surface of numtel/ntru-circom's index.js served by the MI355X HIP engine.
//
//   import NTRU, { multiplyPolynomials, dividePolynomials, addPolynomials, ... } from './index.mjs'
//
// Same contract as the reference for the functions it covers (file:line = reference index.js):
//   * every return value is a fresh plain Array of Numbers / plain object (test/reference.test.js:60 uses
//     deepStrictEqual on a plain Array; circomkit takes number arrays as signals);
//   * inputs are never mutated; everything is synchronous; errors are `throw new Error(msg)` with the
//     reference's messages; expandArray overflow surfaces as RangeError (index.js:535);
//   * constructor options / public mutable fields N,p,q,df,dg,dr,f,fp,fq,g,h,I (index.js:9-27); one additive option, lift
//     ('reference', the default, or 'centred': see "the lift" in the class).
// All polynomial products and splits run on the GPU through the N-API addon -> C ABI (include/ntru_engine.h).
// There is no JavaScript arithmetic fallback: without the addon or a GPU the first call throws.
//
// Key generation runs on the device too (loadPrivateKeyF, generatePrivateKeyF, generateNewPublicKeyGH,
// generatePublicKeyH).  The whole export list of the reference is here (default NTRU + its 19 named functions):
// polyInv / extendedEuclideanAlgorithm / dividePolynomials by an arbitrary divisor / products modulo more than 65536 run
// on the engine's generic family (ntru_generic_*: the reference's own algorithms, one item per wavefront), which also
// serves the f that are not units, so that loadPrivateKeyF behaves like the reference there too.
import { createRequire } from 'module';
import nodeCrypto from 'crypto';
const { randomFillSync } = nodeCrypto;

const require = createRequire(import.meta.url);
let addon = null;
let engineReady = false;

function engine() {
  if (!addon) addon = require('./ntru_addon.node');       // throws if the addon was not built
  if (!engineReady) {
    addon.create(Number(process.env.NTRU_HIP_DEVICE || 0)); // throws when no GPU: no CPU fallback
    engineReady = true;
  }
  return addon;
}

export function deviceCount() {
  if (!addon) addon = require('./ntru_addon.node');
  return addon.deviceCount();
}

// ---- helpers with the reference's semantics -----------------------------------------------------------------

export function degree(poly) {                                   // index.js:210-215
  for (let i = poly.length - 1; i >= 0; i--) if (poly[i] !== 0) return i;
  return -1;
}

export function trimPolynomial(poly) {                           // index.js:218-221
  const d = degree(poly);
  return d >= 0 ? Array.prototype.slice.call(poly, 0, d + 1) : [0];
}

export function expandArray(arr, len, fill) {                    // index.js:534-536 (RangeError when too long)
  return [...arr, ...Array(len - arr.length).fill(fill)];
}

export function expandArrayToMultiple(array, multiple) {         // index.js:516-532 (mutates, like the reference)
  if (!Array.isArray(array)) throw new Error('First argument must be an array.');
  if (typeof multiple !== 'number' || multiple <= 0 || !Number.isInteger(multiple))
    throw new Error('Multiple must be a positive integer.');
  const target = Math.ceil(array.length / multiple) * multiple;
  while (array.length < target) array.push(0);
  return array;
}

export function addPolynomials(a, b, p) {                        // index.js:235-244 (O(N) host glue)
  const n = Math.max(a.length, b.length), out = [];
  for (let i = 0; i < n; i++) out[i] = (((i < a.length ? a[i] : 0) + (i < b.length ? b[i] : 0)) % p + p) % p;
  return trimPolynomial(out);
}

export function stringToBits(str) {                              // index.js:538-546
  const bits = [];
  for (let i = 0; i < str.length; i++)
    for (const c of str.charCodeAt(i).toString(2).padStart(8, '0')) bits.push(Number(c));
  return bits;
}

export function bitsToString(bits) {                             // index.js:548-556
  let s = '';
  for (let i = 0; i < bits.length; i += 8) s += String.fromCharCode(parseInt(bits.slice(i, i + 8).join(''), 2));
  return s;
}

// index.js:461-488: exactly length-1 draws, i descending, j = u32 % (i+1).  Uses WebCrypto when the host
// provides it (so a seeded shim replays the reference bit for bit) and node's CSPRNG otherwise.
export function generateCustomArray(length, numOnes, numNegOnes) {
  if (numOnes + numNegOnes > length) throw new Error('The total of 1s and -1s cannot exceed the array length.');
  const array = new Array(length).fill(0);
  array.fill(1, 0, numOnes);
  array.fill(-1, numOnes, numOnes + numNegOnes);
  // The reference draws one u32 per step from the global WebCrypto (index.js:481-482).  A WebCrypto the CALLER installed
  // (e.g. a seeded one, to replay) is called exactly like that.  Node's own CSPRNG -- no global at all (Node 12), or the
  // built-in global of Node >= 19, which IS crypto.webcrypto -- delivers the length - 1 draws in ONE call: same count, same
  // distribution, ~0.4 ms less per encryptBits at N = 821 (length - 1 <= 16384 draws stay under WebCrypto's 65536-byte quota).
  const g = typeof globalThis !== 'undefined' && globalThis.crypto && globalThis.crypto.getRandomValues ? globalThis.crypto : null;
  const builtin = g !== null && nodeCrypto.webcrypto !== undefined && g === nodeCrypto.webcrypto;
  const perStep = g !== null && !builtin;
  const u = new Uint32Array(perStep || length < 2 ? 1 : length - 1);
  if (!perStep && length > 1) {
    if (builtin && u.byteLength <= 65536) g.getRandomValues(u); else randomFillSync(u);
  }
  for (let i = length - 1, k = 0; i > 0; i--, k++) {
    if (perStep) g.getRandomValues(u);
    const j = u[perStep ? 0 : k] % (i + 1);
    const t = array[i]; array[i] = array[j]; array[j] = t;
  }
  return array;
}

const mod = (x, p) => ((x % p) + p) % p;

// ---- the reference's remaining O(N) helpers (host glue, like addPolynomials) ------------------------------------

export function modInverse(a, p) {                               // index.js:224-232
  a = ((a % p) + p) % p;
  for (let x = 1; x < p; x++) if ((a * x) % p === 1) return x;
  return null;
}

export function subtractPolynomials(a, b, p) {                   // index.js:247-256
  const n = Math.max(a.length, b.length), out = [];
  for (let i = 0; i < n; i++) out[i] = (((i < a.length ? a[i] : 0) - (i < b.length ? b[i] : 0)) % p + p) % p;
  return trimPolynomial(out);
}

export function multiplyPolynomialsByScalar(poly, scalar, p) {   // index.js:404-406
  return poly.map(coeff => (coeff * scalar) % p);
}

export function bigintToBits(bigint) {                           // index.js:558-566
  const bits = [];
  while (bigint > 0n) { bits.push(Number(bigint & 1n)); bigint >>= 1n; }
  return bits;
}

export function bitsToBigInt(bits) { return BigInt(`0b${bits.join('')}`); }   // index.js:568-570

// ---- generic family of the engine (include/ntru_engine.h, ntru_generic_*): one item, JS Numbers in and out --------
const GENERIC_ERRORS = [null, 'Cannot divide by zero polynomial.', 'No inverse exists for division.', 'invalid_gcd',
  'ntru engine: generic work area exhausted'];
const REFERENCE_KEYGEN_ERRORS = new Set(['invalid_gcd', 'invalid fq', 'invalid fp', GENERIC_ERRORS[1], GENERIC_ERRORS[2]]);

function genericOp(op, a, b, mod) {
  const A = Float64Array.from(a), Bv = Float64Array.from(b);
  const cap = engine().genericCapacity(A.length, Bv.length);
  const o0 = new Float64Array(cap), o1 = op === 1 || op === 2 ? new Float64Array(cap) : null;
  const [status, len0, len1] = engine().genericOp(op, A, Bv, mod, o0, o1);
  if (status) throw new Error(GENERIC_ERRORS[status]);
  return [Array.from(o0.subarray(0, len0)), o1 ? Array.from(o1.subarray(0, len1)) : null];
}

const isI = (b, p) => {                                           // b = [1, 0, ..., 0, -1] (or p-1) of length N+1 >= 2
  const N = b.length - 1;
  if (N < 1 || mod(b[0], p) !== 1 || mod(b[N], p) !== p - 1) return false;
  for (let i = 1; i < N; i++) if (mod(b[i], p) !== 0) return false;
  return true;
};
const fastModulus = (N, p) => Number.isInteger(p) && p >= 2 &&
  ((p & (p - 1)) === 0 ? p <= 65536 : N * (p - 1) * (p - 1) < 65536);

// index.js:425-459 -> { gcd, inverse }
export function extendedEuclideanAlgorithm(a, b, p) {
  const [gcd, inverse] = genericOp(2, a, b, p);
  return { gcd, inverse };
}

// index.js:491-514.  The key-generation case -- ternary f, polyI = 1 - x^N, modulus 3 or a power of two -- runs on the
// batched inversion kernels (k_invert_key + Newton rounds on the matrix cores); the inverse of a unit is unique, so that
// is the reference's result.  Everything else, and every f those kernels flag as a non-unit, goes through the generic
// family, which follows the reference step by step (and throws what it throws).
export function polyInv(polyIn, polyI, polyMod) {
  const N = polyI.length - 1;
  const ternary = polyIn.length <= N && polyIn.every(x => x === 0 || x === 1 || x === -1);
  const pow2 = Number.isInteger(polyMod) && polyMod >= 2 && polyMod <= 65536 && (polyMod & (polyMod - 1)) === 0;
  if (ternary && N >= 2 && N <= 1920 && (polyMod === 3 || pow2) && polyI[0] === 1 && polyI[N] === -1 &&
      polyI.every((x, i) => i === 0 || i === N || x === 0)) {
    const f = Int8Array.from(expandArray(polyIn, N, 0)), flags = new Uint8Array(1);
    if (polyMod === 3) {
      const fp = new Uint8Array(N);
      engine().invertKeyBatch(N, 2, 3, f, 1, null, fp, flags);
      if (!(flags[0] & 16)) return trimPolynomial(Array.from(fp));
    } else {
      const fq = new Uint16Array(N);
      engine().invertKeyBatch(N, polyMod, 3, f, 1, fq, null, flags);
      if (!(flags[0] & 8)) return trimPolynomial(Array.from(fq));
    }
  }
  return genericOp(3, polyIn, polyI, polyMod)[0];
}

// index.js:319-355: linear product, coefficients into [0,p), trimmed.  One GPU polymul-split in a ring that
// holds both operands; c[N+k] = -quot[k], c[k] = rem[k] - c[N+k].  Moduli the packed kernels do not take (above 65536,
// e.g. the 2^20 of test/circuits.test.js:72) run on the generic family.
export function multiplyPolynomials(a, b, p) {
  if (a.length === 0 || b.length === 0) return [0];
  const N = Math.max(a.length, b.length, 2);
  if (!fastModulus(N, p)) return genericOp(0, a, b, p)[0];
  const A = new Uint16Array(N), Bv = new Uint16Array(N), quot = new Uint16Array(N), rem = new Uint16Array(N);
  for (let i = 0; i < a.length; i++) A[i] = mod(a[i], p);
  for (let i = 0; i < b.length; i++) Bv[i] = mod(b[i], p);
  engine().polymulSplit(N, p, A, Bv, 1, quot, rem);
  const out = new Array(2 * N - 1);
  for (let k = 0; k < N; k++) {
    const hi = (p - quot[k]) % p;
    out[k] = mod(rem[k] - hi, p);
    if (k < N - 1) out[N + k] = hi;
  }
  return trimPolynomial(out);
}

// index.js:358-401.  The hot path's divisor b = I = 1 - x^N with a reduced dividend is the closed-form split kernel;
// any other divisor (or an unreduced dividend) is long division on the generic family.
export function dividePolynomials(a, b, p) {
  if (degree(b) === -1) throw new Error('Cannot divide by zero polynomial.');
  const N = b.length - 1;
  if (!(Number.isInteger(p) && p >= 2 && p <= 65536 && isI(b, p) && a.length <= 2 * N &&
        a.every(x => Number.isInteger(x) && x >= 0 && x < p))) {
    const [quotient, remainder] = genericOp(1, a, b, p);
    return { quotient, remainder };
  }
  const A = new Uint16Array(2 * N), quot = new Uint16Array(N), rem = new Uint16Array(N);
  A.set(a);
  engine().splitByI(N, p, A, 1, quot, rem);
  const nq = Math.max(a.length - N, 0);
  return {
    quotient: nq ? trimPolynomial(Array.from(quot.subarray(0, nq))) : [0],
    remainder: trimPolynomial(Array.from(rem)),
  };
}

// addPolynomials on the GPU for reduced operands (the homomorphic sum of test/reference.test.js:46-61).
export function addCiphertexts(e1, e2, q) {
  const N = Math.max(e1.length, e2.length, 1);
  const A = new Uint16Array(N), Bv = new Uint16Array(N), out = new Uint16Array(N);
  A.set(e1); Bv.set(e2);
  engine().addBatch(N, q, A, Bv, 1, out);
  return trimPolynomial(Array.from(out));
}

// The groups of a sum over B rows: offsets (Array or BigInt64Array of G + 1 row indices) or null for ONE group of every row.
function tallyGroups(offsets, B) {
  if (offsets == null) return { off: null, K: Math.max(B, 1), G: B > 0 ? 1 : 0 };
  const off = offsets instanceof BigInt64Array ? offsets : BigInt64Array.from(Array.from(offsets), x => BigInt(x));
  if (off.length < 1) throw new TypeError('offsets must hold G + 1 row indices');
  return { off, K: 0, G: off.length - 1 };
}

// The homomorphic sum of many ciphertexts in one device pass: addPolynomials folded over every group of `rows` (arrays of coefficients in
// [0, q)), each row first scaled by its weight as multiplyPolynomialsByScalar does.  offsets null: one group, returns the trimmed sum;
// else an Array of them, group g = rows[offsets[g] .. offsets[g + 1]).
export function sumCiphertexts(rows, q, offsets = null, weights = null) {
  const B = rows.length;
  const N = Math.max(2, ...rows.map(r => r.length));
  const flat = new Uint16Array(B * N);
  rows.forEach((r, b) => flat.set(r, b * N));
  const w = weights ? Uint16Array.from(weights, x => ((x % q) + q) % q) : null;
  const { off, K, G } = tallyGroups(offsets, B);
  const out = new Uint16Array(G * N);
  engine().sumGroups(N, q, flat, w, off, K, G, B, out);
  const sums = Array.from({ length: G }, (_, g) => trimPolynomial(Array.from(out.subarray(g * N, (g + 1) * N))));
  return offsets == null ? sums[0] : sums;
}

// The weight matrix of a combination, row b = the G weights of ciphertext b: an Array of B arrays of G numbers, or a Uint16Array[B * G]
// with G.  -> { w: Uint16Array[B * G] reduced below q, G }
function combineWeights(weights, B, G, q) {
  if (!(weights instanceof Uint16Array)) {
    const rows = Array.from(weights, r => Array.from(r));
    if (rows.length !== B) throw new TypeError(`combine: ${rows.length} rows of weights for ${B} rows`);
    G = rows.length ? rows[0].length : G;
    if (rows.some(r => r.length !== G)) throw new TypeError('combine: every row of weights must hold G weights');
    weights = Uint16Array.from(rows.flat(), x => ((x % q) + q) % q);
  }
  if (!Number.isInteger(G) || G < 1 || G > 4096) throw new RangeError('combine: need 1 <= G <= 4096');
  if (weights.length !== B * G) throw new TypeError(`combine: weights must hold B * G = ${B * G} values`);
  return { w: weights, G };
}

// out[g] = (sum over b of w[b * G + g] * rows[b]) mod q for the dense rows flat: Uint16Array[B * N] -> Uint16Array[G * N].  Composed from
// sumGroups, one weighted sum of ONE group per output column: the same bytes as the engine's ntru_combine_batch, which reads the rows
// once, but not that call (INTEGRATION.md, "Combining ciphertexts"): from Node this is correct, not fast.
function combineRows(N, q, flat, B, w, G) {
  const out = new Uint16Array(G * N), col = new Uint16Array(B), one = new Uint16Array(N);
  for (let g = 0; g < G && B > 0; g++) {
    for (let b = 0; b < B; b++) col[b] = w[b * G + g];
    engine().sumGroups(N, q, flat, col, null, B, 1, B, one);
    out.set(one, g * N);
  }
  return out;
}

// G linear combinations of the same ciphertexts: weights[b] holds the G weights of rows[b] (or weights: Uint16Array[B * G] and G), and
// combination g is addPolynomials folded over every row scaled by weights[b][g] as multiplyPolynomialsByScalar does.  Returns the G
// trimmed sums; entry g is sumCiphertexts(rows, q, null, column g of weights).
export function combineCiphertexts(rows, q, weights, G = null) {
  const B = rows.length;
  const N = Math.max(2, ...rows.map(r => r.length));
  const flat = new Uint16Array(B * N);
  rows.forEach((r, b) => flat.set(r, b * N));
  const m = combineWeights(weights, B, G, q);
  const out = combineRows(N, q, flat, B, m.w, m.G);
  return Array.from({ length: m.G }, (_, g) => trimPolynomial(Array.from(out.subarray(g * N, (g + 1) * N))));
}

// B rows, rows: Uint16Array[B * N], times the ONE polynomial poly (numbers of any sign, at most N of them) modulo (x^N - 1, q): row b is
// dividePolynomials(multiplyPolynomials(row b, poly, q), I, q).  -> the remainders Uint16Array[B * N], or { quotient, remainder } with
// wantQuot.  Composed from polymulSplit with poly repeated per row: the same bytes as the engine's ntru_mul_shared_batch, which keeps poly
// as one Toeplitz matrix on the matrix cores, but not that call (INTEGRATION.md, "Multiplying by a shared polynomial"): from Node this is
// correct, not fast.  On ciphertexts the product multiplies the noise by the 1-norm of poly.
export function multiplyByPolynomialBatch(rows, N, q, B, poly, wantQuot = false) {
  if (poly.length > N) throw new RangeError('Invalid array length');
  if (!(rows instanceof Uint16Array) || rows.length !== B * N) throw new TypeError(`multiplyByPolynomialBatch: rows must be a Uint16Array of B * N = ${B * N} values`);
  const s = new Uint16Array(B * N), quot = new Uint16Array(B * N), rem = new Uint16Array(B * N);
  if (B > 0) {
    for (let i = 0; i < poly.length; i++) s[i] = mod(poly[i], q);
    for (let b = 1; b < B; b++) s.copyWithin(b * N, 0, N);
    engine().polymulSplit(N, q, rows, s, B, quot, rem);
  }
  return wantQuot ? { quotient: quot, remainder: rem } : rem;
}

// Rows of packOutput(q - 1, N, e) field elements, BigUint64Array[B * outputSize * 4] -> the dense rows Uint16Array[B * N]: unpackInput of
// every row with the pad dropped, whatever the pad and the bits above an element's fields hold.
function unpackRows(N, q, packed, B) {
  const [bits, per, , outputSize] = engine().packParams(q - 1, N);
  const wide = new Uint16Array(B * outputSize * per), dense = new Uint16Array(B * N);
  if (B) engine().unpackBatch(q - 1, per * bits, packed, outputSize, B, wide);
  for (let b = 0; b < B; b++) dense.set(wide.subarray(b * outputSize * per, b * outputSize * per + N), b * N);
  return dense;
}

// sumCiphertexts on B ciphertexts in the circuits' wire format (packed as above; weights: Array or Uint16Array of B, or null): the sums
// of the groups as ONE dense Uint16Array[G * N], not trimmed.  Composed from unpackBatch and sumGroups: the same results as the engine's
// ntru_sum_groups_packed, which reads the packed rows once, but not that call (INTEGRATION.md, "Packed ciphertexts").
export function sumPackedCiphertexts(packed, N, q, B, offsets = null, weights = null) {
  const w = weights ? Uint16Array.from(weights, x => ((x % q) + q) % q) : null;
  const { off, K, G } = tallyGroups(offsets, B);
  const out = new Uint16Array(G * N);
  engine().sumGroups(N, q, unpackRows(N, q, packed, B), w, off, K, G, B, out);
  return out;
}

const limbsToBigInt = (l, at) => l[at] | (l[at + 1] << 64n) | (l[at + 2] << 128n) | (l[at + 3] << 192n);

// index.js:572-596 on the GPU: same object as the reference (`expected` is an Array of BigInt).
export function packOutput(maxVal, dataLen, data) {
  const [maxInputBits, numInputsPerOutput, arrLen, outputSize] = engine().packParams(maxVal, dataLen);
  const inArr = Uint16Array.from(expandArray(data, dataLen, 0));
  const limbs = new BigUint64Array(outputSize * 4);
  engine().packBatch(maxVal, dataLen, inArr, 1, limbs);
  const expected = [];
  for (let o = 0; o < outputSize; o++) expected.push(limbsToBigInt(limbs, 4 * o));
  return { maxInputBits, maxOutputBits: numInputsPerOutput * maxInputBits, outputSize, arrLen, expected };
}

// index.js:598-620 on the GPU (`data`: Array of BigInt below 2^256).
export function unpackInput(maxVal, packedBits, data) {
  const [maxInputBits] = engine().packParams(maxVal, 0);
  const per = Math.floor(packedBits / maxInputBits);
  const limbs = new BigUint64Array(data.length * 4);
  const M = (1n << 64n) - 1n;
  data.forEach((v, i) => { for (let k = 0; k < 4; k++) limbs[4 * i + k] = (v >> BigInt(64 * k)) & M; });
  const out = new Uint16Array(per * data.length);
  if (data.length) engine().unpackBatch(maxVal, packedBits, limbs, data.length, 1, out);
  return { maxInputBits, packedBits, packedSize: data.length, unpackedSize: per * data.length,
    unpacked: trimPolynomial(Array.from(out)) };
}

const withZero = ta => { const a = Array.from(ta); a.push(0); return a; };

export default class NTRU {
  constructor(options) {
    Object.assign(this, {                                        // index.js:9-23
      N: 167, p: 3, q: 128, df: 61, dg: 20, dr: 18, f: null, fp: null, fq: null, g: null, h: null,
    }, options);
    this.I = (new Array(this.N + 1)).fill(0);                    // index.js:25-27
    this.I[0] = 1;
    this.I[this.I.length - 1] = -1;
    if (this.lift !== undefined && this.lift !== 'reference' && this.lift !== 'centred') {
      throw new Error(`lift: unknown mode ${String(this.lift)} ('reference' or 'centred')`);
    }
  }

  // ---- the lift (additive; INTEGRATION.md "The lift").  new NTRU({..., lift: 'centred'}) decrypts with the true centred lift,
  // x > q/2 ? (x - q) mod p : x % p, in place of index.js:117's x > q/2 ? (x + 1) % p : x % p, which returns the plaintext only where
  // -q = 1 (mod p) -- not at q = 4096 with p = 3, nor at almost any q with p = 5 or 7.  Without the option (or with 'reference') every
  // method below runs exactly what it ran before the option existed.  The engine's ntru_engine_set_lift has no export in the addon yet
  // (its export list is fixed), so the centred mode is composed here from existing exports: the first stage with the witness on
  // (remainder1 does not depend on the lift), the lift on typed arrays in JavaScript, c = fp b through polymulSplit(N, p, ...) with fp
  // repeated per row.  decryptBits, decryptStr, decryptBatch and tallyBatch do that; the forms that cannot be composed this way throw.
  get _centred() { return this.lift === 'centred'; }
  _refuseCentred(name) {
    if (this._centred) throw new Error(`${name}: not available with the option lift: 'centred' (the addon exports no native path for it yet)`);
  }
  // remainder1 rows Uint16Array[B*N] -> { value, quotient2 } of the centred b, Uint8Array[B*N] each
  _centredSecondStage(r1, B) {
    const { N, p, q } = this, add = (p - q % p) % p;
    const fp = expandArray(this.fp, N, 0);
    const b = new Uint16Array(B * N), fpRows = new Uint16Array(B * N);
    for (let i = 0; i < B * N; i++) { const x = r1[i]; b[i] = 2 * x > q ? (x + add) % p : x % p; }   // strict >, like index.js:117
    for (let r = 0; r < B; r++) fpRows.set(fp, r * N);
    const quot = new Uint16Array(B * N), rem = new Uint16Array(B * N);
    engine().polymulSplit(N, p, fpRows, b, B, quot, rem);
    return { value: Uint8Array.from(rem), quotient2: Uint8Array.from(quot) };
  }

  calculateNq() { return Math.ceil(Math.log2(this.q * this.q * this.N)); }   // index.js:201-203
  calculateNp() { return Math.ceil(Math.log2(this.p * this.p * this.N)); }   // index.js:204-206

  encryptStr(inputPlain) { return this.encryptBits(stringToBits(inputPlain)).value; }               // :80-83
  decryptStr(encrypted) { return bitsToString(expandArrayToMultiple(this.decryptBits(encrypted).value, 8)); } // :84-86

  encryptBits(m) {                                               // index.js:87-110
    const { N, p, q } = this;
    const r = generateCustomArray(N, this.dr, this.dr).map(x => x === -1 ? p - 1 : x);
    const mPad = expandArray(m, N, 0), hPad = expandArray(this.h, N, 0);
    // addPolynomials(m, rhq, q) reduces any integer m[i] modulo q (index.js:91, :241); the device adds a byte, and
    // (m mod q) mod 256 is the same residue modulo q whenever q divides 256 -- otherwise m mod q must fit the byte.
    const mDev = Uint8Array.from(mPad, x => { const v = mod(x, q); return q <= 256 ? v : v & 255; });
    if (q > 256 && mPad.some(x => mod(x, q) > 255)) return this.encryptBitsWide(m, r, mPad, hPad);
    const e = new Uint16Array(N), quot = new Uint16Array(N);
    engine().encryptBatch(N, q, Uint16Array.from(hPad), Uint8Array.from(r), mDev, 1, e, quot);
    return {
      value: trimPolynomial(Array.from(e)),
      inputs: { r, m: mPad, h: hPad, quotientE: withZero(quot), remainderE: withZero(e) },
      params: [q, this.calculateNq(), N],
    };
  }

  // Plaintext coefficients that do not fit the kernel's byte operand (the reference accepts any integer): the same
  // three steps as index.js:90-92 as separate engine calls.
  encryptBitsWide(m, r, mPad, hPad) {
    const { N, q } = this;
    const rhqm = addPolynomials(m, multiplyPolynomials(r, this.h, q), q);
    const { quotient, remainder } = dividePolynomials(rhqm, this.I, q);
    return {
      value: trimPolynomial(remainder),
      inputs: { r, m: mPad, h: hPad, quotientE: expandArray(quotient.map(x => x % q), N + 1, 0),
        remainderE: expandArray(remainder, N + 1, 0) },
      params: [q, this.calculateNq(), N],
    };
  }

  decryptBits(e) {                                               // index.js:111-140
    const { N, p, q } = this;
    const f = this.f.map(x => x === -1 ? q - 1 : x);             // TypeError when f is null, like the reference
    const ePad = expandArray(e, N, 0), fpPad = expandArray(this.fp, N, 0);
    let value = new Uint8Array(N), q2 = new Uint8Array(N);
    const q1 = new Uint16Array(N), r1 = new Uint16Array(N);
    engine().decryptBatch(N, q, p, Int8Array.from(expandArray(this.f, N, 0)), Uint8Array.from(fpPad),
      Uint16Array.from(ePad), 1, value, q1, r1, q2);
    if (this._centred) ({ value, quotient2: q2 } = this._centredSecondStage(r1, 1));
    return {
      value: trimPolynomial(Array.from(value)),
      inputs: {
        f: expandArray(f, N, 0), fp: fpPad, e: ePad,
        quotient1: withZero(q1), remainder1: withZero(r1), quotient2: withZero(q2), remainder2: withZero(value),
      },
      params: [q, this.calculateNq(), p, this.calculateNp(), N],
    };
  }

  // index.js:30-49.  Units (every f a key generator ends up with) take the batched inversion kernels: fq and fp are
  // unique, so they are the reference's, and its validity checks pass by construction.  For an f those kernels flag,
  // the reference's own sequence runs on the generic family: same assignments in the same order, same throws, same
  // acceptance of the non-units its `&&` checks let through (index.js:41-45, :451).
  loadPrivateKeyF(fArr) {
    const { N, p, q } = this;
    const ternary = fArr.length <= N && fArr.every(x => x === 0 || x === 1 || x === -1);
    if (ternary && p === 3 && N >= 2 && N <= 1920 && fastModulus(N, q) && (q & (q - 1)) === 0) {   // the engine's N range, as in polyInv
      const fq = new Uint16Array(N), fp = new Uint8Array(N), flags = new Uint8Array(1);
      engine().invertKeyBatch(N, q, p, Int8Array.from(expandArray(fArr, N, 0)), 1, fq, fp, flags);
      if (!(flags[0] & 24)) {
        this.f = fArr;
        this.fq = trimPolynomial(Array.from(fq));
        this.fp = trimPolynomial(Array.from(fp));
        return true;
      }
    }
    this.f = fArr;
    this.fq = polyInv(this.f, this.I, q);
    this.fp = polyInv(this.f, this.I, p);
    const fmodq = this.f.map(x => x === -1 ? q - 1 : x), fmodp = this.f.map(x => x === -1 ? p - 1 : x);
    const fqDiv = dividePolynomials(multiplyPolynomials(this.fq, fmodq, q), this.I, q);
    if (fqDiv.remainder.length !== 1 && fqDiv.remainder[0] !== 1) throw new Error('invalid fq');
    const fpDiv = dividePolynomials(multiplyPolynomials(this.fp, fmodp, p), this.I, p);
    if (fpDiv.remainder.length !== 1 && fpDiv.remainder[0] !== 1) throw new Error('invalid fp');
    return true;
  }

  generatePrivateKeyF() {                                        // index.js:51-65
    const maxTries = 100;
    let i = 0, retval;
    while ((!retval || !(this.fq && this.fp)) && i++ < maxTries) {
      try {
        retval = this.loadPrivateKeyF(generateCustomArray(this.N, this.df, this.df - 1));
      } catch (error) {
        // the reference swallows everything here; only what IT can throw means "try the next f" -- an engine, addon
        // or GPU failure must surface instead of ending as 'Could not find invertible f'
        if (!REFERENCE_KEYGEN_ERRORS.has(error.message)) throw error;
      }
    }
    if (!this.fq || !this.fp) throw new Error('Could not find invertible f');
  }

  generateNewPublicKeyGH() {                                     // index.js:67-70
    this.g = generateCustomArray(this.N, this.dg, this.dg);
    this.generatePublicKeyH();
  }

  generatePublicKeyH() {                                         // index.js:72-79
    if (!this.f) throw new Error('missing private key F');
    if (!this.g) throw new Error('missing private key G');
    const { N, p, q } = this;
    const h = new Uint16Array(N);
    engine().publicKeyBatch(N, q, p, Uint16Array.from(expandArray(this.fq, N, 0)), Int8Array.from(expandArray(this.g, N, 0)), 1, h);
    this.h = trimPolynomial(Array.from(h));
  }

  verifyKeysInputs() {                                           // index.js:141-197
    if (!this.f) throw new Error('missing private key F');
    if (!this.fq) throw new Error('missing private key Fq');
    if (!this.fp) throw new Error('missing private key Fp');
    if (!this.g) throw new Error('missing private key G');
    if (!this.h) throw new Error('missing public key H');
    const { N, p, q } = this;
    const nq = this.calculateNq(), np = this.calculateNp();
    const pad = a => expandArray(a, N, 0);
    const out = {
      qfq: new Uint16Array(N), rfq: new Uint16Array(N), qfp: new Uint8Array(N), rfp: new Uint8Array(N),
      qh: new Uint16Array(N), rh: new Uint16Array(N), flags: new Uint8Array(1),
    };
    engine().verifyKeysBatch(N, q, p, Int8Array.from(pad(this.f)), Int8Array.from(pad(this.g)),
      Uint16Array.from(pad(this.fq)), Uint8Array.from(pad(this.fp)), Uint16Array.from(pad(this.h)), 1,
      out.qfq, out.rfq, out.qfp, out.rfp, out.qh, out.rh, out.flags);
    if (out.flags[0] & 1) throw new Error('invalid fq');
    if (out.flags[0] & 2) throw new Error('invalid fp');
    const remH = trimPolynomial(Array.from(out.rh));            // index.js:165 walks h exactly as stored
    if (this.h.reduce((bad, cur, index) => bad || remH[index] !== cur, false)) throw new Error('invalid h');
    return {
      fq: { params: [q, nq, N], inputs: { f: pad(this.f.map(x => x === -1 ? q - 1 : x)), fq: pad(this.fq),
        quotientI: withZero(out.qfq), remainderI: withZero(out.rfq) } },
      fp: { params: [p, np, N], inputs: { f: pad(this.f.map(x => x === -1 ? p - 1 : x)), fq: pad(this.fp),
        quotientI: withZero(out.qfp), remainderI: withZero(out.rfp) } },
      h: { params: [q, nq, N], inputs: { f: pad(this.g.map(x => x === -1 ? q - 1 : x)), fq: pad(this.fq.map(x => x * p)),
        quotientI: withZero(out.qh), remainderI: withZero(out.rh) } },
    };
  }

  // ---- additive batch API (typed arrays, fixed stride N; see include/ntru_engine.h for the layout) -----------
  // Page-locked typed arrays (ntru_host_alloc): the batch calls DMA straight from / to them, no staging copy.
  // NTRU.useDevices([0, 1, ...]): encryptBatch / decryptBatch / verifyKeysInputs batches are cut into contiguous shards, one
  // engine + host thread per listed device (ntru_multi_*); [] goes back to the single device.  Returns the engine count.
  static useDevices(ids) { return engine().useDevices(Int32Array.from(ids)); }
  static allocUint8(n) { return new Uint8Array(engine().allocPinned(n), 0, n); }
  static allocUint16(n) { return new Uint16Array(engine().allocPinned(2 * n), 0, n); }

  // r: Uint8Array[B*N] in {0,1,2}, m: Uint8Array[B*N]  ->  { e, quotientE } as Uint16Array[B*N]
  // `out` may carry preallocated result arrays (e.g. from NTRU.allocUint16, which are page-locked and DMA'd in place).
  encryptBatch(r, m, B, wantWitness = true, out = {}) {
    const { N, q } = this;
    const e = out.e || new Uint16Array(B * N), quot = wantWitness ? (out.quotientE || new Uint16Array(B * N)) : null;
    engine().encryptBatch(N, q, Uint16Array.from(expandArray(this.h, N, 0)), r, m, B, e, quot);
    return { e, quotientE: quot };
  }

  // ---- one mix step (additive): re-randomises ciphertexts under h and optionally reorders them -- encryptBits (index.js:87-110) with
  // the old ciphertext in the place of m.  e: Uint16Array[Bin*N] (any value, reduced mod q), r: Uint8Array[B*N] in {0,1,2}, src: B row
  // indices into e (Array or BigInt64Array; repeats allowed; null: row i, B <= Bin) -> { e, quotientE, m } as Uint16Array[B*N]: output
  // row i is (Enc(0; r[i]) + e[src[i]]) mod q, quotientE that of Enc(0; r[i]), m the gathered rows: {r, m, h, quotientE, remainderE: e}
  // satisfies VerifyEncrypt (circuits/ntru.circom:188-208).  Composed here from encryptBatch on a zero message and addBatch, with the
  // gather on the typed arrays; the bytes are those of the engine's fused ntru_reencrypt_batch, which has no native Node path yet.
  reencryptBatch(e, r, B, src = null, wantWitness = true, out = {}) {
    const { N, q } = this;
    const Bin = e.length / N;
    if (!Number.isInteger(Bin)) throw new RangeError('reencryptBatch: e is not a whole number of rows');
    if (r.length !== B * N) throw new RangeError('reencryptBatch: r must hold B rows');
    if (src == null && B > Bin) throw new RangeError('reencryptBatch: without src, B must not exceed the rows of e');
    if (src != null && src.length !== B) throw new RangeError('reencryptBatch: src must hold B indices');
    const m = new Uint16Array(B * N);
    for (let i = 0; i < B; i++) {
      const s = src == null ? i : Number(src[i]);
      if (!Number.isInteger(s) || s < 0 || s >= Bin) throw new RangeError(`reencryptBatch: src[${i}] = ${s} is outside the rows of e`);
      const row = e.subarray(s * N, (s + 1) * N);
      for (let k = 0; k < N; k++) m[i * N + k] = row[k] & (q - 1);
    }
    const zero = this.encryptBatch(r, new Uint8Array(B * N), B, wantWitness, { quotientE: out.quotientE });
    const sum = out.e || new Uint16Array(B * N);
    if (B > 0) engine().addBatch(N, q, zero.e, m, B, sum);
    return { e: sum, quotientE: zero.quotientE, m };
  }

  // r for B encryptions drawn on the GPU: generateCustomArray(N, dr, dr) with -1 -> p-1 (index.js:89) on the ChaCha20
  // stream of `key` (Uint32Array[8]) for item indices firstItem .. firstItem+B-1; replayable on any host.
  // NTRU.samplerRounds(rounds): 20 (ChaCha20 as in RFC 8439, the default), 12 or 8 rounds of the block function behind sampleR and the
  // sampler stage of pipeline(); returns the count in force (no argument: only reads it).  Additive: the reference has no such knob because
  // its draws come from crypto.getRandomValues; generateCustomArray's shuffle and `u32 % (i + 1)` reduction are unchanged.
  static samplerRounds(rounds = 0) { return engine().setSamplerRounds(rounds); }

  sampleR(key, firstItem, B) {
    const r = new Uint8Array(B * this.N);
    engine().sampleTernary(this.N, this.dr, this.dr, this.p - 1, key, firstItem, B, r);
    return r;
  }

  // e: Uint16Array[B*N] -> { value, quotient1, remainder1, quotient2 }
  decryptBatch(e, B, wantWitness = true, out = {}) {
    const { N, p, q } = this;
    if (this._centred) return this._decryptBatchCentred(e, B, wantWitness, out);
    const value = out.value || new Uint8Array(B * N);
    const q1 = wantWitness ? (out.quotient1 || new Uint16Array(B * N)) : null;
    const r1 = wantWitness ? (out.remainder1 || new Uint16Array(B * N)) : null;
    const q2 = wantWitness ? (out.quotient2 || new Uint8Array(B * N)) : null;
    engine().decryptBatch(N, q, p, Int8Array.from(expandArray(this.f, N, 0)), Uint8Array.from(expandArray(this.fp, N, 0)),
      e, B, value, q1, r1, q2);
    return { value, quotient1: q1, remainder1: r1, quotient2: q2 };
  }

  _decryptBatchCentred(e, B, wantWitness, out) {
    const { N, p, q } = this;
    const scratch = new Uint8Array(B * N), q1 = out.quotient1 || new Uint16Array(B * N), r1 = out.remainder1 || new Uint16Array(B * N);
    engine().decryptBatch(N, q, p, Int8Array.from(expandArray(this.f, N, 0)), Uint8Array.from(expandArray(this.fp, N, 0)),
      e, B, scratch, q1, r1, null);
    const second = this._centredSecondStage(r1, B);
    const keep = (given, got) => { if (!given) return got; given.set(got); return given; };
    const value = keep(out.value, second.value);
    if (!wantWitness) return { value, quotient1: null, remainder1: null, quotient2: null };
    return { value, quotient1: q1, remainder1: r1, quotient2: keep(out.quotient2, second.quotient2) };
  }

  // ---- tallies (additive): sums the ciphertexts rows: Uint16Array[B*N] in groups (offsets: G + 1 row indices, BigInt64Array or Array;
  // null: one group of every row), each row scaled by its weight (Uint16Array[B] below q, or null), and decrypts every sum.
  // -> { sum, value, quotient1, remainder1, quotient2 }, [G*N] each: row g is what decryptBatch returns for sum row g.
  tallyBatch(rows, B, offsets = null, weights = null, wantWitness = true) { return this._tally(rows, B, offsets, weights, wantWitness, false); }
  // The same on a libuv worker thread: a Promise of the same object; the arrays must be left alone until it settles.
  tallyBatchAsync(rows, B, offsets = null, weights = null, wantWitness = true) { return this._tally(rows, B, offsets, weights, wantWitness, true); }
  _tally(rows, B, offsets, weights, wantWitness, asynchronous) {
    const { N, p, q } = this;
    if (asynchronous) this._refuseCentred('tallyBatchAsync');
    const centred = this._centred, witness = wantWitness || centred;            // the centred second stage starts from remainder1
    const { off, K, G } = tallyGroups(offsets, B);
    const sum = new Uint16Array(G * N), value = new Uint8Array(G * N);
    const q1 = witness ? new Uint16Array(G * N) : null, r1 = witness ? new Uint16Array(G * N) : null;
    const q2 = witness ? new Uint8Array(G * N) : null;
    const args = [N, q, p, Int8Array.from(expandArray(this.f, N, 0)), Uint8Array.from(expandArray(this.fp, N, 0)), rows, weights, off, K, G, B,
      sum, value, q1, r1, q2];
    const res = { sum, value, quotient1: q1, remainder1: r1, quotient2: q2 };
    if (asynchronous) return engine().tallyDecryptBatchAsync(...args).then(() => res);
    engine().tallyDecryptBatch(...args);
    if (!centred) return res;
    const second = this._centredSecondStage(r1, G);
    if (!wantWitness) return { sum, value: second.value, quotient1: null, remainder1: null, quotient2: null };
    return { sum, value: second.value, quotient1: q1, remainder1: r1, quotient2: second.quotient2 };
  }

  // ---- combinations (additive): combines the ciphertexts rows: Uint16Array[B*N] by the weight matrix weights (Uint16Array[B*G] below q
  // with G, or an Array of B arrays of G numbers) and decrypts every combination, in this instance's lift.
  // -> { sum, value, quotient1, remainder1, quotient2 }, [G*N] each: row g is what decryptBatch returns for sum row g.  Composed from
  // sumGroups and decryptBatch (combineRows above).
  combineBatch(rows, B, weights, G = null, wantWitness = true) {
    const m = combineWeights(weights, B, G, this.q);
    const sum = combineRows(this.N, this.q, rows, B, m.w, m.G);
    return { sum, ...this.decryptBatch(sum, m.G, wantWitness) };
  }

  // rows: Uint16Array[B*N] times the one polynomial poly modulo (x^N - 1, q) (multiplyByPolynomialBatch above).
  multiplyByPolynomialBatch(rows, B, poly, wantQuot = false) { return multiplyByPolynomialBatch(rows, this.N, this.q, B, poly, wantQuot); }

  // The decryption noise of the ciphertexts e: Uint16Array[B*N] under this key -> { peak: Uint16Array[B], energy: Array of B Numbers
  // (exact: below 2^53), margin: Int32Array[B] }.  With a = remainder1 of decryptBits(row) and c_k = a_k > q/2 ? a_k - q : a_k:
  // peak = max |c_k|, energy = sum c_k^2, margin = q/2 - peak.  Composed from decryptBatch with its witnesses and a reduction of
  // remainder1 in JavaScript: the same numbers as the engine's ntru_noise_batch, which runs one product and stores 10 bytes per row, but
  // not that call (INTEGRATION.md, "Measuring noise").  A row whose noise has wrapped past q/2 shows the norm of the wrapped value only.
  noiseBatch(e, B) {
    const { N, q } = this;
    if (!(e instanceof Uint16Array) || e.length !== B * N) throw new TypeError(`noiseBatch: e must be a Uint16Array of B * N = ${B * N} values`);
    const r1 = B > 0 ? this.decryptBatch(e, B, true).remainder1 : new Uint16Array(0);      // remainder1 does not depend on the lift
    const peak = new Uint16Array(B), energy = new Array(B).fill(0), margin = new Int32Array(B);
    for (let b = 0; b < B; b++) {
      let m = 0, s = 0;
      for (let k = 0; k < N; k++) {
        const a = r1[b * N + k], c = a > q / 2 ? q - a : a;
        if (c > m) m = c;
        s += c * c;
      }
      peak[b] = m; energy[b] = s; margin[b] = q / 2 - m;
    }
    return { peak, energy, margin };
  }

  // Which of the ciphertexts e: Uint16Array[B*N] repeat an earlier row of the batch or of prior: Uint16Array[S*N] (rows accepted before)
  // -> { first: Array of B Numbers, unique: Array of Numbers }.  Rows are equal when every coefficient agrees modulo q.  The prior rows
  // take the indices 0 .. S - 1, the new rows S .. S + B - 1; first[b] is the smallest index of a row equal to row b, unique the
  // batch-local b with first[b] === S + b, ascending.  Composed in JavaScript, a map from the reduced row to the index that saw it first:
  // the same numbers as the engine's ntru_dedup_rows, which fingerprints, sorts and compares on the device, but not that call
  // (INTEGRATION.md, "Removing duplicates").
  dedupCiphertexts(e, B, { prior = null } = {}) {
    const { N, q } = this;
    if (!(e instanceof Uint16Array) || e.length !== B * N) throw new TypeError(`dedupCiphertexts: e must be a Uint16Array of B * N = ${B * N} values`);
    if (prior !== null && (!(prior instanceof Uint16Array) || prior.length % N !== 0)) throw new TypeError('dedupCiphertexts: prior must be a Uint16Array of whole rows');
    const S = prior === null ? 0 : prior.length / N;
    const seen = new Map(), first = new Array(B), unique = [], row = new Uint16Array(N);
    const keyOf = (a, at) => {
      for (let k = 0; k < N; k++) row[k] = a[at + k] % q;
      return String.fromCharCode.apply(null, row);
    };
    for (let i = 0; i < S; i++) { const key = keyOf(prior, i * N); if (!seen.has(key)) seen.set(key, i); }
    for (let b = 0; b < B; b++) {
      const key = keyOf(e, b * N);
      if (!seen.has(key)) seen.set(key, S + b);
      first[b] = seen.get(key);
      if (first[b] === S + b) unique.push(b);
    }
    return { first, unique };
  }

  // tallyBatch on ciphertexts in the wire format: packed is BigUint64Array[B * outputSize * 4], rows of packOutput(q - 1, N, e).  Composed
  // from unpackBatch and tallyDecryptBatch (same results as ntru_tally_decrypt_packed_batch, not that call).
  tallyPackedBatch(packed, B, offsets = null, weights = null, wantWitness = true) {
    this._refuseCentred('tallyPackedBatch');
    return this._tally(unpackRows(this.N, this.q, packed, B), B, offsets, weights, wantWitness, false);
  }

  // The same on device handles (devAlloc): offsetsDev holds G + 1 int64 row indices on the device (null: uniform groups of K rows); only
  // enqueues.  sumGroupsDev is the sum alone for any modulus.
  tallyBatchDev(fDev, fpDev, rowsDev, B, G, sumDev, valueDev, { offsetsDev = null, K = 0, weightsDev = null, q1Dev = null, r1Dev = null, q2Dev = null } = {}) {
    this._refuseCentred('tallyBatchDev');
    engine().tallyDecryptBatchDev(this.N, this.q, this.p, fDev, fpDev, rowsDev, weightsDev, offsetsDev, K, G, B, sumDev, valueDev, q1Dev, r1Dev, q2Dev);
  }

  static sumGroupsDev(N, mod, rowsDev, B, G, outDev, { offsetsDev = null, K = 0, weightsDev = null } = {}) {
    engine().sumGroupsDev(N, mod, rowsDev, weightsDev, offsetsDev, K, G, B, outDev);
  }

  // ---- one key pair per item (additive): row b of r, m / e goes with key b of `keys`, a generateKeysBatch result (its first B rows are
  // used; an item flagged there throws the reference's 'Could not find invertible f').  Same results, row by row, as loadKeyFromBatch(keys, b)
  // followed by encryptBatch / decryptBatch of that one row.
  _perKeyRows(keys, B, names) {
    const { N } = this;
    if (!keys.flags || keys.flags.length < B) throw new TypeError('batch per key: keys hold fewer than B items');
    for (let b = 0; b < B; b++) if (keys.flags[b]) throw new Error('Could not find invertible f');
    return names.map(n => {
      if (!keys[n] || keys[n].length < B * N) throw new TypeError(`batch per key: keys.${n} is missing or short`);
      return keys[n].subarray(0, B * N);
    });
  }
  encryptBatchPerKey(keys, r, m, B, wantWitness = true, out = {}) {
    const { N, q } = this;
    const [h] = this._perKeyRows(keys, B, ['h']);
    const e = out.e || new Uint16Array(B * N), quot = wantWitness ? (out.quotientE || new Uint16Array(B * N)) : null;
    engine().encryptPeritemBatch(N, q, h, r, m, B, e, quot);
    return { e, quotientE: quot };
  }
  decryptBatchPerKey(keys, e, B, wantWitness = true, out = {}) {
    const { N, p, q } = this;
    this._refuseCentred('decryptBatchPerKey');
    const [f, fp] = this._perKeyRows(keys, B, ['f', 'fp']);
    const value = out.value || new Uint8Array(B * N);
    const q1 = wantWitness ? (out.quotient1 || new Uint16Array(B * N)) : null;
    const r1 = wantWitness ? (out.remainder1 || new Uint16Array(B * N)) : null;
    const q2 = wantWitness ? (out.quotient2 || new Uint8Array(B * N)) : null;
    engine().decryptPeritemBatch(N, q, p, f, fp, e, B, value, q1, r1, q2);
    return { value, quotient1: q1, remainder1: r1, quotient2: q2 };
  }

  // Device-resident pipeline for a batch of plaintexts (additive): the stages of the reference's encrypt / decrypt flow that the
  // caller names run back to back on the GPU, chunk by chunk, and only what is asked for crosses PCIe:
  //   sampleR: { key: Uint32Array[8], firstItem }   r = generateCustomArray(N, dr, dr) with -1 -> p-1 (index.js:89, :461-488) drawn on the
  //                                                 device from the ChaCha20 stream of `key` (replayable) -- or  r: Uint8Array[B*N]
  //   encrypt                                       always (index.js:87-110, this.h)
  //   decrypt: true                                 decryptBits of the fresh ciphertexts (index.js:111-140, this.f / this.fp)
  //   pack: true                                    packOutput (index.js:572-596) of the last stage's result: value (maxVal p-1) when
  //                                                 decrypting, else the ciphertext (maxVal q-1); BigUint64Array[B*outputSize*4] limbs
  //   want: { r, e, value }                         which plain arrays come back (default: e without decrypt, value with it, nothing
  //                                                 but `packed` when pack is set)
  // m: Uint8Array[B*N].  Arrays in `out` (e.g. from NTRU.allocUint8, page-locked) are filled in place.
  pipeline(opts) { return this._pipeline(opts, false); }
  // The same on a libuv worker thread: a Promise of the same result object; the arrays must be left alone until it settles.
  pipelineAsync(opts) { return this._pipeline(opts, true); }
  _pipeline({ m, B, sampleR = null, r = null, decrypt = false, pack = false, want = null, out = {} }, asynchronous) {
    const { N, p, q, dr } = this;
    if (decrypt) this._refuseCentred(asynchronous ? 'pipelineAsync with decrypt: true' : 'pipeline with decrypt: true');
    if (!(m instanceof Uint8Array) || m.length < B * N) throw new TypeError('pipeline: m must be a Uint8Array of B*N plaintext coefficients');
    if ((sampleR === null) === (r === null)) throw new TypeError('pipeline: give either sampleR: {key, firstItem} or r');
    const w = want || (pack ? {} : (decrypt ? { value: true } : { e: true }));
    const res = {};
    if (w.r && sampleR) res.r = out.r || new Uint8Array(B * N);
    if (w.e) res.e = out.e || new Uint16Array(B * N);
    if (w.value) {
      if (!decrypt) throw new TypeError('pipeline: `value` needs decrypt: true');
      res.value = out.value || new Uint8Array(B * N);
    }
    if (pack) {
      const outputSize = engine().packParams(decrypt ? p - 1 : q - 1, N)[3];
      res.packed = out.packed || new BigUint64Array(B * outputSize * 4);
      res.outputSize = outputSize;
    }
    const args = [N, q, p, Uint16Array.from(expandArray(this.h, N, 0)),
      decrypt ? Int8Array.from(expandArray(this.f, N, 0)) : null, decrypt ? Uint8Array.from(expandArray(this.fp, N, 0)) : null,
      sampleR ? sampleR.key : null, sampleR ? (sampleR.firstItem || 0) : 0, dr, dr, r, m, B,
      res.r || null, res.e || null, res.value || null, res.packed || null];
    if (asynchronous) return engine().pipelineBatchAsync(...args).then(() => res);
    engine().pipelineBatch(...args);
    return res;
  }

  // Opaque device buffers + the engine's *_dev entry points on them, for callers that compose the stages themselves
  // (sizes are checked against every handle before a kernel is launched).
  static devAlloc(bytes) { return engine().devAlloc(bytes); }
  static devFree(handle) { engine().devFree(handle); }
  static devUpload(handle, typedArray) { engine().devUpload(handle, typedArray); }
  static devDownload(typedArray, handle) { engine().devDownload(typedArray, handle); return typedArray; }
  sampleRDev(key, firstItem, B, rDev) { engine().sampleTernaryDev(this.N, this.dr, this.dr, this.p - 1, key, firstItem, B, rDev); }
  encryptBatchDev(hDev, rDev, mDev, B, eDev, quotDev = null) { engine().encryptBatchDev(this.N, this.q, hDev, rDev, mDev, B, eDev, quotDev); }
  decryptBatchDev(fDev, fpDev, eDev, B, valueDev, q1Dev = null, r1Dev = null, q2Dev = null) {
    this._refuseCentred('decryptBatchDev');
    engine().decryptBatchDev(this.N, this.q, this.p, fDev, fpDev, eDev, B, valueDev, q1Dev, r1Dev, q2Dev);
  }
  // one key pair per item on device buffers: hDev [B*N] u16 / fDev [B*N] i8, fpDev [B*N] u8 (e.g. generateKeysBatchDev's outputs)
  encryptBatchPerKeyDev(hDev, rDev, mDev, B, eDev, quotDev = null) {
    engine().encryptPeritemBatchDev(this.N, this.q, hDev, rDev, mDev, B, eDev, quotDev);
  }
  decryptBatchPerKeyDev(fDev, fpDev, eDev, B, valueDev, q1Dev = null, r1Dev = null, q2Dev = null) {
    this._refuseCentred('decryptBatchPerKeyDev');
    engine().decryptPeritemBatchDev(this.N, this.q, this.p, fDev, fpDev, eDev, B, valueDev, q1Dev, r1Dev, q2Dev);
  }
  static packBatchDev(maxVal, dataLen, dataDev, B, outDev, bytes = false) { engine().packBatchDev(maxVal, dataLen, dataDev, B, outDev, bytes); }
  // per-item key products on device buffers (f, g: Int8 rows; fq, h and every quotient / remainder of fq and h: Uint16 rows; fp and its
  // quotient / remainder: Uint8 rows; flags: one byte per item)
  verifyKeysBatchDev(fDev, gDev, fqDev, fpDev, hDev, B, quotFqDev, remFqDev, quotFpDev, remFpDev, quotHDev, remHDev, flagsDev) {
    engine().verifyKeysBatchDev(this.N, this.q, this.p, fDev, gDev, fqDev, fpDev, hDev, B, quotFqDev, remFqDev, quotFpDev, remFpDev,
      quotHDev, remHDev, flagsDev);
  }
  invertKeyBatchDev(fDev, B, fqDev, fpDev, flagsDev) { engine().invertKeyBatchDev(this.N, this.q, this.p, fDev, B, fqDev, fpDev, flagsDev); }
  publicKeyBatchDev(fqDev, gDev, B, hDev) { engine().publicKeyBatchDev(this.N, this.q, this.p, fqDev, gDev, B, hDev); }
  static polymulSplitDev(N, mod, aDev, bDev, B, quotDev, remDev) { engine().polymulSplitDev(N, mod, aDev, bDev, B, quotDev, remDev); }

  // ---- batched key generation: generatePrivateKeyF + generateNewPublicKeyGH (index.js:51-79) for B items, non-units redrawn on the GPU.
  // key: Uint32Array[8], secret (fill it from crypto.randomFillSync; never the key that draws r).  Item i = firstItem + b draws g at
  // ChaCha20 stream position 2^40 + i and attempt t of f at t * 2^44 + i (include/ntru_engine.h, ntru_keygen_batch): any host can replay
  // it.  want: which arrays come back ({ f, g, fq, fp, h, tries }, default all); flags always (nonzero: no invertible f in maxTries
  // draws); pack: also packedH = packOutput(q - 1, N, h) as BigUint64Array[B*outputSize*4].  Arrays in `out` are filled in place.
  generateKeysBatch(opts) { return this._keygen(opts, false); }
  generateKeysBatchAsync(opts) { return this._keygen(opts, true); }
  _keygen({ B, key, firstItem = 0, maxTries = 100, want = null, pack = false, out = {} }, asynchronous) {
    const { N, p, q, df, dg } = this;
    if (!(key instanceof Uint32Array) || key.length < 8) throw new TypeError('generateKeysBatch: key must be a Uint32Array[8]');
    const w = want || { f: true, g: true, fq: true, fp: true, h: true, tries: true };
    const rows = { f: Int8Array, g: Int8Array, fq: Uint16Array, fp: Uint8Array, h: Uint16Array };
    const res = { B };
    for (const [name, T] of Object.entries(rows)) if (w[name]) res[name] = out[name] || new T(B * N);
    if (w.tries) res.tries = out.tries || new Uint8Array(B);
    res.flags = out.flags || new Uint8Array(B);
    if (pack) {
      res.outputSize = engine().packParams(q - 1, N)[3];
      res.packedH = out.packedH || new BigUint64Array(B * res.outputSize * 4);
    }
    const args = [N, q, p, df, dg, key, firstItem, maxTries, B, res.f || null, res.g || null, res.fq || null, res.fp || null,
      res.h || null, res.tries || null, res.flags, res.packedH || null];
    if (asynchronous) return engine().keygenBatchAsync(...args).then(() => res);
    engine().keygenBatch(...args);
    return res;
  }
  // The same on device buffers: workDev of NTRU.keygenWorkspaceBytes(N, B) bytes, f, g (B*N bytes), fq, h (2*B*N), fp (B*N), tries (B,
  // may be null), flags (B).  Waits for the GPU once per call and once per redraw pass (a 4-byte count of the items left to redraw).
  generateKeysBatchDev({ B, key, firstItem = 0, maxTries = 100, workDev, fDev, gDev, fqDev, fpDev, hDev, triesDev = null, flagsDev }) {
    engine().keygenBatchDev(this.N, this.q, this.p, this.df, this.dg, key, firstItem, maxTries, B, workDev, fDev, gDev, fqDev, fpDev,
      hDev, triesDev, flagsDev);
  }
  static keygenWorkspaceBytes(N, B) { return engine().keygenWorkspaceBytes(N, B); }
  // f, fq, fp, g, h of item i of a generateKeysBatch result, as generatePrivateKeyF + generateNewPublicKeyGH leave them.
  loadKeyFromBatch(keys, i) {
    if (keys.flags[i]) throw new Error('Could not find invertible f');
    const { N } = this;
    const row = a => Array.from(a.subarray(i * N, (i + 1) * N));
    this.f = row(keys.f);
    this.fq = trimPolynomial(row(keys.fq));
    this.fp = trimPolynomial(row(keys.fp));
    this.g = row(keys.g);
    this.h = trimPolynomial(row(keys.h));
    return this;
  }

  // Promise-returning twins of the two batch calls: the engine call runs on a libuv worker thread, the event loop keeps
  // turning meanwhile (calls are serialised inside the addon: one engine).  Same arguments, same results; the input and
  // output arrays must be left alone until the Promise settles.
  encryptBatchAsync(r, m, B, wantWitness = true, out = {}) {
    const { N, q } = this;
    const e = out.e || new Uint16Array(B * N), quot = wantWitness ? (out.quotientE || new Uint16Array(B * N)) : null;
    return engine().encryptBatchAsync(N, q, Uint16Array.from(expandArray(this.h, N, 0)), r, m, B, e, quot)
      .then(() => ({ e, quotientE: quot }));
  }

  decryptBatchAsync(e, B, wantWitness = true, out = {}) {
    const { N, p, q } = this;
    this._refuseCentred('decryptBatchAsync');
    const value = out.value || new Uint8Array(B * N);
    const q1 = wantWitness ? (out.quotient1 || new Uint16Array(B * N)) : null;
    const r1 = wantWitness ? (out.remainder1 || new Uint16Array(B * N)) : null;
    const q2 = wantWitness ? (out.quotient2 || new Uint8Array(B * N)) : null;
    return engine().decryptBatchAsync(N, q, p, Int8Array.from(expandArray(this.f, N, 0)),
      Uint8Array.from(expandArray(this.fp, N, 0)), e, B, value, q1, r1, q2)
      .then(() => ({ value, quotient1: q1, remainder1: r1, quotient2: q2 }));
  }

  // ---- byte messages of any length (additive; the reference's encryptStr takes at most N bits, index.js:81).  Same framing and results
  // as the Python NTRU.encryptBytes / decryptBytes: blocks of W = bytesPerBlock bytes, the last one zero padded, bit 7 of a byte first
  // (index.js:542), every block encrypted as encryptStr encrypts it.  Here the bits are expanded and collected in JavaScript around
  // encryptBatch / decryptBatch; the engine's ntru_encrypt_bytes_batch / ntru_decrypt_bytes_batch have no native Node path yet.
  get bytesPerBlock() { return Math.floor(this.N / 8); }

  // data: Uint8Array / Buffer, or a latin-1 string -> { m: Uint8Array[blocks*N], blocks }
  _bytesToRows(data) {
    const { N } = this, W = this.bytesPerBlock;
    if (W < 1) throw new Error(`encryptBytes: N = ${N} holds no whole byte`);
    if (typeof data === 'string') {
      const s = data;
      data = new Uint8Array(s.length);
      for (let i = 0; i < s.length; i++) {
        const c = s.charCodeAt(i);
        if (c > 255) throw new Error('encryptBytes: a string must be latin-1 (char codes below 256); encode it to bytes first');
        data[i] = c;
      }
    }
    const blocks = Math.ceil(data.length / W), m = new Uint8Array(blocks * N);
    for (let i = 0; i < data.length; i++) {
      const at = Math.floor(i / W) * N + 8 * (i % W), x = data[i];
      for (let j = 0; j < 8; j++) m[at + j] = (x >> (7 - j)) & 1;
    }
    return { m, blocks };
  }

  // r: Uint8Array[blocks*N] in {0, 1, p-1} or an array of signed ternary rows; drawn per block like encryptBits' when null
  _bytesR(r, blocks) {
    const { N, p } = this;
    if (r === null || r === undefined) r = Array.from({ length: blocks }, () => generateCustomArray(N, this.dr, this.dr));
    const flat = ArrayBuffer.isView(r) ? r : r.flat();
    if (flat.length !== blocks * N) throw new Error(`encryptBytes: ${flat.length / N} rows of r for ${blocks} blocks`);
    return Uint8Array.from(flat, x => (x === -1 ? p - 1 : x));                 // index.js:89
  }

  _rowsToBytes(value, blocks, length) {
    const { N } = this, W = this.bytesPerBlock, msg = 8 * W;
    const all = new Uint8Array(blocks * W), flags = new Uint8Array(blocks);
    for (let b = 0; b < blocks; b++) {
      let f = 0;
      for (let k = 0; k < N; k++) {
        const v = value[b * N + k];
        if (k < msg) { if (v > 1) f |= 32; all[b * W + (k >> 3)] |= (v & 1) << (7 - (k & 7)); } else if (v !== 0) f |= 64;
      }
      flags[b] = f;                                                           // NTRU_FLAG_NOT_BITS 32, NTRU_FLAG_PAD_NONZERO 64
    }
    let n = all.length;
    if (length === null || length === undefined) while (n > 0 && all[n - 1] === 0) n--;   // decryptStr's trimPolynomial
    else if (!(length >= 0 && length <= n)) throw new Error(`decryptBytes: length ${length} is outside the ${n} bytes of ${blocks} blocks`);
    else n = length;
    return { data: all.slice(0, n), flags };
  }

  // -> Uint16Array[blocks*N], the ciphertext of every block
  encryptBytes(data, r = null) {
    const { m, blocks } = this._bytesToRows(data);
    if (blocks === 0) return new Uint16Array(0);
    return this.encryptBatch(this._bytesR(r, blocks), m, blocks, false).e;
  }
  encryptBytesAsync(data, r = null) {
    const { m, blocks } = this._bytesToRows(data);
    if (blocks === 0) return Promise.resolve(new Uint16Array(0));
    return this.encryptBatchAsync(this._bytesR(r, blocks), m, blocks, false).then(o => o.e);
  }

  // e: Uint16Array[blocks*N] -> { data: Uint8Array (cut to `length`, or trailing zero bytes stripped), flags: Uint8Array[blocks] }
  decryptBytes(e, blocks, length = null) {
    this._refuseCentred('decryptBytes');
    if (blocks === 0) return this._rowsToBytes(new Uint8Array(0), 0, length);
    return this._rowsToBytes(this.decryptBatch(e, blocks, false).value, blocks, length);
  }
  decryptBytesAsync(e, blocks, length = null) {
    this._refuseCentred('decryptBytesAsync');
    if (blocks === 0) return Promise.resolve(this._rowsToBytes(new Uint8Array(0), 0, length));
    return this.decryptBatchAsync(e, blocks, false).then(o => this._rowsToBytes(o.value, blocks, length));
  }

  // ---- scanning (additive; INTEGRATION.md "Scanning: scanBytes"): which blocks does a key decrypt to a well-formed message that carries
  // the tag?  Same definition, order and truncation as the engine's ntru_scan_bytes_batch and the Python NTRU.scanBytes: block b is a hit
  // for a key when decryptBytes gives it flag 0 and bytes [tagOffset, tagOffset + tag.length) of its message equal `tag` (at most 32
  // bytes).  The addon's export list is fixed, so this is composed from decryptBytes per key plus a filter in JavaScript: correct, not
  // fast -- every block's bytes cross the bus.  With lift: 'centred' it throws what decryptBytes throws.
  // e: Uint16Array[blocks*N]; keys: [{f, fp}] or [[f, fp]] (default: this instance's key); maxHits null keeps every hit, 0 only counts.
  // -> per key { count, rows: Array of block indices, bytes: Uint8Array[stored * bytesPerBlock] }, stored = min(count, maxHits)
  scanBytes(e, blocks, { keys = null, tag = new Uint8Array(0), tagOffset = 0, maxHits = null } = {}) {
    const { N, p, q, df, dg, dr, lift } = this, W = this.bytesPerBlock;
    if (typeof tag === 'string') tag = Uint8Array.from(tag, c => c.charCodeAt(0));
    if (tag.length > 32) throw new Error(`scanBytes: a tag has at most 32 bytes, got ${tag.length}`);
    if (!(Number.isInteger(tagOffset) && tagOffset >= 0 && tagOffset + tag.length <= W))
      throw new Error(`scanBytes: the tag [${tagOffset}, ${tagOffset + tag.length}) does not lie inside the ${W} message bytes`);
    if (maxHits !== null && !(Number.isInteger(maxHits) && maxHits >= 0)) throw new Error('scanBytes: negative maxHits');
    if (keys === null) keys = [{ f: this.f, fp: this.fp }];
    if (keys.length < 1) throw new Error('scanBytes: need at least one key');
    const limit = maxHits === null ? blocks : maxHits;
    return keys.map(key => {
      const [f, fp] = Array.isArray(key) ? key : [key.f, key.fp];
      const one = new NTRU({ N, p, q, df, dg, dr, f: Array.from(f), fp: Array.from(fp), lift });
      const { data, flags } = one.decryptBytes(e, blocks, blocks * W);
      const rows = [], kept = [];
      let count = 0;
      for (let b = 0; b < blocks; b++) {
        if (flags[b] !== 0) continue;
        let same = true;
        for (let j = 0; j < tag.length && same; j++) same = data[b * W + tagOffset + j] === tag[j];
        if (!same) continue;
        if (count++ < limit) { rows.push(b); kept.push(data.subarray(b * W, (b + 1) * W)); }
      }
      const bytes = new Uint8Array(kept.length * W);
      kept.forEach((row, i) => bytes.set(row, i * W));
      return { count, rows, bytes };
    });
  }
}

// ---- witness checks: does a witness satisfy VerifyEncrypt / VerifyDecrypt / VerifyInverse (circuits/ntru.circom)? ----------------
// checkWitnesses(template, witnesses): witnesses = [{inputs, params}] as encryptBits, decryptBits and verifyKeysInputs()[fq|fp|h]
// return them, all with the same params; returns one flag value per witness: 0 = accepted, else the OR of EQ 1, TAIL 2, RANGE 4
// (VerifyDecrypt's mod-p stage shifted left by 3) -- include/ntru_engine.h, NTRU_CHECK_*.
const CHECK_SIGNALS = {
  VerifyEncrypt: [['r', 0], ['m', 0], ['h', 0], ['quotientE', 1], ['remainderE', 1]],
  VerifyDecrypt: [['f', 0], ['fp', 0], ['e', 0], ['quotient1', 1], ['remainder1', 1], ['quotient2', 1], ['remainder2', 1]],
  VerifyInverse: [['f', 0], ['fq', 0], ['quotientI', 1], ['remainderI', 1]],
};
const CHECK_PARAMS = { VerifyEncrypt: 3, VerifyDecrypt: 5, VerifyInverse: 3 };

export function checkWitnesses(template, witnesses) {
  const signals = CHECK_SIGNALS[template];
  if (!signals) throw new Error(`checkWitnesses: unknown template ${template} (VerifyEncrypt, VerifyDecrypt or VerifyInverse)`);
  if (!Array.isArray(witnesses)) throw new Error('checkWitnesses: witnesses must be an array of {inputs, params}');
  const B = witnesses.length;
  if (B === 0) return [];
  const params = witnesses[0].params;
  if (!Array.isArray(params) || params.length !== CHECK_PARAMS[template] || !params.every(Number.isInteger))
    throw new Error(`checkWitnesses: ${template} takes ${CHECK_PARAMS[template]} integer params`);
  const N = params[params.length - 1];
  const rows = signals.map(([name, extra]) => {
    const len = N + extra;
    const out = new Uint16Array(B * len);
    witnesses.forEach((w, i) => {
      if (!Array.isArray(w.params) || w.params.length !== params.length || w.params.some((x, j) => x !== params[j]))
        throw new Error(`checkWitnesses: item ${i} has params ${JSON.stringify(w.params)}, item 0 ${JSON.stringify(params)}`);
      const v = w.inputs[name];
      if (!v || v.length !== len) throw new Error(`checkWitnesses: item ${i}: ${name} has length ${v ? v.length : 0}, expected ${len}`);
      for (let k = 0; k < len; k++) {
        const x = v[k];
        if (!Number.isInteger(x) || x < 0 || x > 65535)
          throw new Error(`checkWitnesses: item ${i}: ${name}[${k}] = ${x} is not an integer in [0, 65535]`);
        out[i * len + k] = x;
      }
    });
    return out;
  });
  const flags = new Uint8Array(B);
  if (template === 'VerifyEncrypt') engine().checkEncryptBatch(N, params[0], params[1], ...rows, B, flags);
  else if (template === 'VerifyDecrypt') engine().checkDecryptBatch(N, params[0], params[1], params[2], params[3], ...rows, B, flags);
  else engine().checkInverseBatch(N, params[0], params[1], ...rows, B, flags);
  return Array.from(flags);
}
