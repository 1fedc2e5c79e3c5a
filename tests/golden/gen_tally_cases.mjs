// Golden cases for sums of ciphertexts (tallies): runs the UNMODIFIED reference under Node and records, for seeded keys and
// plaintexts, K ciphertexts of encryptBits (index.js:87-110), their sum folded with addPolynomials (index.js:235-244) -- each
// ciphertext first scaled with multiplyPolynomialsByScalar (index.js:404-406) where the case has weights -- and the full
// decryptBits object (index.js:111-140) of that sum.  `recovered` says whether the reference's decrypted value equals the weighted
// sum of the plaintexts modulo p: sums raise the noise, and the lift of index.js:117 is off for q = 1 (mod 3), so it may be false.
// Only the resulting JSON is committed.  To keep it small every integer array is stored bit-packed: { bits, n, off, b64 } holds n values
// v with v - off in [0, 2^bits), least significant bit first, as base64 (rows of a [K][N] array one after the other);
// tests/ciphertext_sum_ref.py and tests/js/shim_tally.mjs unpack them.
//
//   node tests/golden/gen_tally_cases.mjs [/root/reference] [outdir]
import { writeFileSync } from 'fs';
import { dirname, join } from 'path';
import { fileURLToPath, pathToFileURL } from 'url';

const here = dirname(fileURLToPath(import.meta.url));
const refDir = process.argv[2] || '/root/reference';
const outDir = process.argv[3] || here;
let state = 1;
function nextU32() { let x = state; x ^= x << 13; x >>>= 0; x ^= x >>> 17; x ^= x << 5; x >>>= 0; state = x; return x; }
globalThis.crypto = { getRandomValues(arr) { for (let i = 0; i < arr.length; i++) arr[i] = nextU32(); return arr; } };

function pack(values, bits, off = 0) {
  const flat = values.flat();
  const bytes = Buffer.alloc(Math.ceil(flat.length * bits / 8));
  flat.forEach((v, i) => {
    const x = v - off;
    if (!Number.isInteger(x) || x < 0 || x >= 2 ** bits) throw new Error(`pack: ${v} does not fit ${bits} bits at offset ${off}`);
    for (let b = 0; b < bits; b++) if ((x >> b) & 1) { const at = i * bits + b; bytes[at >> 3] |= 1 << (at & 7); }
  });
  return { bits, n: flat.length, off, b64: bytes.toString('base64') };
}

async function main() {
const ref = await import(pathToFileURL(join(refDir, 'index.js')).href);
const NTRU = ref.default;
const { addPolynomials, multiplyPolynomialsByScalar, trimPolynomial, expandArray } = ref;

// [set name, options, [[K, weights or null], ...]]
const small = { N: 167, q: 128, p: 3, df: 20, dg: 10, dr: 5 };
const mid = { N: 509, q: 2048, p: 3, df: 40, dg: 40, dr: 20 };
const sets = [
  ['n167_q128_low_noise', small, [[2, null], [4, null], [8, null], [2, [1, 2]], [4, [2, 1, 1, 2]]]],
  ['n509_q2048', mid, [[2, null], [4, null], [8, null], [16, null], [32, null], [4, [1, 2, 1, 3]]]],
  ['n167_q128_default', { N: 167, q: 128, p: 3, df: 61, dg: 20, dr: 18 }, [[2, null]]],
  ['n167_q4096_default', { N: 167, q: 4096, p: 3, df: 61, dg: 20, dr: 18 }, [[2, null]]],
];
const cases = [];
let seed = 0x7a11e5;
for (const [name, options, list] of sets) {
  for (const [K, weights] of list) {
    state = (seed++ * 2654435761) >>> 0 || 1;
    const ntru = new NTRU({ ...options });
    ntru.generatePrivateKeyF();
    ntru.generateNewPublicKeyGH();
    const { N, q, p } = options;
    const ms = [], es = [];
    for (let k = 0; k < K; k++) {
      const m = Array.from({ length: N }, () => nextU32() % 2);
      ms.push(m);
      es.push(expandArray(ntru.encryptBits(m).value, N, 0));
    }
    let sum = new Array(N).fill(0), want = new Array(N).fill(0);
    for (let k = 0; k < K; k++) {
      const w = weights ? weights[k] : 1;
      sum = addPolynomials(sum, weights ? multiplyPolynomialsByScalar(es[k], w, q) : es[k], q);
      want = want.map((x, i) => (x + w * ms[k][i]) % p);
    }
    sum = expandArray(sum, N, 0);
    const decrypt = ntru.decryptBits(trimPolynomial(sum));
    const recovered = JSON.stringify(decrypt.value) === JSON.stringify(trimPolynomial(want));
    const qb = Math.log2(q), i = decrypt.inputs;
    cases.push({ set: name, options, K, weights,
                 key: { f: pack(ntru.f, 2, -1), fp: pack(ntru.fp, 2), g: pack(ntru.g, 2, -1), h: pack(ntru.h, qb) },
                 m: pack(ms, 1), e: pack(es, qb), sum: pack(sum, qb),
                 decrypt: { value: pack(decrypt.value, 2), params: decrypt.params,
                            inputs: { f: pack(i.f, qb), fp: pack(i.fp, 2), e: pack(i.e, qb), quotient1: pack(i.quotient1, qb),
                                      remainder1: pack(i.remainder1, qb), quotient2: pack(i.quotient2, 2), remainder2: pack(i.remainder2, 2) } },
                 expected: pack(want, 2), recovered });
  }
}
// one case per line
writeFileSync(join(outDir, 'tally_cases.json'),
  `{"generator":"gen_tally_cases.mjs","cases":[\n${cases.map(c => JSON.stringify(c)).join(',\n')}\n]}\n`);
console.log('tally_cases.json:', cases.map(c => `${c.set} K=${c.K}${c.weights ? 'w' : ''} ${c.recovered}`).join(', '));
}
main().catch(e => { console.error(e); process.exit(1); });
