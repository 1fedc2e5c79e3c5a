// Golden cases for combinations of ciphertexts by a weight matrix: runs the UNMODIFIED reference under Node and records, for seeded
// keys and plaintexts, B = 8 ciphertexts of encryptBits (index.js:87-110) and, for three weight matrices [B][G], every combination
// g folded with addPolynomials (index.js:235-244) over the ciphertexts scaled with multiplyPolynomialsByScalar (index.js:404-406),
// the full decryptBits object (index.js:111-140) of each combination, and `recovered`: whether the reference's decrypted value equals
// the weighted sum of the plaintexts modulo p (weights multiply the noise, and sums raise it, so it may be false).  The generator
// itself asserts that every output of the 0/1 matrix at N = 509 is recovered: the fixture holds at least one end-to-end correct tally.
// Only the resulting JSON is committed.  Integer arrays are stored bit-packed as in gen_tally_cases.mjs: { bits, n, off, b64 } holds n
// values v with v - off in [0, 2^bits), least significant bit first, as base64; tests/combine_ref.py and tests/js/shim_combine.mjs
// unpack them.
//
//   node tests/golden/gen_combine_cases.mjs <checkout of the reference> [outdir]
import { writeFileSync } from 'fs';
import { dirname, join } from 'path';
import { fileURLToPath, pathToFileURL } from 'url';

const here = dirname(fileURLToPath(import.meta.url));
const refDir = process.argv[2];
if (!refDir) { console.error('usage: node gen_combine_cases.mjs <checkout of the reference> [outdir]'); process.exit(2); }
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

const B = 8;
// weights[b] = the weights of ciphertext b, one per output
const matrices = [
  ['memberships', Array.from({ length: B }, (_, b) => [1, b < B / 2 ? 1 : 0, b < B / 2 ? 0 : 1])],   // grand total + two halves
  ['small_weights', [[1, 0], [0, 2], [2, 1], [1, 1], [0, 0], [2, 2], [1, 2], [0, 1]]],
  ['all_ones', Array.from({ length: B }, () => [1])],
];
const sets = [
  ['n167_q128_low_noise', { N: 167, q: 128, p: 3, df: 20, dg: 10, dr: 5 }],
  ['n509_q2048', { N: 509, q: 2048, p: 3, df: 40, dg: 40, dr: 20 }],
];
const out = [];
let seed = 0xc0b1e5;
for (const [name, options] of sets) {
  state = (seed++ * 2654435761) >>> 0 || 1;
  const ntru = new NTRU({ ...options });
  ntru.generatePrivateKeyF();
  ntru.generateNewPublicKeyGH();
  const { N, q, p } = options;
  const qb = Math.log2(q);
  const ms = [], es = [];
  for (let b = 0; b < B; b++) {
    const m = Array.from({ length: N }, () => nextU32() % 2);
    ms.push(m);
    es.push(expandArray(ntru.encryptBits(m).value, N, 0));
  }
  const cases = [];
  for (const [kind, weights] of matrices) {
    const G = weights[0].length;
    const outputs = [];
    for (let g = 0; g < G; g++) {
      let sum = new Array(N).fill(0), want = new Array(N).fill(0);
      for (let b = 0; b < B; b++) {
        const w = weights[b][g];
        sum = addPolynomials(sum, multiplyPolynomialsByScalar(es[b], w, q), q);
        want = want.map((x, i) => (x + w * ms[b][i]) % p);
      }
      sum = expandArray(sum, N, 0);
      const decrypt = ntru.decryptBits(trimPolynomial(sum));
      const recovered = JSON.stringify(decrypt.value) === JSON.stringify(trimPolynomial(want));
      if (kind === 'memberships' && N === 509 && !recovered) throw new Error(`output ${g} of the 0/1 matrix at N = 509 is not recovered`);
      const i = decrypt.inputs;
      outputs.push({ sum: pack(sum, qb), expected: pack(want, 2), recovered,
                     decrypt: { value: pack(decrypt.value, 2), params: decrypt.params,
                                inputs: { f: pack(i.f, qb), fp: pack(i.fp, 2), e: pack(i.e, qb), quotient1: pack(i.quotient1, qb),
                                          remainder1: pack(i.remainder1, qb), quotient2: pack(i.quotient2, 2),
                                          remainder2: pack(i.remainder2, 2) } } });
    }
    cases.push({ kind, G, weights, outputs });
  }
  out.push({ set: name, options, B,
             key: { f: pack(ntru.f, 2, -1), fp: pack(ntru.fp, 2), g: pack(ntru.g, 2, -1), h: pack(ntru.h, qb) },
             m: pack(ms, 1), e: pack(es, qb), cases });
}
// one set per line
writeFileSync(join(outDir, 'combine_cases.json'),
  `{"generator":"gen_combine_cases.mjs","sets":[\n${out.map(c => JSON.stringify(c)).join(',\n')}\n]}\n`);
console.log('combine_cases.json:', out.map(s => `${s.set}: ` + s.cases.map(c => `${c.kind} ${c.outputs.map(o => o.recovered)}`).join('; ')).join(' | '));
}
main().catch(e => { console.error(e); process.exit(1); });
