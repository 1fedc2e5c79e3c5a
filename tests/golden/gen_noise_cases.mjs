// Golden cases for the decryption noise of ciphertexts: runs the UNMODIFIED reference under Node and records, for four parameter sets,
// the reference's own key pair, B = 8 encryptions of encryptBits (index.js:87-110) with their r and m, and the sums of the first
// K = 1, 2, 4 and 8 ciphertexts folded with addPolynomials (index.js:235-244).  For every sum: e, decryptBits(e).inputs.remainder1
// (index.js:113-114), A = p sum(r * g) + f * sum(m) modulo x^N - 1 computed OVER THE INTEGERS by the plain loop below (r as encryptBits
// multiplies it: in {0, 1, p - 1}, index.js:89), and `inside`: whether every A_k lies in (-q/2, q/2] -- the condition under which the centred remainder1 IS A.
// The file is written only when at least 8 sums are inside that interval and at least 2 are not, so that both sides are present.
// Only the resulting JSON is committed.  Integer arrays are stored bit-packed as in gen_tally_cases.mjs: { bits, n, off, b64 } holds n
// values v with v - off in [0, 2^bits), least significant bit first, as base64; tests/noise_ref.py and tests/js/shim_noise.mjs unpack
// them.
//
//   node tests/golden/gen_noise_cases.mjs <checkout of the reference> [outdir] [seed]     (a seed that leaves one side short is refused)
import { writeFileSync } from 'fs';
import { dirname, join } from 'path';
import { fileURLToPath, pathToFileURL } from 'url';

const here = dirname(fileURLToPath(import.meta.url));
const refDir = process.argv[2];
if (!refDir) { console.error('usage: node gen_noise_cases.mjs <checkout of the reference> [outdir]'); process.exit(2); }
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

// x * y modulo x^N - 1 over the integers
function cyclic(x, y, N) {
  const out = new Array(N).fill(0);
  for (let i = 0; i < N; i++) for (let j = 0; j < N; j++) out[(i + j) % N] += x[i] * y[j];
  return out;
}

async function main() {
const ref = await import(pathToFileURL(join(refDir, 'index.js')).href);
const NTRU = ref.default;
const { addPolynomials, trimPolynomial, expandArray } = ref;

const B = 8, KS = [1, 2, 4, 8];
const sets = [
  ['n17_q32', { N: 17, q: 32, p: 3, df: 3, dg: 2, dr: 2 }],
  ['n167_q128_low_noise', { N: 167, q: 128, p: 3, df: 20, dg: 10, dr: 5 }],
  ['n167_q128_default', { N: 167, q: 128, p: 3 }],
  ['n509_q2048', { N: 509, q: 2048, p: 3, df: 40, dg: 40, dr: 20 }],
];
const out = [];
let seed = Number(process.argv[4] || 341), inside = 0, outside = 0;
for (const [name, options] of sets) {
  state = (seed++ * 2654435761) >>> 0 || 1;
  const ntru = new NTRU({ ...options });
  ntru.generatePrivateKeyF();
  ntru.generateNewPublicKeyGH();
  const { N, q, p } = ntru;
  const qb = Math.log2(q);
  const f = expandArray(ntru.f, N, 0), g = expandArray(ntru.g, N, 0);
  const ms = [], rs = [], es = [];
  for (let b = 0; b < B; b++) {
    const m = Array.from({ length: N }, () => nextU32() % 2);
    const enc = ntru.encryptBits(m);
    ms.push(m);
    rs.push(expandArray(enc.inputs.r, N, 0));
    es.push(expandArray(enc.value, N, 0));
  }
  const cases = [];
  for (const K of KS) {
    let sum = new Array(N).fill(0);
    const rsum = new Array(N).fill(0), msum = new Array(N).fill(0);
    for (let b = 0; b < K; b++) {
      sum = addPolynomials(sum, es[b], q);
      for (let i = 0; i < N; i++) { rsum[i] += rs[b][i]; msum[i] += ms[b][i]; }
    }
    sum = expandArray(sum, N, 0);
    const rg = cyclic(rsum, g, N), fm = cyclic(f, msum, N);
    const A = rg.map((x, i) => p * x + fm[i]);
    const ok = A.every(x => 2 * x > -q && 2 * x <= q);
    if (ok) inside++; else outside++;
    const remainder1 = ntru.decryptBits(trimPolynomial(sum)).inputs.remainder1.slice(0, N);
    cases.push({ K, inside: ok, e: pack(sum, qb), remainder1: pack(remainder1, qb), A: pack(A, 16, -32768) });
  }
  out.push({ set: name, options: { N, q, p, df: ntru.df, dg: ntru.dg, dr: ntru.dr }, B,
             key: { f: pack(f, 2, -1), g: pack(g, 2, -1) }, r: pack(rs, 2), m: pack(ms, 1), cases });
}
if (inside < 8 || outside < 2) throw new Error(`the fixture needs both sides: ${inside} sums inside (-q/2, q/2], ${outside} outside`);
writeFileSync(join(outDir, 'noise_cases.json'),
  `{"generator":"gen_noise_cases.mjs","sets":[\n${out.map(c => JSON.stringify(c)).join(',\n')}\n]}\n`);
console.log('noise_cases.json:', out.map(s => `${s.set}: ` + s.cases.map(c => `K=${c.K} ${c.inside ? 'inside' : 'outside'}`).join(', ')).join(' | '));
}
main().catch(e => { console.error(e); process.exit(1); });
