// Golden cases for re-randomising and shuffling ciphertexts (one mix step): runs the UNMODIFIED reference under Node and records, for
// seeded keys and plaintexts, three rounds of encryptBits (index.js:87-110) with the previous round's ciphertext in the place of m --
// addPolynomials(e, multiplyPolynomials(r, h, q), q), then dividePolynomials(., I, q) (index.js:90-92).  Rounds 1 and 2 permute the 6
// rows, round 3 gathers them with repeats into 9.  Per round: r, src (output row i re-randomises row src[i] of the round's input),
// the remainder and quotient % q of every output row, the reference's decryptBits(row).value (index.js:111-140), and `recovered`, one
// flag per output row: does that value equal the plaintext the row descends from?  Re-randomising raises the noise and the lift of
// index.js:117 is off for q = 1 (mod 3), so for the last two sets it may be 0; the first four sets must recover every row of every
// round, else this generator throws.
// Only the resulting JSON is committed.  Every integer array is stored bit-packed: { bits, n, off, b64 } holds n values v with v - off in
// [0, 2^bits), least significant bit first, as base64 (rows of a [K][N] array one after the other); tests/mix_ref.py and
// tests/js/shim_mix.mjs unpack them.
//
//   node tests/golden/gen_mix_cases.mjs [/root/reference] [outdir]
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

function permutation(n) {
  const a = Array.from({ length: n }, (_, i) => i);
  for (let i = n - 1; i > 0; i--) { const j = nextU32() % (i + 1); [a[i], a[j]] = [a[j], a[i]]; }
  return a;
}

async function main() {
const ref = await import(pathToFileURL(join(refDir, 'index.js')).href);
const NTRU = ref.default;
const { trimPolynomial, expandArray } = ref;

// [set name, options, must every row of every round decrypt to its plaintext?]
const sets = [
  ['n17_q32', { N: 17, q: 32, p: 3, df: 3, dg: 2, dr: 1 }, true],
  ['n167_q128_low_noise', { N: 167, q: 128, p: 3, df: 20, dg: 10, dr: 5 }, true],
  ['n509_q2048', { N: 509, q: 2048, p: 3, df: 40, dg: 40, dr: 20 }, true],
  ['n701_q8192', { N: 701, q: 8192, p: 3, df: 60, dg: 60, dr: 30 }, true],
  ['n167_q128_default', { N: 167, q: 128, p: 3, df: 61, dg: 20, dr: 18 }, false],
  ['n821_q4096', { N: 821, q: 4096, p: 3, df: 60, dg: 60, dr: 30 }, false],
];
const K = 6, K3 = 9;
const cases = [];
// At N = 17 / q = 32 three more rounds of noise leave little margin: of eight seeds tried, this is the one under which the reference
// recovers every row of the first four sets (the larger three of them recover under every seed tried).
let seed = 0x5eed04;
for (const [name, options, mustRecover] of sets) {
  state = (seed++ * 2654435761) >>> 0 || 1;
  const ntru = new NTRU({ ...options });
  ntru.generatePrivateKeyF();
  ntru.generateNewPublicKeyGH();
  const { N, q } = options;
  const qb = Math.log2(q);
  const ms = [], es = [];
  for (let k = 0; k < K; k++) {
    const m = Array.from({ length: N }, () => nextU32() % 2);
    ms.push(m);
    es.push(expandArray(ntru.encryptBits(m).value, N, 0));
  }
  let cur = es, plain = ms;
  const rounds = [];
  for (let round = 0; round < 3; round++) {
    const src = round < 2 ? permutation(K) : Array.from({ length: K3 }, () => nextU32() % K);
    const rs = [], rem = [], quot = [], values = [], recovered = [], nextPlain = [];
    for (const s of src) {
      const enc = ntru.encryptBits(cur[s]);
      if (JSON.stringify(enc.inputs.m) !== JSON.stringify(cur[s])) throw new Error('the witness m is not the old ciphertext');
      rs.push(enc.inputs.r);
      rem.push(enc.inputs.remainderE.slice(0, N));
      quot.push(enc.inputs.quotientE.slice(0, N));
      if (enc.inputs.remainderE[N] !== 0 || enc.inputs.quotientE[N] !== 0) throw new Error('coefficient N of the witness is not 0');
      const value = expandArray(ntru.decryptBits(enc.value).value, N, 0);
      values.push(value);
      nextPlain.push(plain[s]);
      recovered.push(JSON.stringify(value) === JSON.stringify(plain[s]) ? 1 : 0);
    }
    if (mustRecover && recovered.includes(0)) throw new Error(`${name}: round ${round + 1} does not recover every plaintext`);
    rounds.push({ src, r: pack(rs, 2), remainder: pack(rem, qb), quotient: pack(quot, qb), value: pack(values, 2),
                  recovered: pack(recovered, 1) });
    cur = rem;
    plain = nextPlain;
  }
  cases.push({ set: name, options, mustRecover,
               key: { f: pack(ntru.f, 2, -1), fp: pack(ntru.fp, 2), g: pack(ntru.g, 2, -1), h: pack(expandArray(ntru.h, N, 0), qb) },
               m: pack(ms, 1), e: pack(es, qb), rounds });
}
// one case per line
writeFileSync(join(outDir, 'mix_cases.json'),
  `{"generator":"gen_mix_cases.mjs","cases":[\n${cases.map(c => JSON.stringify(c)).join(',\n')}\n]}\n`);
console.log('mix_cases.json:', cases.map(c => `${c.set} ${c.rounds.map(r => r.recovered.b64).join('/')}`).join(', '));
}
main().catch(e => { console.error(e); process.exit(1); });
