// Golden cases for scanning a batch of ciphertexts for the rows a key decrypts to a well-formed, tagged message: runs the UNMODIFIED
// reference under Node and records, for seeded key pairs and messages, the reference's decryptBits(e).value (index.js:111-140) of every
// row under every key, and what follows from it by the definition in include/ntru_engine.h ("scanning"):
//   row b is a hit for key k  <=>  value, extended to N coefficients, has only 0 / 1 among its first 8 W coefficients (W = N >> 3 message
//                                  bytes, most significant bit first as stringToBits, index.js:538-546), 0 in every later one, and
//                                  the message bytes [tagOffset, tagOffset + tag.length) equal the tag.
// Per set: K = 3 key pairs and 11 rows -- two tagged messages encrypted (encryptBits, index.js:87-110) under each key, one message per
// key whose tag has one bit flipped, two rows of arbitrary values below q.  Recorded: `value` [K][B][N], `hit` [K][B] and, per key, the
// hits in row order with their W message bytes.
// The first two sets use moduli where the lift of index.js:117 is right (q = 2 mod 3): every tagged row must be a hit under its own key
// and every wrong-tag row a miss, every key must have a hit and a miss, else this generator throws (pick another seed).  The third set
// (q = 256 = 1 mod 3) has the lift wrong: its honest rows are expected to miss under the reference's lift, and the generator throws if
// one does not.
// Only the resulting JSON is committed.  Integer arrays are stored bit-packed as in gen_mix_cases.mjs: { bits, n, off, b64 } holds n values
// v with v - off in [0, 2^bits), least significant bit first, as base64; tests/scan_ref.py and tests/js/shim_scan.mjs unpack them.
//
//   node tests/golden/gen_scan_cases.mjs <directory of the reference> [outdir]
import { writeFileSync } from 'fs';
import { dirname, join } from 'path';
import { fileURLToPath, pathToFileURL } from 'url';

const here = dirname(fileURLToPath(import.meta.url));
const refDir = process.argv[2];
const outDir = process.argv[3] || here;
if (!refDir) { console.error('usage: node gen_scan_cases.mjs <directory of the reference> [outdir]'); process.exit(2); }
let state = 1;
function nextU32() { let x = state; x ^= x << 13; x >>>= 0; x ^= x >>> 17; x ^= x << 5; x >>>= 0; state = x; return x; }
globalThis.crypto = { getRandomValues(arr) { for (let i = 0; i < arr.length; i++) arr[i] = nextU32(); return arr; } };

function pack(values, bits, off = 0) {
  const flat = values.flat(Infinity);
  const bytes = Buffer.alloc(Math.ceil(flat.length * bits / 8));
  flat.forEach((v, i) => {
    const x = v - off;
    if (!Number.isInteger(x) || x < 0 || x >= 2 ** bits) throw new Error(`pack: ${v} does not fit ${bits} bits at offset ${off}`);
    for (let b = 0; b < bits; b++) if ((x >> b) & 1) { const at = i * bits + b; bytes[at >> 3] |= 1 << (at & 7); }
  });
  return { bits, n: flat.length, off, b64: bytes.toString('base64') };
}

const bitsOf = bytes => bytes.flatMap(x => Array.from({ length: 8 }, (_, j) => (x >> (7 - j)) & 1));

// The definition: the W message bytes of `value` [N] when it is a hit, else null.
function hitBytes(value, N, W, tag, tagOffset) {
  if (value.some((v, i) => (i < 8 * W ? v > 1 : v !== 0))) return null;
  const bytes = Array.from({ length: W }, (_, i) => value.slice(8 * i, 8 * i + 8).reduce((a, b) => 2 * a + b, 0));
  return tag.every((t, j) => bytes[tagOffset + j] === t) ? bytes : null;
}

async function main() {
const ref = await import(pathToFileURL(join(refDir, 'index.js')).href);
const NTRU = ref.default;
const { trimPolynomial, expandArray } = ref;

// [set name, options, tag, tagOffset, is the lift of index.js:117 right for this q?]
const sets = [
  ['n17_q32', { N: 17, q: 32, p: 3, df: 3, dg: 2, dr: 1 }, [0xc3], 1, true],
  ['n167_q128', { N: 167, q: 128, p: 3, df: 20, dg: 10, dr: 5 }, [0x4e, 0x54, 0x52, 0x55], 3, true],
  ['n167_q256_lift_off', { N: 167, q: 256, p: 3, df: 20, dg: 10, dr: 5 }, [0x4e, 0x54, 0x52, 0x55], 3, false],
];
const K = 3;
const cases = [];
// seed: the first of those tried under which the three sets meet the conditions above
let seed = Number(process.env.SCAN_SEED || 0x5ca701);
for (const [name, options, tag, tagOffset, liftRight] of sets) {
  state = (seed++ * 2654435761) >>> 0 || 1;
  const { N, q } = options;
  const qb = Math.log2(q), W = N >> 3;
  const keys = [];
  for (let k = 0; k < K; k++) {
    const ntru = new NTRU({ ...options });
    ntru.generatePrivateKeyF();
    ntru.generateNewPublicKeyGH();
    keys.push(ntru);
  }
  const message = flip => {
    const bytes = Array.from({ length: W }, () => nextU32() & 255);
    tag.forEach((t, j) => { bytes[tagOffset + j] = t; });
    if (flip) bytes[tagOffset + (nextU32() % tag.length)] ^= 1 << (nextU32() % 8);
    return bytes;
  };
  const rows = [], kinds = [], plain = [];
  const add = (k, kind, bytes) => {
    rows.push(expandArray(keys[k].encryptBits(bitsOf(bytes)).value, N, 0));
    kinds.push({ key: k, kind });
    plain.push(bytes);
  };
  for (let k = 0; k < K; k++) add(k, 'tagged', message(false));
  for (let k = 0; k < K; k++) add(k, 'wrong_tag', message(true));
  for (let k = 0; k < K; k++) add(k, 'tagged', message(false));
  for (let i = 0; i < 2; i++) {
    rows.splice(3 + 5 * i, 0, Array.from({ length: N }, () => nextU32() % q));
    kinds.splice(3 + 5 * i, 0, { key: -1, kind: 'arbitrary' });
    plain.splice(3 + 5 * i, 0, null);
  }
  const B = rows.length;
  const values = [], hit = [], hits = [];
  for (let k = 0; k < K; k++) {
    const vk = [], hk = [], list = [];
    for (let b = 0; b < B; b++) {
      const value = expandArray(keys[k].decryptBits(trimPolynomial(rows[b])).value, N, 0);
      const bytes = hitBytes(value, N, W, tag, tagOffset);
      vk.push(value);
      hk.push(bytes ? 1 : 0);
      if (bytes) list.push({ row: b, bytes });
      const own = kinds[b].key === k;
      if (liftRight && own && kinds[b].kind === 'tagged' && JSON.stringify(bytes) !== JSON.stringify(plain[b]))
        throw new Error(`${name}: key ${k} does not recover its tagged row ${b}`);
      if (liftRight && own && kinds[b].kind === 'wrong_tag' && bytes) throw new Error(`${name}: wrong-tag row ${b} is a hit`);
      if (!liftRight && own && bytes) throw new Error(`${name}: honest row ${b} is a hit although the lift is off`);
    }
    if (liftRight && (!hk.includes(1) || !hk.includes(0))) throw new Error(`${name}: key ${k} lacks a hit or a miss`);
    values.push(vk); hit.push(hk); hits.push(list);
  }
  cases.push({ set: name, options, liftRight, W, tag, tagOffset, kinds,
               keys: keys.map(n => ({ f: pack(n.f, 2, -1), fp: pack(expandArray(n.fp, N, 0), 2), h: pack(expandArray(n.h, N, 0), qb) })),
               e: pack(rows, qb), value: pack(values, 2), hit: pack(hit, 1), hits });
}
// one case per line
writeFileSync(join(outDir, 'scan_cases.json'),
  `{"generator":"gen_scan_cases.mjs","cases":[\n${cases.map(c => JSON.stringify(c)).join(',\n')}\n]}\n`);
console.log('scan_cases.json:', cases.map(c => `${c.set} ${c.hits.map(l => l.map(h => h.row).join('+')).join('/')}`).join(', '));
}
main().catch(e => { console.error(e); process.exit(1); });
