// Golden cases for counting the decrypted byte messages of a batch by choice and group: runs the UNMODIFIED reference under Node and
// records, for seeded key pairs and ballots, the reference's decryptBits(e).value (index.js:111-140) of every row under the counting key,
// and what follows from it by the definition in include/ntru_engine.h ("counting"), with W = N >> 3 message bytes, most significant bit
// first as stringToBits (index.js:538-546):
//   cls(b) = nChoices + 2 (malformed)   value, extended to N coefficients, has something above 1 among its first 8 W coefficients or
//                                       something other than 0 behind them;
//            nChoices + 1 (bad tag)     else, the message bytes [tagOffset, tagOffset + tag.length) differ from the tag;
//            nChoices     (other)       else, v = the big-endian integer of the bytes [fieldOffset, fieldOffset + fieldLength) lies
//                                       outside [firstChoice, firstChoice + nChoices);
//            v - firstChoice            otherwise;
//   count[g][c] = the rows with group[b] == g and cls(b) == c.
// Per set: the counting key pair, a second "foreign" key pair, and 16 rows -- nine honest ballots for four different choices, one ballot
// with v = firstChoice - 1, one with v = firstChoice + nChoices, one whose tag has one bit flipped (all encrypted with encryptBits,
// index.js:87-110, under the counting key), two honest-looking ballots encrypted under the foreign key, two rows of arbitrary values
// below q -- with group ids in {0, 1, 2}.
// The first two sets use moduli where the lift of index.js:117 is right (q = 2 mod 3): every honest ballot must land in its own choice
// bin, and a choice bin, OTHER, BAD_TAG and MALFORMED must each be non-empty, else this generator throws (pick another seed).  The
// third set (q = 256 = 1 mod 3) has the lift wrong: no honest ballot may land in a choice bin under the reference's lift, and the
// generator throws if one does.
// Only the resulting JSON is committed.  Integer arrays are stored bit-packed as in gen_scan_cases.mjs: { bits, n, off, b64 } holds n
// values v with v - off in [0, 2^bits), least significant bit first, as base64; tests/count_ref.py unpacks them.
//
//   node tests/golden/gen_count_cases.mjs <directory of the reference> [outdir]
import { writeFileSync } from 'fs';
import { dirname, join } from 'path';
import { fileURLToPath, pathToFileURL } from 'url';

const here = dirname(fileURLToPath(import.meta.url));
const refDir = process.argv[2];
const outDir = process.argv[3] || here;
if (!refDir) { console.error('usage: node gen_count_cases.mjs <directory of the reference> [outdir]'); process.exit(2); }
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

// The definition: the class of `value` [N] under the layout `lay`.
function classOf(value, W, lay) {
  const { tag, tagOffset, fieldOffset, fieldLength, firstChoice, nChoices } = lay;
  if (value.some((v, i) => (i < 8 * W ? v > 1 : v !== 0))) return nChoices + 2;
  const bytes = Array.from({ length: W }, (_, i) => value.slice(8 * i, 8 * i + 8).reduce((a, b) => 2 * a + b, 0));
  if (!tag.every((t, j) => bytes[tagOffset + j] === t)) return nChoices + 1;
  let v = 0;
  for (let j = 0; j < fieldLength; j++) v = v * 256 + bytes[fieldOffset + j];
  return v < firstChoice || v - firstChoice >= nChoices ? nChoices : v - firstChoice;
}

async function main() {
const ref = await import(pathToFileURL(join(refDir, 'index.js')).href);
const NTRU = ref.default;
const { trimPolynomial, expandArray } = ref;

// [set name, options, layout, is the lift of index.js:117 right for this q?]
const small = { tag: [0xc3], tagOffset: 1, fieldOffset: 0, fieldLength: 1, firstChoice: 1, nChoices: 4 };
const large = { tag: [0x4e, 0x54, 0x52, 0x55], tagOffset: 3, fieldOffset: 8, fieldLength: 2, firstChoice: 0x0100, nChoices: 5 };
const sets = [
  ['n17_q32', { N: 17, q: 32, p: 3, df: 3, dg: 2, dr: 1 }, small, true],
  ['n167_q128', { N: 167, q: 128, p: 3, df: 20, dg: 10, dr: 5 }, large, true],
  ['n167_q256_lift_off', { N: 167, q: 256, p: 3, df: 20, dg: 10, dr: 5 }, large, false],
];
// the rows of a set in order: [kind, choice (an index; -1 and nChoices are the two outside the range)]
const plan = n => [['honest', 0], ['honest', 1], ['foreign', 1], ['honest', 2], ['below', -1], ['arbitrary', null], ['honest', 0],
                   ['honest', 3], ['wrong_tag', 2], ['honest', 1], ['above', n], ['foreign', 0], ['honest', 2], ['arbitrary', null],
                   ['honest', 0], ['honest', 3]];
const cases = [];
// seed: the first of those tried under which the three sets meet the conditions above
let seed = Number(process.env.COUNT_SEED || 0xc0117);
for (const [name, options, lay, liftRight] of sets) {
  state = (seed++ * 2654435761) >>> 0 || 1;
  const { N, q } = options;
  const qb = Math.log2(q), W = N >> 3, n = lay.nChoices;
  const keys = [];
  for (let k = 0; k < 2; k++) {                    // 0: the counting key, 1: the foreign key
    const ntru = new NTRU({ ...options });
    ntru.generatePrivateKeyF();
    ntru.generateNewPublicKeyGH();
    keys.push(ntru);
  }
  const ballot = (choice, flip) => {
    const bytes = Array.from({ length: W }, () => nextU32() & 255);
    lay.tag.forEach((t, j) => { bytes[lay.tagOffset + j] = t; });
    const v = lay.firstChoice + choice;
    for (let j = 0; j < lay.fieldLength; j++) bytes[lay.fieldOffset + j] = Math.floor(v / 256 ** (lay.fieldLength - 1 - j)) & 255;
    if (flip) bytes[lay.tagOffset + (nextU32() % lay.tag.length)] ^= 1 << (nextU32() % 8);
    return bytes;
  };
  const rows = [], kinds = [], group = [], value = [], cls = [];
  const count = Array.from({ length: 3 }, () => new Array(n + 3).fill(0));
  for (const [kind, choice] of plan(n)) {
    rows.push(kind === 'arbitrary' ? Array.from({ length: N }, () => nextU32() % q)
      : expandArray(keys[kind === 'foreign' ? 1 : 0].encryptBits(bitsOf(ballot(choice, kind === 'wrong_tag'))).value, N, 0));
    kinds.push({ kind, choice });
    group.push(nextU32() % 3);
  }
  rows.forEach((row, b) => {
    const val = expandArray(keys[0].decryptBits(trimPolynomial(row)).value, N, 0);
    const c = classOf(val, W, lay);
    value.push(val); cls.push(c);
    count[group[b]][c]++;
    const { kind, choice } = kinds[b];
    if (liftRight && kind === 'honest' && c !== choice) throw new Error(`${name}: honest row ${b} for choice ${choice} has class ${c}`);
    if (!liftRight && kind === 'honest' && c < n) throw new Error(`${name}: honest row ${b} is in a choice bin although the lift is off`);
  });
  const total = c => count.reduce((s, g) => s + g[c], 0);
  if (liftRight && ![n, n + 1, n + 2].every(c => total(c) > 0)) throw new Error(`${name}: OTHER, BAD_TAG or MALFORMED is empty`);
  if (liftRight && !Array.from({ length: n }, (_, c) => total(c)).some(x => x > 0)) throw new Error(`${name}: no choice bin is filled`);
  cases.push({ set: name, options, liftRight, W, ...lay, G: 3, kinds, group,
               keys: keys.map(k => ({ f: pack(k.f, 2, -1), fp: pack(expandArray(k.fp, N, 0), 2), h: pack(expandArray(k.h, N, 0), qb) })),
               e: pack(rows, qb), value: pack(value, 2), cls, count });
}
// one case per line
writeFileSync(join(outDir, 'count_cases.json'),
  `{"generator":"gen_count_cases.mjs","cases":[\n${cases.map(c => JSON.stringify(c)).join(',\n')}\n]}\n`);
console.log('count_cases.json:', cases.map(c => `${c.set} ${c.cls.join(' ')}`).join(', '));
}
main().catch(e => { console.error(e); process.exit(1); });
