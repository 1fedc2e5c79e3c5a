// Golden cases for byte messages: runs the UNMODIFIED reference under Node and records, for seeded keys and messages, what its
// encryptStr / decryptStr (index.js:80-86) do block by block.  A message is cut here into blocks of W = floor(N / 8) bytes (the
// reference itself takes at most N bits, index.js:81); for every block the file holds
//   chunk       the block's bytes (the last block of a message is NOT padded here: the shims pad it with zero bytes)
//   bits        stringToBits(chunk) (index.js:538-546), 8 bits per byte
//   r           the r that encryptBits drew for it (inputs.r: -1 already mapped to p - 1, index.js:89)
//   value       encryptBits(bits).value = encryptStr(chunk), expanded to N coefficients
//   decrypted   decryptBits(value).value expanded to N coefficients: the bit row decryptStr reads
//   str         decryptStr(value) as bytes
// The generator throws when a decryptStr differs from its chunk, so every committed case is one the reference itself recovers; since
// decryptStr trims trailing zero coefficients, no chunk ends in a zero byte.  Only the resulting JSON is committed; integer arrays are
// bit-packed { bits, n, off, b64 } as in gen_tally_cases.mjs (tests/message_bytes_ref.py and tests/js/shim_bytes.mjs unpack them).
//
//   node tests/golden/gen_bytes_cases.mjs [/root/reference] [outdir]
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
const { stringToBits, expandArray } = ref;

const sets = [
  ['n17_q32', { N: 17, q: 32, p: 3, df: 3, dg: 2, dr: 2 }],
  ['n167_q128_low_noise', { N: 167, q: 128, p: 3, df: 20, dg: 10, dr: 5 }],
  ['n167_q128_default', { N: 167, q: 128, p: 3, df: 61, dg: 20, dr: 18 }],
  ['n509_q2048', { N: 509, q: 2048, p: 3, df: 40, dg: 40, dr: 20 }],
];
const out = [];
let seed = 0xb17e5;
for (const [name, options] of sets) {
  state = (seed++ * 2654435761) >>> 0 || 1;
  const ntru = new NTRU({ ...options });
  ntru.generatePrivateKeyF();
  ntru.generateNewPublicKeyGH();
  const { N, q } = options, W = Math.floor(N / 8), qb = Math.log2(q);
  const lengths = [1, W - 1, W, W + 1, 2 * W, 3 * W + 1, 1, W, W + 1, 2 * W].filter(n => n >= 1);
  const messages = [];
  lengths.forEach((len, mi) => {
    const bytes = Array.from({ length: len }, () => nextU32() & 0xff);
    // interior 0x00 and 0xff where there is room, and no block (so no message either) that ends in a zero byte
    if (len >= 3) bytes[1 + (mi % (len - 2))] = 0x00;
    if (len >= 4) bytes[1 + ((mi + 1) % (len - 2))] = 0xff;
    for (let i = 0; i < len; i++) if ((i % W === W - 1 || i === len - 1) && bytes[i] === 0) bytes[i] = 1 + (nextU32() % 255);
    const blocks = [];
    for (let o = 0; o < len; o += W) {
      const chunk = bytes.slice(o, o + W);
      const str = String.fromCharCode(...chunk);
      const bits = stringToBits(str);
      const enc = ntru.encryptBits(bits);
      const back = ntru.decryptStr(enc.value);
      if (back !== str) throw new Error(`${name}: message ${mi}, block at ${o}: decryptStr does not return the chunk`);
      const decrypted = expandArray(ntru.decryptBits(enc.value).value, N, 0);
      blocks.push({ chunk: pack(chunk, 8), bits: pack(bits, 1), r: pack(enc.inputs.r, 2), value: pack(expandArray(enc.value, N, 0), qb),
                    decrypted: pack(decrypted, 2), str: pack(Array.from(back, c => c.charCodeAt(0)), 8) });
    }
    messages.push({ length: len, blocks });
  });
  out.push({ set: name, options, W,
             key: { f: pack(ntru.f, 2, -1), fp: pack(ntru.fp, 2), g: pack(ntru.g, 2, -1), h: pack(ntru.h, qb) }, messages });
}
// one message per line
const text = out.map(s => {
  const { messages, ...head } = s;
  return `${JSON.stringify(head).slice(0, -1)},"messages":[\n${messages.map(m => JSON.stringify(m)).join(',\n')}\n]}`;
}).join(',\n');
writeFileSync(join(outDir, 'bytes_cases.json'), `{"generator":"gen_bytes_cases.mjs","sets":[\n${text}\n]}\n`);
console.log('bytes_cases.json:', out.map(s => `${s.set} W=${s.W} ${s.messages.length} messages, ${s.messages.reduce((a, m) => a + m.blocks.length, 0)} blocks`).join('; '));
}
main().catch(e => { console.error(e); process.exit(1); });
