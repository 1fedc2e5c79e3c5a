// Byte messages through the Node shim: encryptBytes / decryptBytes on every message of tests/golden/bytes_cases.json with the recorded r
// (the reference's ciphertexts block by block, then the message back with flags 0), a wrong key of the same N (flagged), the refusal of a
// string above latin-1, and one batch that tests/test_message_bytes_js_gpu.py wrote to <dir> as raw files (data, r, key and the Python
// engine's e / out / flags) through the synchronous and the Async forms.
//   node tests/js/shim_bytes.mjs <dir>
import { readFileSync } from 'fs';
import { dirname, join } from 'path';
import { fileURLToPath } from 'url';

import NTRU from '../../ntru-circom_amd/js/index.mjs';

const here = dirname(fileURLToPath(import.meta.url));
const [dir] = process.argv.slice(2);
const same = (a, b, what) => {
  if (a.length !== b.length) throw new Error(`${what}: lengths differ (${a.length}, ${b.length})`);
  for (let i = 0; i < a.length; i++) if (a[i] !== b[i]) throw new Error(what + ': differs at ' + i);
};

// { bits, n, off, b64 } of tests/golden/gen_bytes_cases.mjs -> Array of integers
function unpack(a) {
  const bytes = Buffer.from(a.b64, 'base64');
  return Array.from({ length: a.n }, (_, i) => {
    let x = 0;
    for (let b = 0; b < a.bits; b++) { const at = i * a.bits + b; if ((bytes[at >> 3] >> (at & 7)) & 1) x |= 1 << b; }
    return x + a.off;
  });
}
const each = o => Object.fromEntries(Object.entries(o).map(([k, v]) => [k, unpack(v)]));

async function main() {
const { sets } = JSON.parse(readFileSync(join(here, '..', 'golden', 'bytes_cases.json'), 'utf8'));
let nMessages = 0;
const byN = {};
for (const s of sets) {
  const ntru = new NTRU({ ...s.options, ...each(s.key) });
  const { N } = ntru;
  if (ntru.bytesPerBlock !== s.W) throw new Error(s.set + ': bytesPerBlock');
  (byN[N] = byN[N] || []).push({ ntru, s, values: [] });
  for (const m of s.messages) {
    const blocks = m.blocks.map(each), what = `${s.set} length ${m.length}`;
    const data = Uint8Array.from(blocks.flatMap(b => b.chunk)), r = Uint8Array.from(blocks.flatMap(b => b.r));
    const value = blocks.flatMap(b => b.value);
    byN[N][byN[N].length - 1].values.push(value);
    const e = ntru.encryptBytes(data, r);
    same(Array.from(e), value, what + ' ciphertext');
    same(Array.from(ntru.encryptBytes(String.fromCharCode(...data), blocks.map(b => b.r))), value, what + ' ciphertext of the string');
    const back = ntru.decryptBytes(e, blocks.length, m.length);
    same(back.data, data, what + ' message');
    same(back.flags, new Uint8Array(blocks.length), what + ' flags');
    same(ntru.decryptBytes(e, blocks.length).data, data, what + ' message, stripped');
    const later = await ntru.decryptBytesAsync(await ntru.encryptBytesAsync(data, r), blocks.length, m.length);
    same(later.data, data, what + ' async message');
    nMessages++;
  }
}
// another key of the same N: at least one block is flagged
for (const group of Object.values(byN)) {
  if (group.length < 2) continue;
  const [a, b] = group;
  const flat = a.values.flat();
  const { flags } = b.ntru.decryptBytes(Uint16Array.from(flat), flat.length / a.ntru.N);
  if (!flags.some(x => x !== 0)) throw new Error('a wrong key was not flagged');
  if (flags.some(x => x & ~96)) throw new Error('unknown flag bits');
}
let refused = false;
try { new NTRU(sets[1].options).encryptBytes('snow ☃'); } catch (err) { refused = /latin-1/.test(err.message); }
if (!refused) throw new Error('a string above latin-1 was not refused');

// the batch of the Python engine
const meta = JSON.parse(readFileSync(join(dir, 'bytes.json'), 'utf8'));
const load = (T, name) => { const b = readFileSync(join(dir, name + '.bin')); return new T(b.buffer.slice(b.byteOffset, b.byteOffset + b.byteLength)); };
const ntru = new NTRU({ ...meta.options, h: Array.from(load(Uint16Array, 'h')), f: Array.from(load(Int8Array, 'f')), fp: Array.from(load(Uint8Array, 'fp')) });
const data = load(Uint8Array, 'data'), r = load(Uint8Array, 'r');
const e = ntru.encryptBytes(data, r);
same(e, load(Uint16Array, 'e'), 'batch ciphertext');
const mixed = load(Uint16Array, 'e_mixed');
const got = ntru.decryptBytes(mixed, meta.blocks, meta.blocks * ntru.bytesPerBlock);
same(got.data, load(Uint8Array, 'out'), 'batch message');
same(got.flags, load(Uint8Array, 'flags'), 'batch flags');
const got2 = await ntru.decryptBytesAsync(mixed, meta.blocks, meta.length);
same(got2.data, load(Uint8Array, 'out').slice(0, meta.length), 'batch message, async, cut');
console.log(`shim_bytes: ${nMessages} fixture messages, batch of ${meta.blocks} blocks`);
}
main().catch(e => { console.error(e); process.exit(1); });
