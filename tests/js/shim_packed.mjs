// Packed ciphertexts through the Node shim: sumPackedCiphertexts and tallyPackedBatch, which the shim composes from unpackBatch, sumGroups
// and tallyDecryptBatch, on a batch that tests/test_packed_ciphertexts_js_gpu.py wrote to <dir> as raw little-endian files: the packed rows
// (every ignored bit set), weights, offsets, f, fp, and what the restatement and the Python engine's packed calls gave for them.
//   node tests/js/shim_packed.mjs <dir>
import { readFileSync } from 'fs';
import { join } from 'path';

import NTRU, { sumPackedCiphertexts } from '../../ntru-circom_amd/js/index.mjs';

const [dir] = process.argv.slice(2);
const same = (a, b, what) => {
  if (a.length !== b.length) throw new Error(what + ': lengths differ');
  for (let i = 0; i < a.length; i++) if (a[i] !== b[i]) throw new Error(what + ': differs at ' + i);
};
const { N, q, p, B, G } = JSON.parse(readFileSync(join(dir, 'packed.json'), 'utf8'));
const load = (T, name) => { const b = readFileSync(join(dir, name + '.bin')); return new T(b.buffer.slice(b.byteOffset, b.byteOffset + b.byteLength)); };
const packed = load(BigUint64Array, 'packed'), weights = load(Uint16Array, 'weights'), offsets = load(BigInt64Array, 'offsets');
const f = load(Int8Array, 'f'), fp = load(Uint8Array, 'fp');

same(sumPackedCiphertexts(packed, N, q, B, offsets, weights), load(Uint16Array, 'sum'), 'ragged weighted sum');
same(sumPackedCiphertexts(packed, N, q, B, offsets), load(Uint16Array, 'sum_plain'), 'ragged sum');
same(sumPackedCiphertexts(packed, N, q, B), load(Uint16Array, 'sum_all'), 'one group');

const ntru = new NTRU({ N, q, p, f: Array.from(f), fp: Array.from(fp) });
const t = ntru.tallyPackedBatch(packed, B, offsets, weights);
for (const k of ['sum', 'value', 'quotient1', 'remainder1', 'quotient2'])
  same(t[k], load(k === 'value' || k === 'quotient2' ? Uint8Array : Uint16Array, k), 'tally ' + k);
const lean = ntru.tallyPackedBatch(packed, B, offsets, weights, false);
if (lean.quotient1 !== null) throw new Error('value-only tally returned witnesses');
same(lean.value, t.value, 'value-only tally');
console.log(`shim_packed: ${B} packed rows of N=${N} q=${q} in ${G} groups`);
