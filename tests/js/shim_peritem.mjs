// One key pair per item through the Node shim: encryptBatchPerKey / decryptBatchPerKey on a generateKeysBatch result, their *Dev twins
// on device handles (checked against the host forms here), and the 'Could not find invertible f' refusal.  Writes r, m and every result
// array to <out dir> as raw little-endian files plus peritem.json; tests/test_peritem_scheme_js_gpu.py compares them with the Python engine.
//   node tests/js/shim_peritem.mjs <profile> <B> <out dir>
import { readFileSync, writeFileSync } from 'fs';
import { dirname, join } from 'path';
import { fileURLToPath } from 'url';

import NTRU from '../../ntru-circom_amd/js/index.mjs';

const here = dirname(fileURLToPath(import.meta.url));
const [profile, Bs, outDir] = process.argv.slice(2);
const B = Number(Bs);
const opts = JSON.parse(readFileSync(join(here, '..', 'golden', `scheme_${profile}.json`), 'utf8')).options;
const ntru = new NTRU({ ...opts });
const { N } = ntru;
const key = Uint32Array.from([11, 22, 33, 44, 55, 66, 77, 88]);
const rKey = Uint32Array.from([1, 3, 5, 7, 9, 11, 13, 15]);
const dump = (name, a) => writeFileSync(join(outDir, name + '.bin'), Buffer.from(a.buffer, a.byteOffset, a.byteLength));
const same = (a, b, what) => {
  if (a.length !== b.length) throw new Error(what + ': lengths differ');
  for (let i = 0; i < a.length; i++) if (a[i] !== b[i]) throw new Error(what + ': differs at ' + i);
};

const keys = ntru.generateKeysBatch({ B, key });
for (let b = 0; b < B; b++) if (keys.flags[b]) throw new Error('a key pair of this profile failed: pick another key');
const n = B * N;
const r = ntru.sampleR(rKey, 0, B);
const m = new Uint8Array(n);
for (let i = 0; i < n; i++) m[i] = (i * 7 + (i >> 5)) % 3;

// host forms
const enc = ntru.encryptBatchPerKey(keys, r, m, B);
const dec = ntru.decryptBatchPerKey(keys, enc.e, B);
const lean = ntru.decryptBatchPerKey(keys, enc.e, B, false);
if (lean.quotient1 !== null) throw new Error('value-only decrypt returned witnesses');
same(lean.value, dec.value, 'value-only decrypt');

// device forms on the same keys
const up = a => { const d = NTRU.devAlloc(a.byteLength); NTRU.devUpload(d, a); return d; };
const [hD, fD, fpD, rD, mD] = [keys.h, keys.f, keys.fp, r, m].map(up);
const eD = NTRU.devAlloc(2 * n), qD = NTRU.devAlloc(2 * n), vD = NTRU.devAlloc(n), q1D = NTRU.devAlloc(2 * n), r1D = NTRU.devAlloc(2 * n),
  q2D = NTRU.devAlloc(n);
ntru.encryptBatchPerKeyDev(hD, rD, mD, B, eD, qD);
ntru.decryptBatchPerKeyDev(fD, fpD, eD, B, vD, q1D, r1D, q2D);
const down = (T, len, h) => NTRU.devDownload(new T(len), h);
same(down(Uint16Array, n, eD), enc.e, 'dev e'); same(down(Uint16Array, n, qD), enc.quotientE, 'dev quotientE');
same(down(Uint8Array, n, vD), dec.value, 'dev value'); same(down(Uint16Array, n, q1D), dec.quotient1, 'dev quotient1');
same(down(Uint16Array, n, r1D), dec.remainder1, 'dev remainder1'); same(down(Uint8Array, n, q2D), dec.quotient2, 'dev quotient2');
for (const d of [hD, fD, fpD, rD, mD, eD, qD, vD, q1D, r1D, q2D]) NTRU.devFree(d);

// a flagged item is refused like loadKeyFromBatch refuses it
const flagged = { ...keys, flags: Uint8Array.from(keys.flags) };
flagged.flags[B - 1] = 1;
let refused = false;
try { ntru.encryptBatchPerKey(flagged, r, m, B); } catch (err) { refused = err.message === 'Could not find invertible f'; }
if (!refused) throw new Error('a flagged key was not refused');

for (const [name, a] of Object.entries({ r, m, e: enc.e, quotientE: enc.quotientE, value: dec.value, quotient1: dec.quotient1,
  remainder1: dec.remainder1, quotient2: dec.quotient2 })) dump(name, a);
writeFileSync(join(outDir, 'peritem.json'), JSON.stringify({ N, q: ntru.q, p: ntru.p, B, key: Array.from(key) }));
console.log(`shim_peritem: ${B} items, one key pair each`);
