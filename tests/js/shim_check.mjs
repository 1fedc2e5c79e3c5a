// checkWitnesses through the shim: the reference-captured witnesses of tests/golden/scheme_*.json are accepted, single-entry
// mutations give the flags of the closed form (include/ntru_engine.h NTRU_CHECK_*), malformed input throws.
// Usage: node tests/js/shim_check.mjs   (needs a GPU)
import { deepStrictEqual, throws } from 'assert';
import { readFileSync } from 'fs';
import { dirname, join } from 'path';
import { fileURLToPath } from 'url';

import { checkWitnesses } from '../../ntru-circom_amd/js/index.mjs';

const here = dirname(fileURLToPath(import.meta.url));
const golden = name => JSON.parse(readFileSync(join(here, '..', 'golden', name), 'utf8'));
const clone = w => JSON.parse(JSON.stringify(w));

const byTemplate = { VerifyEncrypt: [], VerifyDecrypt: [], VerifyInverse: [] };
for (const prof of ['n17_q32', 'n167_q128', 'n509_q2048', 'n821_q4096', 'n701_q8192']) {
  for (const key of golden(`scheme_${prof}.json`).keys) {
    for (const c of key.cases) { byTemplate.VerifyEncrypt.push(c.encrypt); byTemplate.VerifyDecrypt.push(c.decrypt); }
    for (const x of [...(key.sums || []), ...(key.degenerate || [])]) byTemplate.VerifyDecrypt.push(x.decrypt);
    for (const n of ['fq', 'fp', 'h']) byTemplate.VerifyInverse.push(key.verifyKeysInputs[n]);
  }
}
let total = 0;
for (const [template, ws] of Object.entries(byTemplate)) {
  const groups = new Map();
  for (const w of ws) { const k = JSON.stringify(w.params); if (!groups.has(k)) groups.set(k, []); groups.get(k).push(w); }
  for (const grp of groups.values()) { deepStrictEqual(checkWitnesses(template, grp), grp.map(() => 0)); total += grp.length; }
}
deepStrictEqual(total, 178);

const mutate = (w, name, idx, f) => { const m = clone(w); m.inputs[name][idx] = f(m.inputs[name][idx]); return m; };
const enc = byTemplate.VerifyEncrypt[0], dec = byTemplate.VerifyDecrypt[0], inv = byTemplate.VerifyInverse[0];
const [q, , N] = enc.params;
deepStrictEqual(checkWitnesses('VerifyEncrypt', [enc, mutate(enc, 'remainderE', 0, x => x + 1), mutate(enc, 'remainderE', 0, x => x + q),
  mutate(enc, 'quotientE', N, () => 1)]), [0, 1, 0, 3]);
deepStrictEqual(checkWitnesses('VerifyDecrypt', [mutate(dec, 'remainder2', 0, x => x + 1), mutate(dec, 'remainder1', 0, () => 65535)]), [8, 45]);
deepStrictEqual(checkWitnesses('VerifyInverse', [mutate(inv, 'remainderI', 0, x => x + 1)]), [1]);

// malformed input
const other = byTemplate.VerifyEncrypt.find(w => w.params[2] !== N);
throws(() => checkWitnesses('VerifyEncrypt', [enc, other]), /params/);
throws(() => checkWitnesses('VerifyEncrypt', [mutate(enc, 'r', 0, x => x)].map(w => { w.inputs.r.pop(); return w; })), /length/);
throws(() => checkWitnesses('VerifyEncrypt', [mutate(enc, 'm', 1, () => 65536)]), /\[0, 65535\]/);
throws(() => checkWitnesses('VerifyEncrypt', [mutate(enc, 'h', 1, () => -1)]), /\[0, 65535\]/);
throws(() => checkWitnesses('VerifyDecrypt', [mutate(dec, 'e', 2, () => 1.5)]), /\[0, 65535\]/);
throws(() => checkWitnesses('VerifyInverse', [enc]), /length 0/);
throws(() => checkWitnesses('VerifyCombine', [enc]), /unknown template/);
console.log(`shim_check: ${total} golden witnesses accepted, mutations and malformed input as expected`);
