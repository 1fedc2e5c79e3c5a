// The option lift: 'centred' of the Node shim: the captured 821 / 4096 ciphertexts decrypt to their plaintexts (decryptBits, decryptStr's
// route, decryptBatch), the first stage of the witness is the captured one, a tally with room to count (p = 7; inputs and expected counts
// written by tests/test_lift_js_gpu.py to <dir>/tally.json) returns the counts, the forms without a composed path throw an Error that names
// the option, and an instance without the option returns the captured reference objects as ever.
//   node tests/js/shim_lift.mjs <dir>
import assert from 'assert';
import { readFileSync } from 'fs';
import { dirname, join } from 'path';
import { fileURLToPath } from 'url';

import NTRU, { trimPolynomial } from '../../ntru-circom_amd/js/index.mjs';

const here = dirname(fileURLToPath(import.meta.url));
const [dir] = process.argv.slice(2);
const gold = JSON.parse(readFileSync(join(here, '..', 'golden', 'scheme_n821_q4096.json'), 'utf8'));
const key = gold.keys[0], opts = { ...gold.options, f: key.f, fp: key.fp, fq: key.fq, g: key.g, h: key.h };
const { N } = gold.options;

// ---- the captured cases
const plain = new NTRU(opts), centred = new NTRU({ ...opts, lift: 'centred' }), named = new NTRU({ ...opts, lift: 'reference' });
const B = key.cases.length;
const e = new Uint16Array(B * N), m = new Uint8Array(B * N);
key.cases.forEach((c, b) => { e.set(c.decrypt.inputs.e, b * N); m.set(c.m, b * N); });
for (const c of key.cases) {
  const d = c.decrypt;
  assert.deepStrictEqual(plain.decryptBits(d.inputs.e), d);                       // without the option: the reference's object
  assert.deepStrictEqual(named.decryptBits(d.inputs.e), d);
  const out = centred.decryptBits(d.inputs.e);
  assert.deepStrictEqual(out.value, trimPolynomial(c.m));
  assert.notDeepStrictEqual(d.value, trimPolynomial(c.m));                        // which the reference lift does not return
  assert.deepStrictEqual(out.inputs.quotient1, d.inputs.quotient1);
  assert.deepStrictEqual(out.inputs.remainder1, d.inputs.remainder1);
  assert.deepStrictEqual(out.inputs.remainder2, out.value.concat(new Array(N + 1 - out.value.length).fill(0)));
  assert.deepStrictEqual([out.inputs.f, out.inputs.fp, out.inputs.e, out.params], [d.inputs.f, d.inputs.fp, d.inputs.e, d.params]);
  assert.strictEqual(out.inputs.quotient2.length, N + 1);
}
const batch = centred.decryptBatch(e, B);
assert.deepStrictEqual(Array.from(batch.value), Array.from(m));
const first = plain.decryptBatch(e, B);
assert.deepStrictEqual(batch.quotient1, first.quotient1);
assert.deepStrictEqual(batch.remainder1, first.remainder1);
assert.notDeepStrictEqual(Array.from(first.value), Array.from(m));
for (let b = 0; b < B; b++) {                                                     // the batch rows are the single calls
  const one = centred.decryptBits(key.cases[b].decrypt.inputs.e);
  assert.deepStrictEqual(Array.from(batch.quotient2.subarray(b * N, (b + 1) * N)).concat([0]), one.inputs.quotient2);
}
const lean = centred.decryptBatch(e, B, false);
assert.deepStrictEqual([lean.quotient1, lean.remainder1, lean.quotient2], [null, null, null]);
assert.deepStrictEqual(Array.from(lean.value), Array.from(m));
const given = { value: new Uint8Array(B * N), remainder1: new Uint16Array(B * N) };
const into = centred.decryptBatch(e, B, true, given);
assert.ok(into.value === given.value && into.remainder1 === given.remainder1);
assert.deepStrictEqual(Array.from(given.value), Array.from(m));
// decryptStr: a string that fits N bits, encrypted by the instance itself
const text = 'the centred lift returns this';
assert.strictEqual(centred.decryptStr(centred.encryptStr(text)).replace(/\0+$/, ''), text);

// ---- a tally with room to count
const t = JSON.parse(readFileSync(join(dir, 'tally.json'), 'utf8'));
const tallyOpts = { N: t.N, q: t.q, p: t.p, f: t.f, fp: t.fp };
const rows = Uint16Array.from(t.e.flat());
const counted = new NTRU({ ...tallyOpts, lift: 'centred' }).tallyBatch(rows, t.G * t.K, Array.from({ length: t.G + 1 }, (_, g) => g * t.K));
assert.deepStrictEqual(Array.from(counted.value), t.counts.flat());
assert.strictEqual(counted.remainder1.length, t.G * t.N);
const leanTally = new NTRU({ ...tallyOpts, lift: 'centred' }).tallyBatch(rows, t.G * t.K, Array.from({ length: t.G + 1 }, (_, g) => g * t.K), null, false);
assert.deepStrictEqual(Array.from(leanTally.value), t.counts.flat());
assert.strictEqual(leanTally.remainder1, null);
const verbatim = new NTRU(tallyOpts).tallyBatch(rows, t.G * t.K, Array.from({ length: t.G + 1 }, (_, g) => g * t.K));
assert.notDeepStrictEqual(Array.from(verbatim.value), t.counts.flat());
assert.deepStrictEqual(counted.sum, verbatim.sum);
assert.deepStrictEqual(counted.remainder1, verbatim.remainder1);

// ---- the forms without a composed path throw, and name the option
const names = /lift: 'centred'/;
const none = null;
const refused = {
  decryptBatchAsync: () => centred.decryptBatchAsync(e, B),
  tallyBatchAsync: () => centred.tallyBatchAsync(e, B),
  pipelineAsync: () => centred.pipelineAsync({ m, B, r: new Uint8Array(B * N), decrypt: true }),
  decryptBytesAsync: () => centred.decryptBytesAsync(e, B),
  decryptBatchDev: () => centred.decryptBatchDev(none, none, none, B, none),
  tallyBatchDev: () => centred.tallyBatchDev(none, none, none, B, 1, none, none),
  decryptBatchPerKeyDev: () => centred.decryptBatchPerKeyDev(none, none, none, B, none),
  pipeline: () => centred.pipeline({ m, B, r: new Uint8Array(B * N), decrypt: true }),
  decryptBatchPerKey: () => centred.decryptBatchPerKey({ flags: new Uint8Array(B) }, e, B),
  decryptBytes: () => centred.decryptBytes(e, B),
  tallyPackedBatch: () => centred.tallyPackedBatch(new BigUint64Array(4), 1),
};
for (const [name, call] of Object.entries(refused)) assert.throws(call, names, name);
assert.throws(() => new NTRU({ ...opts, lift: 'center' }), /lift/);
// the encrypt-only pipeline has no lift in it and runs as ever
const r = centred.sampleR(Uint32Array.from([1, 2, 3, 4, 5, 6, 7, 8]), 0, B);
assert.deepStrictEqual(centred.pipeline({ m, B, r }).e, plain.pipeline({ m, B, r }).e);
console.log(`shim_lift: ${B} captured cases, tally of ${t.G} groups of ${t.K} at p = ${t.p}, ${Object.keys(refused).length} refused forms`);
