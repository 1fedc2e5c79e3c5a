// Sums of ciphertexts through the Node shim: sumCiphertexts and tallyBatch on every case of tests/golden/tally_cases.json (bit-identical
// to the reference's fold and decryptBits), then one ragged weighted batch that tests/test_ciphertext_sum_js_gpu.py wrote to <dir> as raw
// little-endian files (rows, weights, offsets, f, fp and the Python engine's sum / value / quotient1 / remainder1 / quotient2), through
// the host form and the *Dev twins.
//   node tests/js/shim_tally.mjs <dir>
import { readFileSync } from 'fs';
import { dirname, join } from 'path';
import { fileURLToPath } from 'url';

import NTRU, { sumCiphertexts, trimPolynomial } from '../../ntru-circom_amd/js/index.mjs';

const here = dirname(fileURLToPath(import.meta.url));
const [dir] = process.argv.slice(2);
const same = (a, b, what) => {
  if (a.length !== b.length) throw new Error(what + ': lengths differ');
  for (let i = 0; i < a.length; i++) if (a[i] !== b[i]) throw new Error(what + ': differs at ' + i);
};

// { bits, n, off, b64 } of tests/golden/gen_tally_cases.mjs -> Array of integers
function unpack(a) {
  const bytes = Buffer.from(a.b64, 'base64');
  return Array.from({ length: a.n }, (_, i) => {
    let x = 0;
    for (let b = 0; b < a.bits; b++) { const at = i * a.bits + b; if ((bytes[at >> 3] >> (at & 7)) & 1) x |= 1 << b; }
    return x + a.off;
  });
}
const rowsOf = (flat, K, N) => Array.from({ length: K }, (_, k) => flat.slice(k * N, (k + 1) * N));
const each = o => Object.fromEntries(Object.entries(o).map(([k, v]) => [k, unpack(v)]));

const { cases } = JSON.parse(readFileSync(join(here, '..', 'golden', 'tally_cases.json'), 'utf8'));
for (const c of cases) {
  c.key = each(c.key); c.e = rowsOf(unpack(c.e), c.K, c.options.N); c.sum = unpack(c.sum); c.expected = unpack(c.expected);
  c.decrypt.inputs = each(c.decrypt.inputs);
  const what = `${c.set} K=${c.K}`;
  same(sumCiphertexts(c.e, c.options.q, null, c.weights), trimPolynomial(c.sum), what + ' sumCiphertexts');
  const ntru = new NTRU({ ...c.options, ...c.key });
  const { N } = ntru;
  const t = ntru.tallyBatch(Uint16Array.from(c.e.flat()), c.K, null, c.weights ? Uint16Array.from(c.weights) : null);
  const inp = c.decrypt.inputs;
  for (const [got, name] of [[t.sum, 'e'], [t.quotient1, 'quotient1'], [t.remainder1, 'remainder1'], [t.quotient2, 'quotient2'],
    [t.value, 'remainder2']]) same(Array.from(got).concat(new Array(inp[name].length - N).fill(0)), inp[name], what + ' ' + name);
  if (c.recovered) same(Array.from(t.value), c.expected, what + ' homomorphic value');
}

async function raggedBatch() {
const meta = JSON.parse(readFileSync(join(dir, 'tally.json'), 'utf8'));
const { N, q, p, B, G } = meta;
const load = (T, name) => { const b = readFileSync(join(dir, name + '.bin')); return new T(b.buffer.slice(b.byteOffset, b.byteOffset + b.byteLength)); };
const rows = load(Uint16Array, 'rows'), weights = load(Uint16Array, 'weights'), offsets = load(BigInt64Array, 'offsets');
const f = load(Int8Array, 'f'), fp = load(Uint8Array, 'fp');
const want = { sum: load(Uint16Array, 'sum'), value: load(Uint8Array, 'value'), quotient1: load(Uint16Array, 'quotient1'),
  remainder1: load(Uint16Array, 'remainder1'), quotient2: load(Uint8Array, 'quotient2') };
const ntru = new NTRU({ N, q, p, f: Array.from(f), fp: Array.from(fp) });
const t = ntru.tallyBatch(rows, B, offsets, weights);
for (const k of Object.keys(want)) same(t[k], want[k], 'ragged ' + k);
const lean = ntru.tallyBatch(rows, B, offsets, weights, false);
if (lean.quotient1 !== null) throw new Error('value-only tally returned witnesses');
same(lean.value, want.value, 'value-only tally');
const later = await ntru.tallyBatchAsync(rows, B, offsets, weights);
for (const k of Object.keys(want)) same(later[k], want[k], 'async ' + k);

const up = a => { const d = NTRU.devAlloc(a.byteLength); NTRU.devUpload(d, a); return d; };
const [rD, wD, oD, fD, fpD] = [rows, weights, offsets, f, fp].map(up);
const n = G * N;
const sD = NTRU.devAlloc(2 * n), s2D = NTRU.devAlloc(2 * n), vD = NTRU.devAlloc(n), q1D = NTRU.devAlloc(2 * n), r1D = NTRU.devAlloc(2 * n),
  q2D = NTRU.devAlloc(n);
ntru.tallyBatchDev(fD, fpD, rD, B, G, sD, vD, { offsetsDev: oD, weightsDev: wD, q1Dev: q1D, r1Dev: r1D, q2Dev: q2D });
NTRU.sumGroupsDev(N, q, rD, B, G, s2D, { offsetsDev: oD, weightsDev: wD });
const down = (T, len, h) => NTRU.devDownload(new T(len), h);
same(down(Uint16Array, n, sD), want.sum, 'dev sum'); same(down(Uint16Array, n, s2D), want.sum, 'dev sumGroups');
same(down(Uint8Array, n, vD), want.value, 'dev value'); same(down(Uint16Array, n, q1D), want.quotient1, 'dev quotient1');
same(down(Uint16Array, n, r1D), want.remainder1, 'dev remainder1'); same(down(Uint8Array, n, q2D), want.quotient2, 'dev quotient2');
let refused = false;
try { NTRU.sumGroupsDev(N, q, rD, B * 2, G, s2D, { offsetsDev: oD }); } catch (err) { refused = true; }   // rows handle too small for 2 B rows
if (!refused) throw new Error('a rows handle that is too small was not refused');
for (const d of [rD, wD, oD, fD, fpD, sD, s2D, vD, q1D, r1D, q2D]) NTRU.devFree(d);
console.log(`shim_tally: ${cases.length} fixture cases, ragged batch of ${B} rows in ${G} groups`);
}
raggedBatch().catch(e => { console.error(e); process.exit(1); });
