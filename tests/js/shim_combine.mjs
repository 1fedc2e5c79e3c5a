// Combinations of ciphertexts through the Node shim: combineCiphertexts and ntru.combineBatch on every case of
// tests/golden/combine_cases.json (bit-identical to the reference's fold and decryptBits), with the weight matrix as an Array of rows and
// as a Uint16Array with G, and the refusals of a malformed matrix.
//   node tests/js/shim_combine.mjs
import { readFileSync } from 'fs';
import { dirname, join } from 'path';
import { fileURLToPath } from 'url';

import NTRU, { combineCiphertexts, sumCiphertexts, trimPolynomial } from '../../ntru-circom_amd/js/index.mjs';

const here = dirname(fileURLToPath(import.meta.url));
const same = (a, b, what) => {
  if (a.length !== b.length) throw new Error(what + ': lengths differ');
  for (let i = 0; i < a.length; i++) if (a[i] !== b[i]) throw new Error(what + ': differs at ' + i);
};

// { bits, n, off, b64 } of tests/golden/gen_combine_cases.mjs -> Array of integers
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
const throws = (fn, what) => { let t = false; try { fn(); } catch (err) { t = true; } if (!t) throw new Error(what + ' was not refused'); };

const { sets } = JSON.parse(readFileSync(join(here, '..', 'golden', 'combine_cases.json'), 'utf8'));
let outputs = 0;
for (const s of sets) {
  const { N, q } = s.options;
  const key = each(s.key), e = rowsOf(unpack(s.e), s.B, N);
  const ntru = new NTRU({ ...s.options, ...key });
  const flat = Uint16Array.from(e.flat());
  for (const c of s.cases) {
    const what = `${s.set} ${c.kind}`;
    const sums = c.outputs.map(o => unpack(o.sum));
    const got = combineCiphertexts(e, q, c.weights);
    const typed = combineCiphertexts(e, q, Uint16Array.from(c.weights.flat()), c.G);
    const t = ntru.combineBatch(flat, s.B, c.weights);
    const t2 = ntru.combineBatch(flat, s.B, Uint16Array.from(c.weights.flat()), c.G, false);
    if (t2.quotient1 !== null) throw new Error(what + ': value-only combination returned witnesses');
    same(t2.value, t.value, what + ' value-only');
    c.outputs.forEach((o, g) => {
      same(got[g], trimPolynomial(sums[g]), `${what} combineCiphertexts ${g}`);
      same(typed[g], got[g], `${what} combineCiphertexts (typed) ${g}`);
      same(got[g], sumCiphertexts(e, q, null, c.weights.map(r => r[g])), `${what} column ${g} through sumCiphertexts`);
      const inp = each(o.decrypt.inputs), row = a => Array.from(a.subarray(g * N, (g + 1) * N));
      for (const [arr, name] of [[t.sum, 'e'], [t.quotient1, 'quotient1'], [t.remainder1, 'remainder1'], [t.quotient2, 'quotient2'],
        [t.value, 'remainder2']]) same(row(arr).concat(new Array(inp[name].length - N).fill(0)), inp[name], `${what} ${g} ${name}`);
      if (o.recovered) same(trimPolynomial(row(t.value)), trimPolynomial(unpack(o.expected)), `${what} ${g} homomorphic value`);
      outputs++;
    });
  }
  throws(() => combineCiphertexts(e, q, s.cases[0].weights.slice(1)), 'a weight matrix with a row missing');
  throws(() => combineCiphertexts(e, q, new Uint16Array(s.B * 2), 3), 'a typed weight matrix of the wrong size');
  throws(() => ntru.combineBatch(flat, s.B, new Uint16Array(s.B)), 'a typed weight matrix without G');
}
console.log(`shim_combine: ${sets.length} sets, ${outputs} combinations`);
