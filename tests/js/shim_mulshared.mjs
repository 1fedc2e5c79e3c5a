// A batch times one shared polynomial through the Node shim: multiplyByPolynomialBatch and ntru.multiplyByPolynomialBatch on the cases
// of tests/golden/mulshared_cases.json (the reference's multiplyPolynomials + dividePolynomials(., I, q), N = 17 / q = 32 among them),
// against the shim's own reference-style pair per row, with a signed polynomial, and the refusals of malformed arguments.
//   node tests/js/shim_mulshared.mjs
import { readFileSync } from 'fs';
import { dirname, join } from 'path';
import { fileURLToPath } from 'url';

import NTRU, { dividePolynomials, multiplyByPolynomialBatch, multiplyPolynomials } from '../../ntru-circom_amd/js/index.mjs';

const here = dirname(fileURLToPath(import.meta.url));
const same = (a, b, what) => {
  if (a.length !== b.length) throw new Error(what + ': lengths differ');
  for (let i = 0; i < a.length; i++) if (a[i] !== b[i]) throw new Error(what + ': differs at ' + i);
};
const padded = (a, n) => Array.from(a).concat(new Array(n - a.length).fill(0));
const throws = (fn, what) => { let t = false; try { fn(); } catch (err) { t = true; } if (!t) throw new Error(what + ' was not refused'); };

const { sets } = JSON.parse(readFileSync(join(here, '..', 'golden', 'mulshared_cases.json'), 'utf8'));
let rowsDone = 0;
for (const s of sets) {
  const { N, q } = s, B = s.rows.length;
  const flat = Uint16Array.from(s.rows.flat());
  const I = new Array(N + 1).fill(0);
  I[0] = 1; I[N] = -1;
  const both = multiplyByPolynomialBatch(flat, N, q, B, s.s, true);
  const rem = multiplyByPolynomialBatch(flat, N, q, B, s.s);
  same(rem, both.remainder, `N=${N} remainder-only`);
  const ntru = new NTRU({ N, q, p: 3, df: 1, dg: 1, dr: 1 });
  same(ntru.multiplyByPolynomialBatch(flat, B, s.s), rem, `N=${N} NTRU method`);
  // a signed polynomial is the same polynomial modulo q
  same(multiplyByPolynomialBatch(flat, N, q, B, s.s.map(v => (v > q / 2 ? v - q : v))), rem, `N=${N} signed coefficients`);
  s.cases.forEach((c, b) => {
    const row = a => Array.from(a.subarray(b * N, (b + 1) * N));
    same(row(both.quotient), padded(c.quotient, N), `N=${N} row ${b} quotient (fixture)`);
    same(row(both.remainder), padded(c.remainder, N), `N=${N} row ${b} remainder (fixture)`);
    const d = dividePolynomials(multiplyPolynomials(s.rows[b], s.s, q), I, q);
    same(row(both.quotient), padded(d.quotient, N), `N=${N} row ${b} quotient (shim, reference style)`);
    same(row(both.remainder), padded(d.remainder, N), `N=${N} row ${b} remainder (shim, reference style)`);
    rowsDone++;
  });
  same(multiplyByPolynomialBatch(new Uint16Array(0), N, q, 0, s.s), new Uint16Array(0), `N=${N} no rows`);
  throws(() => multiplyByPolynomialBatch(flat, N, q, B, new Array(N + 1).fill(1)), 'a polynomial longer than N');
  throws(() => multiplyByPolynomialBatch(flat, N, q, B + 1, s.s), 'rows of the wrong size');
  throws(() => multiplyByPolynomialBatch(s.rows.flat(), N, q, B, s.s), 'rows that are no Uint16Array');
}
if (!sets.some(s => s.N === 17 && s.q === 32)) throw new Error('the N = 17, q = 32 set is missing');
console.log(`shim_mulshared: ${sets.length} sets, ${rowsDone} rows`);
