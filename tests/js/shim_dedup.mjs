// Removing duplicates through the Node shim: ntru.dedupCiphertexts on every case of tests/golden/dedup_cases.json against the first and
// unique the fixture records, and the refusals of malformed arguments.  Composed in JavaScript: needs neither the addon nor a GPU.
//   node tests/js/shim_dedup.mjs
import { readFileSync } from 'fs';
import { dirname, join } from 'path';
import { fileURLToPath } from 'url';

import NTRU from '../../ntru-circom_amd/js/index.mjs';

const here = dirname(fileURLToPath(import.meta.url));
const same = (a, b, what) => {
  if (a.length !== b.length) throw new Error(what + ': lengths differ');
  for (let i = 0; i < a.length; i++) if (a[i] !== b[i]) throw new Error(what + ': differs at ' + i);
};
const throws = (fn, what) => { let t = false; try { fn(); } catch (err) { t = true; } if (!t) throw new Error(what + ' was not refused'); };

const { cases } = JSON.parse(readFileSync(join(here, '..', 'golden', 'dedup_cases.json'), 'utf8'));
let rows = 0;
for (const c of cases) {
  const ntru = new NTRU({ N: c.N, q: c.q });
  const B = c.rows.length, flat = Uint16Array.from(c.rows.flat());
  const prior = c.prior.length ? Uint16Array.from(c.prior.flat()) : null;
  const got = ntru.dedupCiphertexts(flat, B, { prior });
  same(got.first, c.first, `${c.name} first`);
  same(got.unique, c.unique, `${c.name} unique`);
  if (!prior) same(ntru.dedupCiphertexts(flat, B).first, c.first, `${c.name} without options`);
  same(ntru.dedupCiphertexts(new Uint16Array(0), 0, { prior }).unique, [], `${c.name} no rows`);
  throws(() => ntru.dedupCiphertexts(flat, B + 1), 'rows of the wrong size');
  throws(() => ntru.dedupCiphertexts(Array.from(flat), B), 'rows that are no Uint16Array');
  throws(() => ntru.dedupCiphertexts(flat, B, { prior: new Uint16Array(c.N + 1) }), 'a prior set that is no whole number of rows');
  rows += B;
}
console.log(`shim_dedup: ${cases.length} cases, ${rows} rows`);
