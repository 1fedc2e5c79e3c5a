// Re-randomising and shuffling through the Node shim: ntru.reencryptBatch, which the shim composes from encryptBatch (zero message) and
// addBatch, on every round of every case of tests/golden/mix_cases.json (the unmodified reference's results), plus the decrypt of the
// outputs and the method's refusals.
//   node tests/js/shim_mix.mjs
import { readFileSync } from 'fs';
import { dirname, join } from 'path';
import { fileURLToPath } from 'url';

import NTRU from '../../ntru-circom_amd/js/index.mjs';

const here = dirname(fileURLToPath(import.meta.url));
const unpack = ({ bits, n, off, b64 }) => {
  const bytes = Buffer.from(b64, 'base64');
  const out = new Array(n);
  for (let i = 0; i < n; i++) {
    let v = 0;
    for (let b = 0; b < bits; b++) { const at = i * bits + b; if ((bytes[at >> 3] >> (at & 7)) & 1) v += 2 ** b; }
    out[i] = v + off;
  }
  return out;
};
const same = (a, b, what) => {
  if (a.length !== b.length) throw new Error(what + ': lengths differ');
  for (let i = 0; i < a.length; i++) if (a[i] !== b[i]) throw new Error(what + ': differs at ' + i);
};
const throws = (fn, what) => { try { fn(); } catch (e) { if (e instanceof RangeError) return; throw e; } throw new Error(what + ': no RangeError'); };

const { cases } = JSON.parse(readFileSync(join(here, '..', 'golden', 'mix_cases.json'), 'utf8'));
let rounds = 0;
for (const c of cases) {
  const { N, q, p } = c.options;
  const ntru = new NTRU({ ...c.options, h: unpack(c.key.h), f: unpack(c.key.f), fp: unpack(c.key.fp) });
  let cur = Uint16Array.from(unpack(c.e));
  for (const rd of c.rounds) {
    const B = rd.src.length, r = Uint8Array.from(unpack(rd.r));
    const got = ntru.reencryptBatch(cur, r, B, rd.src);
    same(got.e, unpack(rd.remainder), `${c.set}: remainder`);
    same(got.quotientE, unpack(rd.quotient), `${c.set}: quotient`);
    for (let i = 0; i < B; i++) same(got.m.subarray(i * N, (i + 1) * N), cur.subarray(rd.src[i] * N, (rd.src[i] + 1) * N), `${c.set}: m`);
    const lean = ntru.reencryptBatch(cur, r, B, BigInt64Array.from(rd.src, x => BigInt(x)), false);
    if (lean.quotientE !== null) throw new Error('value-only call returned the quotient');
    same(lean.e, got.e, `${c.set}: value-only`);
    same(ntru.decryptBatch(got.e, B, false).value, unpack(rd.value), `${c.set}: decrypt`);
    cur = got.e;
    rounds++;
  }
  // src == null: row i; values >= q are reduced
  const B = 4, r = Uint8Array.from(unpack(c.rounds[2].r).slice(0, B * N));
  const wide = cur.map(x => x + (q <= 32768 ? q : 0));
  same(ntru.reencryptBatch(wide, r, B).e, ntru.reencryptBatch(cur, r, B, [0, 1, 2, 3]).e, `${c.set}: identity`);
  throws(() => ntru.reencryptBatch(cur, r, B, [0, 1, 2, cur.length / N]), 'index past the rows');
  throws(() => ntru.reencryptBatch(cur, r, B, [0, -1, 2, 3]), 'negative index');
  throws(() => ntru.reencryptBatch(cur.subarray(0, 2 * N), r, B), 'B > Bin without src');
}
console.log(`shim_mix: ${rounds} rounds of ${cases.length} cases`);
