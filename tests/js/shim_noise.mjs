// The decryption noise of ciphertexts through the Node shim: ntru.noiseBatch on every sum of tests/golden/noise_cases.json against the
// reduction of the reference's own remainder1, against A = p sum(r * g) + f * sum(m) over the integers for the sums whose A lies in
// (-q/2, q/2], under both lift options, and the refusals of malformed arguments.
//   node tests/js/shim_noise.mjs
import { readFileSync } from 'fs';
import { dirname, join } from 'path';
import { fileURLToPath } from 'url';

import NTRU from '../../ntru-circom_amd/js/index.mjs';

const here = dirname(fileURLToPath(import.meta.url));
const same = (a, b, what) => {
  if (a.length !== b.length) throw new Error(what + ': lengths differ');
  for (let i = 0; i < a.length; i++) if (a[i] !== b[i]) throw new Error(what + ': differs at ' + i);
};
// { bits, n, off, b64 } of tests/golden/gen_noise_cases.mjs -> Array of integers
function unpack(a) {
  const bytes = Buffer.from(a.b64, 'base64');
  return Array.from({ length: a.n }, (_, i) => {
    let x = 0;
    for (let b = 0; b < a.bits; b++) { const at = i * a.bits + b; if ((bytes[at >> 3] >> (at & 7)) & 1) x |= 1 << b; }
    return x + a.off;
  });
}
const throws = (fn, what) => { let t = false; try { fn(); } catch (err) { t = true; } if (!t) throw new Error(what + ' was not refused'); };

const { sets } = JSON.parse(readFileSync(join(here, '..', 'golden', 'noise_cases.json'), 'utf8'));
let rows = 0, inside = 0, outside = 0;
for (const s of sets) {
  const { N, q } = s.options, B = s.cases.length;
  const flat = Uint16Array.from(s.cases.map(c => unpack(c.e)).flat());
  const peak = [], energy = [];
  for (const c of s.cases) {
    const cen = unpack(c.remainder1).map(a => (a > q / 2 ? a - q : a));
    peak.push(Math.max(...cen.map(Math.abs)));
    energy.push(cen.reduce((t, x) => t + x * x, 0));
    if (c.inside) {
      const A = unpack(c.A);
      if (Math.max(...A.map(Math.abs)) !== peak[peak.length - 1] || A.reduce((t, x) => t + x * x, 0) !== energy[energy.length - 1])
        throw new Error(`${s.set} K=${c.K}: the centred remainder1 is not A`);
      inside++;
    } else outside++;
    rows++;
  }
  for (const lift of ['reference', 'centred']) {
    const ntru = new NTRU({ ...s.options, lift });
    ntru.loadPrivateKeyF(unpack(s.key.f));
    const got = ntru.noiseBatch(flat, B);
    same(Array.from(got.peak), peak, `${s.set} peak (${lift})`);
    same(got.energy, energy, `${s.set} energy (${lift})`);
    same(Array.from(got.margin), peak.map(x => q / 2 - x), `${s.set} margin (${lift})`);
    same(Array.from(ntru.noiseBatch(new Uint16Array(0), 0).peak), [], `${s.set} no rows`);
    throws(() => ntru.noiseBatch(flat, B + 1), 'rows of the wrong size');
    throws(() => ntru.noiseBatch(Array.from(flat), B), 'rows that are no Uint16Array');
  }
}
if (inside < 8 || outside < 2) throw new Error(`the fixture needs both sides: ${inside} inside, ${outside} outside`);
console.log(`shim_noise: ${sets.length} sets, ${rows} rows`);
