// Golden cases for the product of a batch with one shared polynomial: runs the UNMODIFIED reference under Node and records, for seeded
// rows and one polynomial s per set, multiplyPolynomials(row, s, q) (index.js:319-355) followed by dividePolynomials(., I, q)
// (index.js:358-401) with I = 1 - x^N, as the reference's own (trimmed) quotient and remainder per row.  s carries the values at which
// the digits of k_mul_shared_m change (0, 63, 64, 65, 127, 128, q - 64, q - 1, reduced modulo q) and one row holds q - 1 everywhere.
// Only the resulting JSON is committed; tests/mulshared_ref.py and tests/js/shim_mulshared.mjs read it.
//
//   node tests/golden/gen_mulshared_cases.mjs <checkout of the reference> [outdir]
import { writeFileSync } from 'fs';
import { dirname, join } from 'path';
import { fileURLToPath, pathToFileURL } from 'url';

const here = dirname(fileURLToPath(import.meta.url));
const refDir = process.argv[2];
if (!refDir) { console.error('usage: node gen_mulshared_cases.mjs <checkout of the reference> [outdir]'); process.exit(2); }
const outDir = process.argv[3] || here;
let state = 0x5eed1;
function nextU32() { let x = state; x ^= x << 13; x >>>= 0; x ^= x >>> 17; x ^= x << 5; x >>>= 0; state = x; return x; }

async function main() {
const { multiplyPolynomials, dividePolynomials } = await import(pathToFileURL(join(refDir, 'index.js')).href);
const out = [];
for (const [N, q, B] of [[17, 32, 3], [33, 4096, 3], [65, 8192, 2], [31, 128, 2]]) {
  const I = new Array(N + 1).fill(0);
  I[0] = 1; I[N] = -1;
  const s = Array.from({ length: N }, () => nextU32() % q);
  [0, 63, 64, 65, 127, 128, q - 64, q - 1].forEach((v, i) => { s[i + 1] = ((v % q) + q) % q; });
  s[N - 1] = 1 + nextU32() % (q - 1);                        // a leading coefficient the reference does not trim
  const rows = Array.from({ length: B }, (_, b) => Array.from({ length: N }, () => (b === 1 ? q - 1 : nextU32() % q)));
  const cases = rows.map(row => {
    const { quotient, remainder } = dividePolynomials(multiplyPolynomials(row, s, q), I, q);
    return { quotient, remainder };
  });
  out.push({ N, q, s, rows, cases });
}
writeFileSync(join(outDir, 'mulshared_cases.json'),
  `{"generator":"gen_mulshared_cases.mjs","sets":[\n${out.map(c => JSON.stringify(c)).join(',\n')}\n]}\n`);
console.log('mulshared_cases.json:', out.map(s => `N=${s.N} q=${s.q} B=${s.rows.length}`).join(' | '));
}
main().catch(e => { console.error(e); process.exit(1); });
