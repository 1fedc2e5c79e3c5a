// Scanning through the Node shim: ntru.scanBytes, which the shim composes from decryptBytes per key and a filter in JavaScript, on every
// case of tests/golden/scan_cases.json (the unmodified reference's results) -- counts, rows, bytes, truncation, the refusals -- and, when
// a file is named, on an engine-made batch whose expected result the Python side wrote (tests/test_scan_js_gpu.py).
//   node tests/js/shim_scan.mjs [expected.json]
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
  if (a.length !== b.length) throw new Error(`${what}: lengths differ (${a.length}, ${b.length})`);
  for (let i = 0; i < a.length; i++) if (a[i] !== b[i]) throw new Error(what + ': differs at ' + i);
};
const throws = (fn, needle, what) => {
  try { fn(); } catch (e) { if (String(e.message).includes(needle)) return; throw e; }
  throw new Error(what + ': did not throw');
};

const { cases } = JSON.parse(readFileSync(join(here, '..', 'golden', 'scan_cases.json'), 'utf8'));
let checked = 0;
for (const c of cases) {
  const { N } = c.options, W = c.W;
  const keys = c.keys.map(k => ({ f: unpack(k.f), fp: unpack(k.fp) }));
  const e = Uint16Array.from(unpack(c.e)), B = e.length / N;
  const hit = unpack(c.hit);
  const ntru = new NTRU({ ...c.options, f: keys[1].f, fp: keys[1].fp });
  const opts = { tag: Uint8Array.from(c.tag), tagOffset: c.tagOffset };
  const all = ntru.scanBytes(e, B, { keys, ...opts });
  if (all.length !== keys.length) throw new Error('one result per key');
  all.forEach((got, k) => {
    const want = c.hits[k];
    if (got.count !== want.length) throw new Error(`${c.set}: count of key ${k}: ${got.count}, recorded ${want.length}`);
    same(got.rows, want.map(h => h.row), `${c.set}: rows of key ${k}`);
    same(got.rows, hit.slice(k * B, (k + 1) * B).flatMap((x, b) => (x ? [b] : [])), `${c.set}: hit flags of key ${k}`);
    same(got.bytes, want.flatMap(h => h.bytes), `${c.set}: bytes of key ${k}`);
    checked++;
  });
  // the instance's own key is the default; pairs are accepted as well
  const own = ntru.scanBytes(e, B, opts);
  if (own.length !== 1 || own[0].count !== c.hits[1].length) throw new Error(`${c.set}: default key`);
  same(own[0].rows, all[1].rows, `${c.set}: default key rows`);
  same(ntru.scanBytes(e, B, { keys: keys.map(k => [k.f, k.fp]), ...opts })[2].rows, all[2].rows, `${c.set}: keys as pairs`);
  // truncation keeps the first hits and the whole count; 0 only counts
  const cut = ntru.scanBytes(e, B, { keys, ...opts, maxHits: 1 });
  cut.forEach((got, k) => {
    if (got.count !== all[k].count) throw new Error(`${c.set}: truncated count`);
    same(got.rows, all[k].rows.slice(0, 1), `${c.set}: truncated rows`);
    same(got.bytes, all[k].bytes.subarray(0, got.rows.length * W), `${c.set}: truncated bytes`);
  });
  ntru.scanBytes(e, B, { keys, ...opts, maxHits: 0 }).forEach((got, k) => {
    if (got.count !== all[k].count || got.rows.length || got.bytes.length) throw new Error(`${c.set}: count only`);
  });
  // no tag: the flags alone; a tag nobody carries: nothing
  ntru.scanBytes(e, B, { keys }).forEach((got, k) => { if (got.count < all[k].count) throw new Error(`${c.set}: no tag`); });
  const nobody = Uint8Array.from(c.tag, x => x ^ 0xff);
  ntru.scanBytes(e, B, { keys, tag: nobody, tagOffset: c.tagOffset }).forEach((got, k) => {
    if (got.count !== 0 && c.tag.length === 4) throw new Error(`${c.set}: a tag nobody carries`);          // (one byte may match by chance)
  });
  if (ntru.scanBytes(e.subarray(0, 0), 0, { keys, ...opts })[0].count !== 0) throw new Error('no blocks');
  throws(() => ntru.scanBytes(e, B, { keys, tag: new Uint8Array(33) }), '32 bytes', 'tag of 33 bytes');
  throws(() => ntru.scanBytes(e, B, { keys, tag: Uint8Array.from(c.tag), tagOffset: W }), 'does not lie inside', 'tag past the message');
  throws(() => ntru.scanBytes(e, B, { keys, maxHits: -1 }), 'maxHits', 'negative maxHits');
  throws(() => ntru.scanBytes(e, B, { keys: [] }), 'at least one key', 'no keys');
  // the centred lift: what decryptBytes throws
  const centred = new NTRU({ ...c.options, f: keys[0].f, fp: keys[0].fp, lift: 'centred' });
  throws(() => centred.scanBytes(e, B, opts), "decryptBytes: not available with the option lift: 'centred'", 'centred');
}

if (process.argv[2]) {
  const x = JSON.parse(readFileSync(process.argv[2], 'utf8'));
  const e = new Uint16Array(Uint8Array.from(Buffer.from(x.e, 'base64')).buffer);
  const ntru = new NTRU({ ...x.options });
  const got = ntru.scanBytes(e, x.B, { keys: x.keys, tag: Uint8Array.from(x.tag), tagOffset: x.tagOffset, maxHits: x.maxHits });
  x.want.forEach((want, k) => {
    if (got[k].count !== want.count) throw new Error(`batch: count of key ${k}: ${got[k].count}, expected ${want.count}`);
    same(got[k].rows, want.rows, `batch: rows of key ${k}`);
    same(got[k].bytes, Buffer.from(want.bytes, 'base64'), `batch: bytes of key ${k}`);
    checked++;
  });
}
console.log(`shim_scan: ${checked} key results of ${cases.length} cases${process.argv[2] ? ' and one batch' : ''}`);
