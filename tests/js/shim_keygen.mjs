// Batched key generation through the Node shim: ntru.generateKeysBatch (host arrays, sync and Async) and generateKeysBatchDev (device
// handles), the four per-item *Dev bindings against their host forms, handle checks, loadKeyFromBatch.  Writes the arrays to <out dir>
// as raw little-endian files plus keys.json; tests/test_keygen_js_gpu.py replays them on the CPU oracle.
//   node tests/js/shim_keygen.mjs <profile> <B> <out dir>
import { readFileSync, writeFileSync } from 'fs';
import { createRequire } from 'module';
import { dirname, join } from 'path';
import { fileURLToPath } from 'url';

import NTRU from '../../ntru-circom_amd/js/index.mjs';

const here = dirname(fileURLToPath(import.meta.url));
// the addon instance the shim uses (same file: the same module and engine), for the host forms the shim has no method for
const addon = createRequire(import.meta.url)('../../ntru-circom_amd/js/ntru_addon.node');
const [profile, Bs, outDir] = process.argv.slice(2);
const B = Number(Bs);
const opts = JSON.parse(readFileSync(join(here, '..', 'golden', `scheme_${profile}.json`), 'utf8')).options;
const ntru = new NTRU({ ...opts });
const { N, p, q } = ntru;
const key = Uint32Array.from([101, 202, 303, 404, 505, 606, 707, 808]);
const firstItem = 1000;
const dump = (name, a) => writeFileSync(join(outDir, name + '.bin'), Buffer.from(a.buffer, a.byteOffset, a.byteLength));
const same = (a, b, what) => {
  if (a.length !== b.length) throw new Error(what + ': lengths differ');
  for (let i = 0; i < a.length; i++) if (a[i] !== b[i]) throw new Error(what + ': differs at ' + i);
};

async function main() {
  // 1. host form, every array down, packed h too
  const keys = ntru.generateKeysBatch({ B, key, firstItem, maxTries: 100, pack: true });
  for (const n of ['f', 'g', 'fq', 'fp', 'h', 'tries', 'flags', 'packedH']) dump(n, keys[n]);
  // 2. the Async twin into page-locked arrays
  const outPin = { h: NTRU.allocUint16(B * N), flags: NTRU.allocUint8(B) };
  const lean = await ntru.generateKeysBatchAsync({ B, key, firstItem, want: { h: true }, out: outPin });
  if (lean.h !== outPin.h || lean.f !== undefined) throw new Error('async keygen: unexpected outputs');
  same(lean.h, keys.h, 'async h'); same(lean.flags, keys.flags, 'async flags');
  // 3. the device form
  const n = B * N;
  const dev = {
    workDev: NTRU.devAlloc(NTRU.keygenWorkspaceBytes(N, B)), fDev: NTRU.devAlloc(n), gDev: NTRU.devAlloc(n), fqDev: NTRU.devAlloc(2 * n),
    fpDev: NTRU.devAlloc(n), hDev: NTRU.devAlloc(2 * n), triesDev: NTRU.devAlloc(B), flagsDev: NTRU.devAlloc(B),
  };
  ntru.generateKeysBatchDev({ B, key, firstItem, maxTries: 100, ...dev });
  const down = (T, len, h) => NTRU.devDownload(new T(len), h);
  same(down(Int8Array, n, dev.fDev), keys.f, 'dev f'); same(down(Int8Array, n, dev.gDev), keys.g, 'dev g');
  same(down(Uint16Array, n, dev.fqDev), keys.fq, 'dev fq'); same(down(Uint8Array, n, dev.fpDev), keys.fp, 'dev fp');
  same(down(Uint16Array, n, dev.hDev), keys.h, 'dev h'); same(down(Uint8Array, B, dev.triesDev), keys.tries, 'dev tries');
  same(down(Uint8Array, B, dev.flagsDev), keys.flags, 'dev flags');

  // 4. the four per-item *Dev bindings against their host forms, on the generated keys
  const ok = [];
  for (let b = 0; b < B; b++) if (!keys.flags[b]) ok.push(b);
  const K = ok.length;
  const pick = (a, T) => { const o = new T(K * N); ok.forEach((b, k) => o.set(a.subarray(b * N, (b + 1) * N), k * N)); return o; };
  const f = pick(keys.f, Int8Array), g = pick(keys.g, Int8Array), fq = pick(keys.fq, Uint16Array), fp = pick(keys.fp, Uint8Array);
  const h = pick(keys.h, Uint16Array);
  const up = a => { const d = NTRU.devAlloc(a.byteLength); NTRU.devUpload(d, a); return d; };
  const [fD, gD, fqD, fpD, hD] = [f, g, fq, fp, h].map(up);
  const eng = { u16: () => NTRU.devAlloc(2 * K * N), u8: () => NTRU.devAlloc(K * N) };
  const vOut = [eng.u16(), eng.u16(), eng.u8(), eng.u8(), eng.u16(), eng.u16(), NTRU.devAlloc(K)];
  ntru.verifyKeysBatchDev(fD, gD, fqD, fpD, hD, K, ...vOut);
  const vTypes = [Uint16Array, Uint16Array, Uint8Array, Uint8Array, Uint16Array, Uint16Array];
  const vHost = vTypes.map(T => new T(K * N)), vFlags = new Uint8Array(K);
  addon.verifyKeysBatch(N, q, p, f, g, fq, fp, h, K, ...vHost, vFlags);
  vHost.forEach((a, i) => same(down(vTypes[i], K * N, vOut[i]), a, 'verifyKeysBatchDev ' + i));
  same(down(Uint8Array, K, vOut[6]), vFlags, 'verifyKeysBatchDev flags');
  const iq = eng.u16(), ip = eng.u8(), ifl = NTRU.devAlloc(K);
  ntru.invertKeyBatchDev(fD, K, iq, ip, ifl);
  const iqH = new Uint16Array(K * N), ipH = new Uint8Array(K * N), iflH = new Uint8Array(K);
  addon.invertKeyBatch(N, q, p, f, K, iqH, ipH, iflH);
  same(down(Uint16Array, K * N, iq), iqH, 'invertKeyBatchDev fq'); same(iqH, fq, 'invertKeyBatch fq');
  same(down(Uint8Array, K * N, ip), ipH, 'invertKeyBatchDev fp'); same(down(Uint8Array, K, ifl), iflH, 'invertKeyBatchDev flags');
  const ph = eng.u16();
  ntru.publicKeyBatchDev(fqD, gD, K, ph);
  same(down(Uint16Array, K * N, ph), h, 'publicKeyBatchDev');
  const a16 = Uint16Array.from(fq), b16 = Uint16Array.from(h), pq = eng.u16(), pr = eng.u16();
  NTRU.polymulSplitDev(N, q, up(a16), up(b16), K, pq, pr);
  const pqH = new Uint16Array(K * N), prH = new Uint16Array(K * N);
  addon.polymulSplit(N, q, a16, b16, K, pqH, prH);
  same(down(Uint16Array, K * N, pq), pqH, 'polymulSplitDev quot'); same(down(Uint16Array, K * N, pr), prH, 'polymulSplitDev rem');

  // 5. an undersized or freed handle is refused before anything is launched
  const refused = (what, fn) => {
    try { fn(); } catch (e) { if (/bad argument/.test(e.message)) return; throw e; }
    throw new Error(what + ': accepted');
  };
  const small = NTRU.devAlloc(K * N - 1);
  refused('undersized h', () => ntru.publicKeyBatchDev(fqD, gD, K, small));
  refused('undersized f', () => ntru.invertKeyBatchDev(small, K + 1, iq, ip, ifl));
  refused('undersized quot', () => NTRU.polymulSplitDev(N, q, fqD, hD, K, small, pr));
  refused('undersized workspace', () => ntru.generateKeysBatchDev({ B, key, ...dev, workDev: small }));
  const freed = NTRU.devAlloc(2 * K * N);
  NTRU.devFree(freed);
  refused('freed rem_h', () => ntru.verifyKeysBatchDev(fD, gD, fqD, fpD, hD, K, vOut[0], vOut[1], vOut[2], vOut[3], vOut[4], freed, vOut[6]));
  refused('freed flags', () => ntru.generateKeysBatchDev({ B, key, ...dev, flagsDev: freed }));

  // 6. loadKeyFromBatch: verifyKeysInputs of the first three good items; a failed item throws the reference's error
  const inputs = ok.slice(0, 3).map(b => ({ item: b, witnesses: new NTRU({ ...opts }).loadKeyFromBatch(keys, b).verifyKeysInputs() }));
  const bad = { ...keys, flags: Uint8Array.from(keys.flags) };
  bad.flags[0] = 8;
  try { ntru.loadKeyFromBatch(bad, 0); throw new Error('loadKeyFromBatch accepted a failed item'); } catch (e) {
    if (e.message !== 'Could not find invertible f') throw e;
  }
  writeFileSync(join(outDir, 'keys.json'), JSON.stringify({ N, q, p, B, firstItem, key: Array.from(key), inputs,
                                                            outputSize: keys.outputSize }));
  console.log(`shim_keygen: ${B} key pairs through host, Async and Dev forms; ${K} checked through the four *Dev bindings`);
}

main().catch(e => { console.error(e); process.exit(1); });
