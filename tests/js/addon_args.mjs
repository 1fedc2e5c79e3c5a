// What ntru_addon.node accepts and refuses, export by export, before any engine exists: names, argument counts, scalar ranges,
// TypedArray types and lengths, null where it is allowed, and the order "validate first, then ask for the engine".
// create() is never called, so this needs no GPU: a valid call ends in "ntru engine not created".  Without an engine there are no
// handles either, so a *Dev export can only be shown to refuse what is not a handle; the GPU tests of the shim use real ones.
import { createRequire } from 'module';
const addon = createRequire(import.meta.url)('../../ntru-circom_amd/js/ntru_addon.node');

const N = 5, B = 3, G = 1, K = 3, Q = 32, P = 3;
const WIDTH = new Map([[Int8Array, 1], [Uint8Array, 1], [Uint16Array, 2], [Uint32Array, 4], [BigInt64Array, 8], [BigUint64Array, 8],
  [Float64Array, 8]]);
const packedLen = (maxVal) => B * addon.packParams(maxVal, N)[3] * 4;
if (packedLen(P - 1) !== packedLen(Q - 1)) throw new Error('pick N so that both packed sizes of pipelineBatch agree');

// ---- argument kinds.  min: the smallest value the addon accepts for that scalar.
const int = (v, min) => ({ kind: 'int', v, min });
const nN = int(N, 1), nB = int(B, 0), nG = int(G, 0), nK = int(K), q = int(Q), p = int(P), any = int(2);
const first = { kind: 'first', v: 7 };
const num = (v) => ({ kind: 'num', v });                                  // a byte count, taken as a double
const flag = { kind: 'flag', v: false };
const buf = (T, len, opt) => ({ kind: 'buf', T, len, opt: !!opt });        // len null: any length is valid
const opt = (T, len) => buf(T, len, true);
const anyArray = { kind: 'buf', T: Uint16Array, len: null, opt: false, anyType: true };   // devUpload / devDownload take every element type
const i8 = Int8Array, u8 = Uint8Array, u16 = Uint16Array, u32 = Uint32Array, i64 = BigInt64Array, u64 = BigUint64Array, f64 = Float64Array;
const n = N * B, n1 = (N + 1) * B, gn = G * N;
// The *Dev twin of a host list: every buffer becomes a handle of the same bytes, except those named in `host`.
const dev = (args, host = []) => args.map((a, i) => (a.kind === 'buf' && !host.includes(i) ?
  { kind: 'handle', bytes: a.len * WIDTH.get(a.T), opt: a.opt } : a));
const handle = (bytes, opt) => ({ kind: 'handle', bytes, opt: !!opt });
const key = buf(u32, 8);

const polymul = [nN, q, buf(u16, n), buf(u16, n), nB, buf(u16, n), buf(u16, n)];
const invert = [nN, q, p, buf(i8, n), nB, opt(u16, n), opt(u8, n), buf(u8, B)];
const pubkey = [nN, q, p, buf(u16, n), buf(i8, n), nB, buf(u16, n)];
const encrypt = [nN, q, buf(u16, N), buf(u8, n), buf(u8, n), nB, buf(u16, n), opt(u16, n)];
const decrypt = [nN, q, p, buf(i8, N), buf(u8, N), buf(u16, n), nB, buf(u8, n), opt(u16, n), opt(u16, n), opt(u8, n)];
const encryptPer = [nN, q, buf(u16, n), buf(u8, n), buf(u8, n), nB, buf(u16, n), opt(u16, n)];
const decryptPer = [nN, q, p, buf(i8, n), buf(u8, n), buf(u16, n), nB, buf(u8, n), opt(u16, n), opt(u16, n), opt(u8, n)];
const verify = [nN, q, p, buf(i8, n), buf(i8, n), buf(u16, n), buf(u8, n), buf(u16, n), nB, buf(u16, n), buf(u16, n), buf(u8, n), buf(u8, n),
  buf(u16, n), buf(u16, n), buf(u8, B)];
const sample = [nN, any, any, any, key, first, nB, buf(u8, n)];
const sum = [nN, q, buf(u16, n), opt(u16, B), opt(i64, G + 1), nK, nG, nB, buf(u16, gn)];
const tally = [nN, q, p, buf(i8, N), buf(u8, N), buf(u16, n), opt(u16, B), opt(i64, G + 1), nK, nG, nB, buf(u16, gn), buf(u8, gn),
  opt(u16, gn), opt(u16, gn), opt(u8, gn)];
const pipeline = [nN, q, p, buf(u16, N), opt(i8, N), opt(u8, N), opt(u32, 8), first, any, any, opt(u8, n), buf(u8, n), nB, opt(u8, n),
  opt(u16, n), opt(u8, n), opt(u64, packedLen(Q - 1))];
const keygen = [nN, q, p, any, any, key, first, any, nB, opt(i8, n), opt(i8, n), opt(u16, n), opt(u8, n), opt(u16, n), opt(u8, B), buf(u8, B),
  opt(u64, packedLen(Q - 1))];
const keygenDev = [nN, q, p, any, any, key, first, any, nB, handle(addon.keygenWorkspaceBytes(N, B)), handle(n), handle(n), handle(2 * n),
  handle(n), handle(2 * n), handle(B, true), handle(B)];
const bits31 = addon.packParams(31, 0)[0], packedSize = 2, per = 2;

// expect: what the valid list gives.  'noengine' (the default) is the "ntru engine not created" Error; a function checks a return value;
// null means the valid list is never sent (create would make an engine).
const isNum = (v) => typeof v === 'number';
const table = {
  deviceCount: { args: [], expect: isNum },
  create: { args: [int(0)], expect: null },
  destroy: { args: [], expect: (v) => v === undefined },
  useDevices: { args: [buf(Int32Array, null)], expect: (v) => v === 0, make: () => new Int32Array(0) },
  supports: { args: [int(N), q], expect: (v) => typeof v === 'boolean' },
  setSamplerRounds: { args: [int(0)] },
  packParams: { args: [int(31), int(N)], expect: (v) => Array.isArray(v) && v.length === 4 && v.every(isNum) },
  genericCapacity: { args: [int(3), int(3)], expect: isNum },
  genericOp: { args: [int(0), buf(f64, null), buf(f64, null), num(7), buf(f64, addon.genericCapacity(3, 3)), opt(f64, addon.genericCapacity(3, 3))],
    make: () => new Float64Array(3) },
  allocPinned: { args: [num(64)] },
  devAlloc: { args: [num(64)] },
  devFree: { args: [handle(1)] },
  devUpload: { args: [handle(16), anyArray], make: () => new Uint16Array(8) },
  devDownload: { args: [anyArray, handle(16)], make: () => new Uint16Array(8) },
  keygenWorkspaceBytes: { args: [int(N), nB], expect: (v) => isNum(v) && v > 0 },
  packBatch: { args: [int(31), int(N), buf(u16, N * B), nB, buf(u64, packedLen(31))] },
  unpackBatch: { args: [int(31), int(per * bits31), buf(u64, packedSize * 4 * B), int(packedSize, 0), nB, buf(u16, packedSize * per * B)] },
  packBatchDev: { args: [int(31), int(N, 0), handle(2 * N * B), nB, handle(packedLen(31) * 8), flag] },
  polymulSplit: { args: polymul }, polymulSplitDev: { args: dev(polymul) },
  splitByI: { args: [nN, q, buf(u16, 2 * n), nB, buf(u16, n), buf(u16, n)] },
  addBatch: { args: [nN, q, buf(u16, n), buf(u16, n), nB, buf(u16, n)] },
  invertKeyBatch: { args: invert }, invertKeyBatchDev: { args: dev(invert) },
  publicKeyBatch: { args: pubkey }, publicKeyBatchDev: { args: dev(pubkey) },
  encryptBatch: { args: encrypt }, encryptBatchDev: { args: dev(encrypt) }, encryptBatchAsync: { args: encrypt },
  decryptBatch: { args: decrypt }, decryptBatchDev: { args: dev(decrypt) }, decryptBatchAsync: { args: decrypt },
  encryptPeritemBatch: { args: encryptPer }, encryptPeritemBatchDev: { args: dev(encryptPer) },
  decryptPeritemBatch: { args: decryptPer }, decryptPeritemBatchDev: { args: dev(decryptPer) },
  verifyKeysBatch: { args: verify }, verifyKeysBatchDev: { args: dev(verify) },
  checkEncryptBatch: { args: [nN, q, any, buf(u16, n), buf(u16, n), buf(u16, n), buf(u16, n1), buf(u16, n1), nB, buf(u8, B)] },
  checkDecryptBatch: { args: [nN, q, any, p, any, buf(u16, n), buf(u16, n), buf(u16, n), buf(u16, n1), buf(u16, n1), buf(u16, n1), buf(u16, n1), nB,
    buf(u8, B)] },
  checkInverseBatch: { args: [nN, q, any, buf(u16, n), buf(u16, n), buf(u16, n1), buf(u16, n1), nB, buf(u8, B)] },
  sampleTernary: { args: sample }, sampleTernaryDev: { args: dev(sample, [4]) },
  sumGroups: { args: sum, groups: [4, 5, 6] }, sumGroupsDev: { args: dev(sum), groups: [4, 5, 6] },
  tallyDecryptBatch: { args: tally, groups: [7, 8, 9] }, tallyDecryptBatchDev: { args: dev(tally), groups: [7, 8, 9] },
  tallyDecryptBatchAsync: { args: tally, groups: [7, 8, 9] },
  pipelineBatch: { args: pipeline }, pipelineBatchAsync: { args: pipeline },
  keygenBatch: { args: keygen }, keygenBatchAsync: { args: keygen }, keygenBatchDev: { args: keygenDev },
};

const EXPORTS = ['addBatch', 'allocPinned', 'checkDecryptBatch', 'checkEncryptBatch', 'checkInverseBatch', 'create', 'decryptBatch',
  'decryptBatchAsync', 'decryptBatchDev', 'decryptPeritemBatch', 'decryptPeritemBatchDev', 'destroy', 'devAlloc', 'devDownload', 'devFree',
  'devUpload', 'deviceCount', 'encryptBatch', 'encryptBatchAsync', 'encryptBatchDev', 'encryptPeritemBatch', 'encryptPeritemBatchDev',
  'genericCapacity', 'genericOp', 'invertKeyBatch', 'invertKeyBatchDev', 'keygenBatch', 'keygenBatchAsync', 'keygenBatchDev',
  'keygenWorkspaceBytes', 'packBatch', 'packBatchDev', 'packParams', 'pipelineBatch', 'pipelineBatchAsync', 'polymulSplit', 'polymulSplitDev',
  'publicKeyBatch', 'publicKeyBatchDev', 'sampleTernary', 'sampleTernaryDev', 'setSamplerRounds', 'splitByI', 'sumGroups', 'sumGroupsDev',
  'supports', 'tallyDecryptBatch', 'tallyDecryptBatchAsync', 'tallyDecryptBatchDev', 'unpackBatch', 'useDevices', 'verifyKeysBatch',
  'verifyKeysBatchDev'];

let checks = 0;
const same = (a, b) => a.length === b.length && a.every((v, i) => v === b[i]);
const names = Object.getOwnPropertyNames(addon).sort();      // the addon defines them non-enumerable: Object.keys(addon) is empty
if (!same(names, EXPORTS)) throw new Error('export names differ: ' + names.join(' '));
if (!same(Object.keys(table).sort(), EXPORTS)) throw new Error('the table does not cover every export');

function outcome(name, list) {
  try { return { value: addon[name](...list) }; } catch (e) { return { error: e }; }
}
function expectThrow(name, list, ctor, re, what) {
  const r = outcome(name, list);
  checks++;
  if (!r.error || r.error.constructor !== ctor || !re.test(r.error.message))
    throw new Error(`${name}: ${what}: expected ${ctor.name} ${re}, got ${r.error ? r.error.constructor.name + ': ' + r.error.message : 'a return value'}`);
}
const tooFew = (name, list, what) => expectThrow(name, list, TypeError, /^too few arguments$/, what);
const badArgs = (name, list, what) => expectThrow(name, list, TypeError, /^bad argument types \/ sizes$/, what);
const noEngine = (name, list, what) => expectThrow(name, list, Error, /^ntru engine not created: /, what);

function valid(row) {
  return row.args.map((a) => {
    if (a.kind === 'buf') return a.len === null ? row.make() : new a.T(a.len);
    if (a.kind === 'handle') return null;
    return a.v;
  });
}
const wrongType = (T) => (T === Uint16Array ? Uint8Array : Uint16Array);
const replaced = (list, i, v) => list.map((x, j) => (j === i ? v : x));

for (const name of EXPORTS) {
  const row = table[name], args = row.args, ok = valid(row);
  const handlesMissing = args.some((a) => a.kind === 'handle' && !a.opt);
  // what the list gives when nothing in it is refused
  const passes = (list, what) => {
    if (handlesMissing) return badArgs(name, list, what + ' (a required handle is null)');
    if (row.expect === undefined) return noEngine(name, list, what);
    if (row.expect === null) return undefined;
    const r = outcome(name, list);
    checks++;
    if (r.error || !row.expect(r.value)) throw new Error(`${name}: ${what}: unexpected ${r.error ? r.error.message : String(r.value)}`);
    return undefined;
  };
  if (args.length) tooFew(name, ok.slice(0, -1), '(a) one argument fewer');
  passes(ok, '(g) the valid list');
  args.forEach((a, i) => {
    const tag = `argument ${i}`;
    if (a.kind === 'int' || a.kind === 'first' || a.kind === 'num') badArgs(name, replaced(ok, i, 'x'), `${tag} as a string`);
    if (a.kind === 'int' && a.min !== undefined) badArgs(name, replaced(ok, i, a.min - 1), `${tag} below its minimum`);
    if (a.kind === 'first') {
      badArgs(name, replaced(ok, i, -1), `(i) ${tag} negative`);
      badArgs(name, replaced(ok, i, 2 ** 53), `(i) ${tag} above 2^53 - 1`);
      passes(replaced(ok, i, 2 ** 53 - 1), `(i) ${tag} = 2^53 - 1`);
    }
    if (a.kind === 'flag') badArgs(name, replaced(ok, i, 1), `${tag} not a boolean`);
    if (a.kind === 'buf') {
      if (a.len !== null && a.len > 0 && !a.opt) badArgs(name, replaced(ok, i, new a.T(a.len - 1)), `(b) ${tag} one element short`);
      if (a.len !== null && a.len > 0 && a.opt && !handlesMissing) badArgs(name, replaced(ok, i, new a.T(a.len - 1)), `(b) optional ${tag} one element short`);
      if (a.len !== null) passes(replaced(ok, i, new a.T(a.len + 1)), `${tag} one element longer`);
      const wrong = new (wrongType(a.T))(a.len === null ? 8 : a.len * 8);
      if (!a.anyType && (!a.opt || !handlesMissing)) badArgs(name, replaced(ok, i, wrong), `(c) ${tag} of the wrong element type`);
      if (!a.opt || !handlesMissing) badArgs(name, replaced(ok, i, [1, 2, 3]), `${tag} a plain array`);
    }
    if (a.kind === 'buf' || a.kind === 'handle') {
      if (!a.opt) {
        badArgs(name, replaced(ok, i, null), `(d) ${tag} null`);
        badArgs(name, replaced(ok, i, undefined), `(d) ${tag} undefined`);
      } else {
        passes(replaced(ok, i, null), `(e) optional ${tag} null`);
        passes(replaced(ok, i, undefined), `(f) optional ${tag} undefined`);
      }
    }
    if (a.kind === 'handle') {
      badArgs(name, replaced(ok, i, 1234), `(h) ${tag} a number`);
      badArgs(name, replaced(ok, i, {}), `(h) ${tag} a plain object`);
      badArgs(name, replaced(ok, i, new Uint8Array(a.bytes)), `(h) ${tag} a TypedArray`);
    }
  });
  if (row.groups) {
    const [iOff, iK, iG] = row.groups, isDev = args[iOff].kind === 'handle';
    const noOff = replaced(ok, iOff, null);
    passes(noOff, '(k) uniform K with G * K == B');
    badArgs(name, replaced(noOff, iK, K - 1), '(k) uniform K with G * K != B');
    badArgs(name, replaced(noOff, iK, 0), '(k) uniform K = 0');
    badArgs(name, replaced(replaced(noOff, iK, 1), iG, B + 1), '(k) uniform K with G > B');
    if (!isDev) {
      const off = (...v) => replaced(ok, iOff, BigInt64Array.from(v.map(BigInt)));
      passes(off(0, B), '(j) offsets 0 .. B');
      passes(off(1, 1), '(j) an empty group');
      badArgs(name, off(2, 1), '(j) offsets that decrease');
      badArgs(name, off(0, B + 1), '(j) offsets that end beyond B');
      badArgs(name, off(-1, B), '(j) a negative first offset');
    }
  }
}
console.log(`addon_args: ${EXPORTS.length} exports, ${checks} checks OK`);
