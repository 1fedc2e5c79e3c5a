"""Host-side mirror of the reference's hot-path interface (numtel/ntru-circom index.js) over the HIP engine.

Same names, argument meaning, return shapes and error behaviour as the reference for:
  class NTRU                 index.js:7-207   (constructor options, public fields, encryptBits, decryptBits,
                                               verifyKeysInputs, encryptStr, decryptStr, calculateNq/Np)
  multiplyPolynomials        index.js:319-355
  addPolynomials             index.js:235-244 (O(N) host glue, as in the reference)
  degree / trimPolynomial / expandArray / generateCustomArray / stringToBits / bitsToString

All polynomial products and the quotient/remainder split run on the GPU through the C ABI
(include/ntru_engine.h); this file only reshapes data (padding, trimming, dict building), which is what
SURVEY.md section 8 assigns to the shim.  Key generation (index.js:30-79) runs on the device as well; polyInv,
extendedEuclideanAlgorithm, dividePolynomials by an arbitrary divisor and products modulo more than 65536 run on the
engine's generic family (ntru_generic_*), which follows the reference step by step, non-units included.
"""
import contextlib
import secrets

import numpy as np

from . import combine as combine_calls
from . import dedup as dedup_calls
from . import lift as lift_calls
from . import audit as audit_calls
from . import mix as mix_calls
from . import packed as packed_calls
from . import scan as scan_calls
from . import count as count_calls
from . import noise as noise_calls
from . import shared_product as shared_calls
from .engine import (FLAG_INVALID_FP, FLAG_INVALID_FQ, FLAG_INVALID_H, FLAG_NOT_UNIT_MOD2, FLAG_NOT_UNIT_MODP,
                     GENERIC_ERRORS, Engine, EngineError)

_DEFAULT_ENGINE = None


def default_engine():
    """Engine on HIP device 0, created on first use.  Raises EngineError when no GPU / library is present."""
    global _DEFAULT_ENGINE
    if _DEFAULT_ENGINE is None:
        _DEFAULT_ENGINE = Engine(0)
    return _DEFAULT_ENGINE


# ---- small helpers with the reference's semantics --------------------------------------------------------

def degree(poly):
    """index.js:210-215"""
    for i in range(len(poly) - 1, -1, -1):
        if poly[i] != 0:
            return i
    return -1


def trimPolynomial(poly):
    """index.js:218-221"""
    d = degree(poly)
    return list(poly[:d + 1]) if d >= 0 else [0]


def expandArray(arr, length, fill=0):
    """index.js:534-536; the reference's `Array(len - arr.length)` throws RangeError when arr is too long."""
    if len(arr) > length:
        raise ValueError("Invalid array length")
    return list(arr) + [fill] * (length - len(arr))


def addPolynomials(a, b, p):
    """index.js:235-244"""
    n = max(len(a), len(b))
    out = [((a[i] if i < len(a) else 0) + (b[i] if i < len(b) else 0)) % p for i in range(n)]
    return trimPolynomial(out)


def generateCustomArray(length, numOnes, numNegOnes, rand_u32=None):
    """index.js:461-488: numOnes 1s, numNegOnes -1s, rest 0, Fisher-Yates with i descending and
    j = u32 % (i+1), exactly length-1 draws.  `rand_u32` (callable -> uint32) defaults to the OS CSPRNG."""
    if numOnes + numNegOnes > length:
        raise ValueError("The total of 1s and -1s cannot exceed the array length.")
    rand_u32 = rand_u32 or (lambda: secrets.randbits(32))
    arr = [1] * numOnes + [-1] * numNegOnes + [0] * (length - numOnes - numNegOnes)
    for i in range(length - 1, 0, -1):
        j = rand_u32() % (i + 1)
        arr[i], arr[j] = arr[j], arr[i]
    return arr


def stringToBits(s):
    """index.js:538-546"""
    return [int(c) for ch in s for c in format(ord(ch), "08b")]


def bitsToString(bits):
    """index.js:548-556.  JS parseInt(str, 2) reads the longest leading run of binary digits and gives NaN when
    there is none; String.fromCharCode(NaN) is '\\u0000' -- wrong-key decryptions (ternary garbage) rely on that."""
    out = []
    for i in range(0, len(bits), 8):
        digits = "".join(str(b) for b in bits[i:i + 8])
        k = 0
        while k < len(digits) and digits[k] in "01":
            k += 1
        out.append(chr(int(digits[:k], 2) & 0xFFFF if k else 0))
    return "".join(out)


class ReferenceError_(ValueError):
    """An error the reference itself throws (`throw new Error(msg)`): str(e) is the reference's message."""


def _js_mod(x, p):
    """JS `%`: truncated remainder, sign of the dividend."""
    return int(np.fmod(x, p))


def _fast_modulus(N, p):
    return p >= 2 and (p <= 65536 if p & (p - 1) == 0 else N * (p - 1) * (p - 1) < 65536)


def _is_I(b, p):
    N = len(b) - 1
    return N >= 1 and b[0] % p == 1 and b[N] % p == p - 1 and all(x % p == 0 for x in b[1:N])


def _raise_status(st):
    if st:
        raise ReferenceError_(GENERIC_ERRORS[int(st)])


def modInverse(a, p):
    """index.js:224-232 (brute force, like the reference; None when there is no inverse)"""
    a = ((_js_mod(a, p)) + p) % p
    for x in range(1, p):
        if (a * x) % p == 1:
            return x
    return None


def subtractPolynomials(a, b, p):
    """index.js:247-256"""
    n = max(len(a), len(b))
    return trimPolynomial([((a[i] if i < len(a) else 0) - (b[i] if i < len(b) else 0)) % p for i in range(n)])


def multiplyPolynomialsByScalar(poly, scalar, p):
    """index.js:404-406: no normalisation (JS `%` keeps the sign), no trimming"""
    return [_js_mod(c * scalar, p) for c in poly]


def bigintToBits(value):
    """index.js:558-566: least significant bit first, [] for 0"""
    bits = []
    while value > 0:
        bits.append(value & 1)
        value >>= 1
    return bits


def bitsToBigInt(bits):
    """index.js:568-570: BigInt('0b' + bits.join(''))"""
    return int("".join(str(b) for b in bits), 2)


def multiplyPolynomials(a, b, p, engine=None):
    """index.js:319-355: linear product, each coefficient in [0,p), trailing zeros trimmed.

    Runs on the GPU as one polymul-split in a ring large enough to hold both operands; the linear
    product is recovered from (quotient, remainder): c[N+k] = -quot[k], c[k] = rem[k] - c[N+k].  Moduli the packed
    kernels do not take (above 65536: test/circuits.test.js:72 uses 2^20) run on the generic family."""
    if len(a) == 0 or len(b) == 0:
        return [0]
    eng = engine or default_engine()
    N = max(len(a), len(b), 2)
    if not _fast_modulus(N, p):
        return eng.generic_multiply(list(a), list(b), p)[0]
    ar = np.array([x % p for x in expandArray(a, N)], dtype=np.int64)
    br = np.array([x % p for x in expandArray(b, N)], dtype=np.int64)
    quot, rem = eng.polymul_split(N, p, ar.astype(np.uint16), br.astype(np.uint16))
    hi = (p - quot[0].astype(np.int64)) % p
    lo = (rem[0].astype(np.int64) - hi) % p
    return trimPolynomial(lo.tolist() + hi.tolist()[:N - 1])


def dividePolynomials(a, b, p, engine=None):
    """index.js:358-401.  The hot path's divisor b = I = [1, 0, ..., 0, -1] with a reduced dividend runs the elementwise
    split kernel (ntru_split_by_I; inside encrypt/decrypt/verify the split is fused into the product kernel); any other
    divisor is long division on the generic family, errors included."""
    if degree(b) == -1:
        raise ReferenceError_("Cannot divide by zero polynomial.")
    eng = engine or default_engine()
    N = len(b) - 1
    if not (2 <= p <= 65536 and _is_I(b, p) and len(a) <= 2 * N and all(0 <= x < p for x in a)):
        quot, rem, st = eng.generic_divide(list(a), list(b), p)
        _raise_status(st[0])
        return {"quotient": quot[0], "remainder": rem[0]}
    quot, rem = eng.split_by_I(N, p, [expandArray(a, 2 * N)])
    nq = max(len(a) - N, 0)
    quotient = trimPolynomial(quot[0].tolist()[:nq]) if nq else [0]
    return {"quotient": quotient, "remainder": trimPolynomial(rem[0].tolist())}


def extendedEuclideanAlgorithm(a, b, p, engine=None):
    """index.js:425-459 -> {'gcd', 'inverse'}"""
    eng = engine or default_engine()
    gcd, inv, st = eng.generic_eea(list(a), list(b), p)
    _raise_status(st[0])
    return {"gcd": gcd[0], "inverse": inv[0]}


def polyInv(polyIn, polyI, polyMod, engine=None):
    """index.js:491-514.  Ternary f, polyI = 1 - x^N and modulus 3 or a power of two take the batched inversion kernels
    (the inverse of a unit is unique); everything else, and every f those kernels flag, runs the reference's own sequence
    on the generic family."""
    eng = engine or default_engine()
    N = len(polyI) - 1
    pow2 = 2 <= polyMod <= 65536 and polyMod & (polyMod - 1) == 0
    if (len(polyIn) <= N and all(x in (-1, 0, 1) for x in polyIn) and 2 <= N and eng.supports(N, 2) and
            (polyMod == 3 or pow2) and polyI[0] == 1 and polyI[N] == -1 and all(x == 0 for x in polyI[1:N])):
        f = [expandArray(list(polyIn), N)]
        if polyMod == 3:
            _, fp, flags = eng.invert_key_batch(N, 2, 3, f, want_fq=False)
            if not int(flags[0]) & FLAG_NOT_UNIT_MODP:
                return trimPolynomial(fp[0].tolist())
        else:
            fq, _, flags = eng.invert_key_batch(N, polyMod, 3, f, want_fp=False)
            if not int(flags[0]) & FLAG_NOT_UNIT_MOD2:
                return trimPolynomial(fq[0].tolist())
    inv, st = eng.generic_poly_inv(list(polyIn), list(polyI), polyMod)
    _raise_status(st[0])
    return inv[0]


def addCiphertexts(e1, e2, q, engine=None):
    """addPolynomials on the GPU (index.js:235-244) for operands already in [0,q): the homomorphic sum of
    test/reference.test.js:46-61."""
    eng = engine or default_engine()
    N = max(len(e1), len(e2), 1)
    out = eng.add_batch(N, q, [expandArray(e1, N)], [expandArray(e2, N)])
    return trimPolynomial(out[0].tolist())


def sumCiphertexts(rows, q, offsets=None, weights=None, engine=None):
    """The homomorphic sum of many ciphertexts in one device pass: addPolynomials (index.js:235-244) folded over every group of
    `rows` (lists of coefficients in [0, q)), each row first scaled by its weight as multiplyPolynomialsByScalar does.  offsets:
    [G + 1] row indices, group g is rows[offsets[g]:offsets[g + 1]]; None: one group of all rows.  Returns the trimmed sum (one
    list), or a list of them when offsets is given."""
    eng = engine or default_engine()
    rows = [list(r) for r in rows]
    N = max([len(r) for r in rows] + [2])
    if weights is not None:
        weights = [int(w) % q for w in weights]
    out = eng.sum_groups(N, q, np.array([expandArray(r, N) for r in rows], dtype=np.uint16).reshape(-1, N), offsets=offsets,
                         weights=weights)
    sums = [trimPolynomial(row.tolist()) for row in out]
    return sums if offsets is not None else sums[0]


def combineCiphertexts(rows, q, weights, engine=None):
    """G linear combinations of the same ciphertexts in one device pass: weights[b] holds the G weights of rows[b] (lists of
    coefficients in [0, q)), and combination g is addPolynomials (index.js:235-244) folded over every row scaled by weights[b][g] as
    multiplyPolynomialsByScalar does.  Returns the G trimmed sums; sumCiphertexts(rows, q, weights=column g) is entry g."""
    eng = engine or default_engine()
    rows = [list(r) for r in rows]
    N = max([len(r) for r in rows] + [2])
    weights = np.asarray([[int(w) % q for w in row] for row in weights], dtype=np.uint16)
    out = combine_calls.combine_batch(eng, N, q, np.array([expandArray(r, N) for r in rows], dtype=np.uint16).reshape(-1, N), weights)
    return [trimPolynomial(row.tolist()) for row in out]


def packOutput(maxVal, dataLen, data, engine=None):
    """index.js:572-596: same dict as the reference; `expected` is a list of Python ints (the reference's BigInts)."""
    eng = engine or default_engine()
    pr = eng.pack_params(maxVal, dataLen)
    limbs = eng.pack_batch(maxVal, dataLen, [expandArray(data, dataLen)])[0]
    expected = [sum(int(w) << (64 * k) for k, w in enumerate(row)) for row in limbs]
    return {"maxInputBits": pr["maxInputBits"], "maxOutputBits": pr["numInputsPerOutput"] * pr["maxInputBits"],
            "outputSize": pr["outputSize"], "arrLen": pr["arrLen"], "expected": expected}


def unpackInput(maxVal, packedBits, data, engine=None):
    """index.js:598-620 (`data`: list of ints below 2^256)."""
    eng = engine or default_engine()
    bits = eng.pack_params(maxVal, 0)["maxInputBits"]
    per = packedBits // bits
    limbs = np.array([[(int(v) >> (64 * k)) & 0xFFFFFFFFFFFFFFFF for k in range(4)] for v in data], dtype=np.uint64)
    un = eng.unpack_batch(maxVal, packedBits, limbs[None])[0].tolist() if len(data) else []
    return {"maxInputBits": bits, "packedBits": packedBits, "packedSize": len(data), "unpackedSize": per * len(data),
            "unpacked": trimPolynomial(un)}


# ---- the scheme class --------------------------------------------------------------------------------------

class NTRU:
    """index.js:7-207, hot-path methods.  Every return value is made of plain Python lists / ints.

    lift="reference" (the default) decrypts with index.js:117 verbatim and never touches the engine's mode; lift="centred" runs every
    decrypt-family method (decryptBits, decryptStr, decryptBytes, tallyBatch, tallyPacked, decryptPackedBatch, decryptBatchPerKey, scanBytes,
    scanPacked, countBytes, countPacked, the decrypt stage of pipeline) with the engine in the centred mode and puts the engine back into the mode it had (lift.py), so
    an engine shared by two instances is never left in the other's mode.  The centred mode returns the plaintext where the reference's
    `+ 1` does not (q = 4096 with p = 3, p = 5 or 7 at almost every q).  The `params` of a witness do not depend on the mode;
    VerifyDecrypt (checkWitnesses) accepts a centred witness only when the addend (p - q % p) % p is 1."""

    def __init__(self, options=None, engine=None, **kw):
        opts = dict(N=167, p=3, q=128, df=61, dg=20, dr=18, f=None, fp=None, fq=None, g=None, h=None)  # index.js:9-23
        opts["lift"] = "reference"
        opts.update(options or {})
        opts.update(kw)
        lift_calls.mode_number(opts["lift"])                                                          # ValueError for an unknown mode
        for k, v in opts.items():
            setattr(self, k, v)
        self.I = [1] + [0] * (self.N - 1) + [-1]                                                      # index.js:25-27
        self._engine = engine

    @property
    def engine(self):
        if self._engine is None:
            self._engine = default_engine()
        return self._engine

    def _lifted(self):
        """The engine in this instance's lift for the duration of a decrypt-family call; the default mode leaves the engine alone."""
        if lift_calls.mode_number(self.lift) == lift_calls.REFERENCE:
            return contextlib.nullcontext()
        return lift_calls.using(self.engine, lift_calls.CENTRED)

    def calculateNq(self):
        """index.js:201-203"""
        return int(np.ceil(np.log2(float(self.q) * self.q * self.N)))

    def calculateNp(self):
        """index.js:204-206"""
        return int(np.ceil(np.log2(float(self.p) * self.p * self.N)))

    # -- encryptBits, index.js:87-110 ---------------------------------------------------------------------
    def encryptBits(self, m, r=None):
        """`r` (signed ternary, length N) may be supplied for replay; by default it is sampled like the reference."""
        N, q, p = self.N, self.q, self.p
        if r is None:
            r = generateCustomArray(N, self.dr, self.dr)
        r = [p - 1 if x == -1 else x for x in r]                                     # :89
        m_pad, h_pad = expandArray(m, N), expandArray(self.h, N)
        # addPolynomials(m, rhq, q) reduces any integer m[i] modulo q (index.js:91, :241); the device adds a byte
        m_dev = [x % q for x in m_pad]
        if q > 256 and any(x > 255 for x in m_dev):       # does not fit the byte operand: the three steps separately
            rhqm = addPolynomials(m, multiplyPolynomials(r, self.h, q, self.engine), q)
            d = dividePolynomials(rhqm, self.I, q, self.engine)
            return {"value": trimPolynomial(d["remainder"]),
                    "inputs": {"r": r, "m": m_pad, "h": h_pad, "quotientE": expandArray(d["quotient"], N + 1),
                               "remainderE": expandArray(d["remainder"], N + 1)},
                    "params": [q, self.calculateNq(), N]}
        e, quot = self.engine.encrypt_batch(N, q, h_pad, [r], [m_dev], want_quot=True)
        e, quot = e[0].tolist(), quot[0].tolist()
        return {
            "value": trimPolynomial(e),
            "inputs": {"r": r, "m": m_pad, "h": h_pad, "quotientE": quot + [0], "remainderE": e + [0]},
            "params": [q, self.calculateNq(), N],
        }

    # -- decryptBits, index.js:111-140 --------------------------------------------------------------------
    def decryptBits(self, e):
        N, q, p = self.N, self.q, self.p
        if self.f is None:
            raise TypeError("Cannot read property 'map' of null")                  # what index.js:112 does
        e_pad = expandArray(e, N)
        f_signed = expandArray(self.f, N)
        with self._lifted():
            value, q1, r1, q2 = self.engine.decrypt_batch(N, q, p, f_signed, expandArray(self.fp, N), [e_pad])
        value = value[0].tolist()
        return {
            "value": trimPolynomial(value),
            "inputs": {
                "f": [q - 1 if x == -1 else x for x in f_signed],
                "fp": expandArray(self.fp, N),
                "e": e_pad,
                "quotient1": q1[0].tolist() + [0],
                "remainder1": r1[0].tolist() + [0],
                "quotient2": q2[0].tolist() + [0],
                "remainder2": value + [0],
            },
            "params": [q, self.calculateNq(), p, self.calculateNp(), N],
        }

    # -- loadPrivateKeyF, index.js:30-49 -------------------------------------------------------------------
    def loadPrivateKeyF(self, fArr):
        """fq = f^-1 mod q, fp = f^-1 mod p.  Units take the batched inversion kernels (unique inverses = the reference's,
        its validity checks pass by construction); an f those kernels flag runs the reference's own sequence on the
        generic family: same assignments in the same order, same errors, same acceptance of the non-units its `&&`
        checks let through (index.js:41-45, :451)."""
        N, q, p = self.N, self.q, self.p
        fArr = list(fArr)
        if (len(fArr) <= N and all(x in (-1, 0, 1) for x in fArr) and p == 3 and q & (q - 1) == 0 and
                self.engine.supports(N, q)):
            fq, fp, flags = self.engine.invert_key_batch(N, q, p, [expandArray(fArr, N)])
            if not int(flags[0]) & (FLAG_NOT_UNIT_MOD2 | FLAG_NOT_UNIT_MODP):
                self.f = fArr
                self.fq, self.fp = trimPolynomial(fq[0].tolist()), trimPolynomial(fp[0].tolist())
                return True
        self.f = fArr
        self.fq = polyInv(self.f, self.I, q, self.engine)
        self.fp = polyInv(self.f, self.I, p, self.engine)
        fmodq = [q - 1 if x == -1 else x for x in self.f]
        fmodp = [p - 1 if x == -1 else x for x in self.f]
        rem = dividePolynomials(multiplyPolynomials(self.fq, fmodq, q, self.engine), self.I, q, self.engine)["remainder"]
        if len(rem) != 1 and rem[0] != 1:
            raise ReferenceError_("invalid fq")
        rem = dividePolynomials(multiplyPolynomials(self.fp, fmodp, p, self.engine), self.I, p, self.engine)["remainder"]
        if len(rem) != 1 and rem[0] != 1:
            raise ReferenceError_("invalid fp")
        return True

    def generatePrivateKeyF(self, max_tries=100):
        """index.js:51-65: draw f with df ones and df - 1 minus ones until it is invertible.  Only the reference's own
        errors mean "next f"; an engine or GPU failure propagates."""
        i, retval = 0, None
        while (not retval or not (self.fq and self.fp)) and i < max_tries:
            i += 1
            try:
                retval = self.loadPrivateKeyF(generateCustomArray(self.N, self.df, self.df - 1))
            except ReferenceError_:
                pass
        if not self.fq or not self.fp:
            raise ValueError("Could not find invertible f")

    def generateNewPublicKeyGH(self):                                       # index.js:67-70
        self.g = generateCustomArray(self.N, self.dg, self.dg)
        self.generatePublicKeyH()

    # -- batched key generation: generatePrivateKeyF + generateNewPublicKeyGH (index.js:51-79) for B items on the device --------
    def generateKeysBatch(self, B, key, firstItem=0, maxTries=100):
        """B key pairs from the ChaCha20 stream under `key` (8 uint32, secret: take it from a CSPRNG, never the key that draws r):
        item i = firstItem + b, positions as include/ntru_engine.h ntru_keygen_batch says.  Returns the engine's dict of arrays
        (f, g, fq, fp, h, tries, flags); a nonzero flags[b] is an item for which no f of maxTries draws was invertible."""
        return self.engine.keygen_batch(self.N, self.q, self.p, self.df, self.dg, key, B, first_item=firstItem, max_tries=maxTries)

    def loadKeyFromBatch(self, keys, i):
        """Sets f, fq, fp, g, h from item i of generateKeysBatch as generatePrivateKeyF + generateNewPublicKeyGH leave them: f and g
        signed length-N lists, fq, fp and h trimmed.  Throws the reference's 'Could not find invertible f' for a failed item."""
        if int(keys["flags"][i]):
            raise ValueError("Could not find invertible f")
        self.f = [int(x) for x in keys["f"][i]]
        self.fq = trimPolynomial([int(x) for x in keys["fq"][i]])
        self.fp = trimPolynomial([int(x) for x in keys["fp"][i]])
        self.g = [int(x) for x in keys["g"][i]]
        self.h = trimPolynomial([int(x) for x in keys["h"][i]])
        return self

    # -- one key pair per item: row b goes with item b of a generateKeysBatch result ------------------------------------------------
    def _per_key_rows(self, keys, B, names):
        flags = np.asarray(keys["flags"])
        if flags.shape[0] < B:
            raise ValueError("batch per key: keys hold fewer than B items")
        if np.any(flags[:B]):
            raise ValueError("Could not find invertible f")
        return [np.asarray(keys[n])[:B] for n in names]

    def encryptBatchPerKey(self, keys, r, m):
        """encryptBits for B items, item b under key b of `keys` (generateKeysBatch; its first B items are used).  r: [B][N] signed
        ternary or already mapped to {0, 1, p-1} (index.js:89); m: [B][N] bytes (index.js:91 adds them mod q).  Returns
        {"e", "quotientE"} as [B][N] uint16 arrays: row b equals remainderE / quotientE of loadKeyFromBatch(keys, b).encryptBits."""
        N, q, p = self.N, self.q, self.p
        r = np.asarray(r).reshape(-1, N)
        r = np.where(r == -1, p - 1, r).astype(np.uint8)
        (h,) = self._per_key_rows(keys, r.shape[0], ["h"])
        e, quot = self.engine.encrypt_peritem_batch(N, q, h, r, m)
        return {"e": e, "quotientE": quot}

    def decryptBatchPerKey(self, keys, e):
        """decryptBits for B ciphertexts, item b under key b of `keys`.  Returns {"value", "quotient1", "remainder1", "quotient2"} as
        [B][N] arrays: row b equals the witness arrays of loadKeyFromBatch(keys, b).decryptBits(e[b])."""
        N, q, p = self.N, self.q, self.p
        e = np.asarray(e).reshape(-1, N)
        f, fp = self._per_key_rows(keys, e.shape[0], ["f", "fp"])
        with self._lifted():
            value, q1, r1, q2 = self.engine.decrypt_peritem_batch(N, q, p, f, fp, e)
        return {"value": value, "quotient1": q1, "remainder1": r1, "quotient2": q2}

    # -- tallies: decryptBits of sums of ciphertexts -----------------------------------------------------------------------------------
    def tallyBatch(self, rows, offsets=None, weights=None, wantWitness=True):
        """Sums the ciphertexts `rows` [B][N] in groups (offsets: [G + 1] row indices; None: one group of every row), each row scaled
        by its weight (None: 1), and decrypts every sum.  Returns {"sum", "value", "quotient1", "remainder1", "quotient2"} as [G][N]
        arrays (the witness arrays are None without wantWitness): row g equals the witness arrays of decryptBits(sum[g])."""
        N, q, p = self.N, self.q, self.p
        if self.f is None:
            raise TypeError("Cannot read property 'map' of null")
        rows = np.asarray(rows).reshape(-1, N)
        if weights is not None:
            weights = np.asarray(weights, dtype=np.int64) % q
        with self._lifted():
            total, value, q1, r1, q2 = self.engine.tally_decrypt_batch(N, q, p, expandArray(self.f, N), expandArray(self.fp, N), rows,
                                                                       offsets=offsets, weights=weights, want_witness=wantWitness)
        return {"sum": total, "value": value, "quotient1": q1, "remainder1": r1, "quotient2": q2}

    def combineBatch(self, rows, weights, want_witness=True):
        """Combines the ciphertexts `rows` [B][N] by the weight matrix `weights` [B][G] (row b: the weights of row b in the G outputs)
        and decrypts every combination.  Returns {"sum", "value", "quotient1", "remainder1", "quotient2"} as [G][N] arrays (the witness
        arrays are None without want_witness): row g equals the witness arrays of decryptBits(sum[g])."""
        N, q, p = self.N, self.q, self.p
        if self.f is None:
            raise TypeError("Cannot read property 'map' of null")
        rows = np.asarray(rows).reshape(-1, N)
        weights = np.asarray(weights, dtype=np.int64) % q
        total = combine_calls.combine_batch(self.engine, N, q, rows, weights)
        with self._lifted():
            value, q1, r1, q2 = self.engine.decrypt_batch(N, q, p, expandArray(self.f, N), expandArray(self.fp, N), total,
                                                          want_witness=want_witness)
        return {"sum": total, "value": value, "quotient1": q1, "remainder1": r1, "quotient2": q2}

    def multiplyByPolynomialBatch(self, rows, poly, want_quot=False):
        """rows [B][N] (ciphertexts, or any rows modulo q) times the one polynomial `poly` (coefficients of any sign, at most N of them)
        modulo (x^N - 1, q): row b is dividePolynomials(multiplyPolynomials(rows[b], poly, q), I, q).  Returns the remainders [B][N],
        or (quotients, remainders) with want_quot.  A ciphertext's noise grows by the 1-norm of poly."""
        N, q = self.N, self.q
        s = np.asarray(expandArray(list(poly), N), dtype=np.int64) % q
        quot, rem = shared_calls.mul_shared_batch(self.engine, N, q, s, np.asarray(rows).reshape(-1, N), want_quot=want_quot)
        return (quot, rem) if want_quot else rem

    def noiseBatch(self, rows, packed=False):
        """The decryption noise of the ciphertexts `rows` ([B][N], or packed rows [B][outputSize][4] with packed=True) under this key:
        {"peak", "energy", "margin"} as [B] arrays, peak = max |a centred at q/2| and energy = the sum of its squares for
        a = remainder1 of decryptBits(row), margin = q // 2 - peak.  A row whose noise has wrapped past q/2 shows the norm of the
        wrapped value only: keep a guard band."""
        N, q = self.N, self.q
        if self.f is None:
            raise TypeError("Cannot read property 'map' of null")
        f = expandArray(self.f, N)
        if packed:
            peak, energy = noise_calls.noise_packed_batch(self.engine, N, q, f, rows)
        else:
            peak, energy = noise_calls.noise_batch(self.engine, N, q, f, np.asarray(rows).reshape(-1, N))
        return {"peak": peak, "energy": energy, "margin": (q // 2 - peak.astype(np.int64))}

    def dedupBatch(self, rows, packed=False, prior=None, salt=None):
        """Which of the ciphertexts `rows` ([B][N], or packed rows [B][outputSize][4] with packed=True) repeat an earlier row of the
        batch or of `prior` (rows accepted before, same format): {"first", "unique"}.  Rows are equal when every coefficient agrees
        modulo q.  The S prior rows take the indices 0 .. S - 1 and the new rows S .. S + B - 1; first[b] is the smallest index of a
        row equal to row b, unique the batch-local indices of the rows with first[b] == S + b, ascending.  salt keys the fingerprint
        that is sorted and never changes the result; None draws one from `secrets`."""
        N, q = self.N, self.q
        if salt is None:
            salt = secrets.randbits(64)
        if packed:
            first, unique = dedup_calls.dedup_packed(self.engine, N, q, rows, prior=prior, salt=salt)
        else:
            first, unique = dedup_calls.dedup_rows(self.engine, N, q, np.asarray(rows).reshape(-1, N),
                                                   prior=None if prior is None else np.asarray(prior).reshape(-1, N), salt=salt)
        return {"first": first, "unique": unique}

    # -- the same on ciphertexts in the wire format: rows of packOutput(q - 1, N, e), uint64 [B][outputSize][4] ----------------------------
    def tallyPacked(self, packed, offsets=None, weights=None, wantWitness=True):
        """tallyBatch on packed rows, summed straight from the field elements: the same dict, sum included, as dense [G][N] arrays."""
        N, q, p = self.N, self.q, self.p
        if self.f is None:
            raise TypeError("Cannot read property 'map' of null")
        if weights is not None:
            weights = np.asarray(weights, dtype=np.int64) % q
        with self._lifted():
            total, value, q1, r1, q2 = packed_calls.tally_decrypt_packed_batch(self.engine, N, q, p, expandArray(self.f, N),
                                                                               expandArray(self.fp, N), packed, offsets=offsets,
                                                                               weights=weights, want_witness=wantWitness)
        return {"sum": total, "value": value, "quotient1": q1, "remainder1": r1, "quotient2": q2}

    def decryptPackedBatch(self, packed, wantWitness=True):
        """decryptBits for B packed ciphertexts.  Returns {"value", "quotient1", "remainder1", "quotient2"} as [B][N] arrays: row b
        equals the witness arrays of decryptBits(unpacked row b)."""
        N, q, p = self.N, self.q, self.p
        if self.f is None:
            raise TypeError("Cannot read property 'map' of null")
        with self._lifted():
            value, q1, r1, q2 = packed_calls.decrypt_packed_batch(self.engine, N, q, p, expandArray(self.f, N), expandArray(self.fp, N),
                                                                  packed, want_witness=wantWitness)
        return {"value": value, "quotient1": q1, "remainder1": r1, "quotient2": q2}

    # -- one mix step: encryptBits (index.js:87-110) with an old ciphertext in the place of m ------------------------------------------
    def reencryptBatch(self, e, r=None, src=None, wantWitness=True):
        """Re-randomises the ciphertexts `e` [B_in][N] under h: output row i is (Enc(0; r[i]) + e[src[i]]) mod q (src None: row i;
        any gather, repeats allowed).  r: [B][N] signed ternary or already mapped to {0, 1, p - 1} (index.js:89); None draws every row
        as encryptBits does.  Returns {"value", "r", "m", "quotientE"} as [B][N] arrays: m is the gathered rows, and
        {r, m, h, quotientE, remainderE: value} satisfies VerifyEncrypt (quotientE is None without wantWitness)."""
        N, q, p = self.N, self.q, self.p
        e = np.asarray(e).reshape(-1, N)
        if src is not None:
            src = np.asarray(src, dtype=np.int64).reshape(-1)
            if np.any((src < 0) | (src >= e.shape[0])):
                raise ValueError("reencryptBatch: src index outside the rows of e")
        B = e.shape[0] if src is None else src.shape[0]
        if r is None:
            r = [generateCustomArray(N, self.dr, self.dr) for _ in range(B)]
        r = np.asarray(r).reshape(-1, N)
        r = np.where(r == -1, p - 1, r).astype(np.uint8)
        m = np.ascontiguousarray((e if src is None else e[src]) % q).astype(np.uint16)
        value, quot = mix_calls.reencrypt_batch(self.engine, N, q, expandArray(self.h, N), r, e % q, src=src, want_quot=wantWitness)
        return {"value": value, "r": r, "m": m, "quotientE": quot}

    def mixBatch(self, e, key, firstItem=0, permId=0, wantWitness=True):
        """One mix step of the ciphertexts `e` [B][N] from a ChaCha20 key (8 words): r[i] is row firstItem + i of the on-device sampler
        (dr ones, dr entries p - 1), src the permutation drawn on the device under (key, permId), output row i is
        (Enc(0; r[i]) + e[src[i]]) mod q.  Returns {"value", "r", "m", "src", "quotientE"}: m is the gathered rows, and
        {r, m, h, quotientE, remainderE: value} satisfies VerifyEncrypt (quotientE is None without wantWitness)."""
        N, q, p = self.N, self.q, self.p
        e = np.ascontiguousarray(np.asarray(e).reshape(-1, N) % q).astype(np.uint16)
        value, quot, r, src = mix_calls.mix_batch(self.engine, N, q, p, expandArray(self.h, N), key, firstItem, self.dr, self.dr, permId, e,
                                                  want_quot=wantWitness)
        return {"value": value, "r": r, "m": e[src], "src": src, "quotientE": quot}

    def auditLinks(self, e_in, e_out, r, in_idx=None, out_idx=None):
        """Checks revealed re-encryption links under h: link l holds when e_out[out_idx[l]] == r[l] * h + e_in[in_idx[l]] modulo
        (x^N - 1, q) (an index list of None: row l).  r: [L][N] signed ternary or already mapped to {0, 1, p - 1}, which must hold dr
        ones and dr entries p - 1.  Returns {"flags", "bad"}: one byte per link (0, or audit.LINK_*) and the number that are not 0."""
        N, q, p = self.N, self.q, self.p
        r = np.asarray(r).reshape(-1, N)
        r = np.where(r == -1, p - 1, r).astype(np.uint8)
        flags, bad = audit_calls.check_links(self.engine, N, q, expandArray(self.h, N), r, np.asarray(e_in).reshape(-1, N) % 65536,
                                             np.asarray(e_out).reshape(-1, N) % 65536, in_idx=in_idx, out_idx=out_idx, other=p - 1,
                                             n1=self.dr, n2=self.dr)
        return {"flags": flags, "bad": bad}

    # -- generatePublicKeyH, index.js:72-79 ----------------------------------------------------------------
    def generatePublicKeyH(self):
        """h = trim((p*fq mod q) * g mod (x^N - 1, q)) on the device."""
        if not self.f:
            raise ValueError("missing private key F")
        if not self.g:
            raise ValueError("missing private key G")
        if not self.fq:
            raise TypeError("Cannot read property 'map' of null")              # what index.js:76 does without fq
        h = self.engine.public_key_batch(self.N, self.q, self.p, [expandArray(self.fq, self.N)], [expandArray(self.g, self.N)])
        self.h = trimPolynomial(h[0].tolist())

    # -- verifyKeysInputs, index.js:141-197 ---------------------------------------------------------------
    def verifyKeysInputs(self):
        for attr, msg in (("f", "missing private key F"), ("fq", "missing private key Fq"),
                          ("fp", "missing private key Fp"), ("g", "missing private key G"),
                          ("h", "missing public key H")):
            if not getattr(self, attr):
                raise ValueError(msg)
        N, q, p = self.N, self.q, self.p
        pad = lambda a: expandArray(a, N)
        out = self.engine.verify_keys_batch(N, q, p, [pad(self.f)], [pad(self.g)], [pad(self.fq)], [pad(self.fp)],
                                            [pad(self.h)])
        flags = int(out["flags"][0])
        if flags & FLAG_INVALID_FQ:
            raise ValueError("invalid fq")
        if flags & FLAG_INVALID_FP:
            raise ValueError("invalid fp")
        # index.js:165 walks h as the caller stored it (untrimmed tails count): redo that literal check here
        rem_h = trimPolynomial(out["rem_h"][0].tolist())
        if flags & FLAG_INVALID_H or any(i >= len(rem_h) or rem_h[i] != cur for i, cur in enumerate(self.h)):
            raise ValueError("invalid h")
        nq, np_ = self.calculateNq(), self.calculateNp()
        row = lambda name: out[name][0].tolist() + [0]
        return {
            "fq": {"params": [q, nq, N],
                   "inputs": {"f": [q - 1 if x == -1 else x for x in pad(self.f)], "fq": pad(self.fq),
                              "quotientI": row("quot_fq"), "remainderI": row("rem_fq")}},
            "fp": {"params": [p, np_, N],
                   "inputs": {"f": [p - 1 if x == -1 else x for x in pad(self.f)], "fq": pad(self.fp),
                              "quotientI": row("quot_fp"), "remainderI": row("rem_fp")}},
            "h": {"params": [q, nq, N],
                  "inputs": {"f": [q - 1 if x == -1 else x for x in pad(self.g)], "fq": [x * p for x in pad(self.fq)],
                             "quotientI": row("quot_h"), "remainderI": row("rem_h")}},
        }

    # -- string helpers, index.js:80-86 -------------------------------------------------------------------
    # ---- additive batch API (the Node shim's ntru.pipeline): stages chained on the GPU, only m up, only what is asked for down
    def pipeline(self, m, sampleR=None, r=None, decrypt=False, pack=False, want=None):
        """m: [B][N] plaintext coefficients.  sampleR = (key[8] uint32, firstItem): r = generateCustomArray(N, dr, dr) with -1 -> p-1
        (index.js:89, :461-488) drawn on the device from a ChaCha20 stream -- or r: [B][N].  encryptBits always (index.js:87-110);
        decrypt: decryptBits of the fresh ciphertexts (index.js:111-140); pack: packOutput (index.js:572-596) of the last stage's
        result.  want: subset of {"r", "e", "value"} (default: e without decrypt, value with it, only `packed` when pack is set)."""
        N = self.N
        if (sampleR is None) == (r is None):
            raise ValueError("pipeline: give either sampleR=(key, firstItem) or r")
        want = set(want) if want is not None else (set() if pack else ({"value"} if decrypt else {"e"}))
        pad = lambda a, dt: np.array(list(a) + [0] * (N - len(a)), dtype=dt)
        key, first = (sampleR if sampleR is not None else (None, 0))
        with (self._lifted() if decrypt else contextlib.nullcontext()):
            return self.engine.pipeline_batch(N, self.q, self.p, pad(self.h, np.uint16), m,
                                              f=pad(self.f, np.int8) if decrypt else None, fp=pad(self.fp, np.uint8) if decrypt else None,
                                              key=key, first_item=first, n1=self.dr, n2=self.dr, r=r,
                                              want_r="r" in want and key is not None, want_e="e" in want, want_value="value" in want,
                                              want_packed=pack)

    # -- byte messages of any length, as packed bits (the reference's encryptStr takes at most N bits, index.js:81) ------------------
    @property
    def bytesPerBlock(self):
        return self.N // 8

    def encryptBytes(self, data, r=None):
        """`data` (bytes, or a latin-1 str: stringToBits, index.js:538-546, misaligns for char codes above 255 and that artefact is not
        reproduced) is cut into ceil(len / W) blocks of W = bytesPerBlock bytes, the last one zero padded, and every block encrypted as
        encryptStr encrypts it (index.js:80-83); the bits are expanded on the device.  r: [blocks][N], signed ternary or mapped to
        {0, 1, p-1}; drawn per block like encryptBits' by default.  Returns the [blocks][N] uint16 ciphertext array."""
        if isinstance(data, str):
            try:
                data = data.encode("latin-1")
            except UnicodeEncodeError:
                raise ValueError("encryptBytes: a str must be latin-1 (char codes below 256); encode it to bytes first") from None
        data = bytes(data)
        N, p, W = self.N, self.p, self.bytesPerBlock
        if W < 1:
            raise ValueError("encryptBytes: N = %d holds no whole byte" % N)
        blocks = -(-len(data) // W)
        if r is None:
            r = [generateCustomArray(N, self.dr, self.dr) for _ in range(blocks)]
        r = np.asarray(r, dtype=np.int64).reshape(-1, N)
        if r.shape[0] != blocks:
            raise ValueError("encryptBytes: %d rows of r for %d blocks" % (r.shape[0], blocks))
        r = np.where(r == -1, p - 1, r).astype(np.uint8)                            # index.js:89
        padded = np.frombuffer(data + bytes(blocks * W - len(data)), np.uint8).reshape(blocks, W)
        e, _ = self.engine.encrypt_bytes_batch(N, self.q, W, expandArray(self.h, N), r, padded, want_quot=False)
        return e

    def decryptBytes(self, e, length=None):
        """decryptStr (index.js:84-86) of every block of e [blocks][N], the bits collected on the device.  Returns (data, flags): data is
        cut to `length` bytes when given, else its trailing zero bytes are stripped (what decryptStr does through trimPolynomial);
        flags [blocks] is 0 for a block that decrypted to bits with an empty pad, else FLAG_NOT_BITS | FLAG_PAD_NONZERO of the engine:
        a wrong key or a decryption failure, which the reference can only show as a garbled string."""
        N, W = self.N, self.bytesPerBlock
        if self.f is None:
            raise TypeError("Cannot read property 'map' of null")                  # what index.js:112 does
        e = np.asarray(e, dtype=np.uint16).reshape(-1, N)
        with self._lifted():
            out, flags = self.engine.decrypt_bytes_batch(N, self.q, self.p, W, expandArray(self.f, N), expandArray(self.fp, N), e)
        data = out.tobytes()
        if length is None:
            return data.rstrip(b"\x00"), flags
        if not 0 <= length <= len(data):
            raise ValueError("decryptBytes: length %d is outside the %d bytes of %d blocks" % (length, len(data), e.shape[0]))
        return data[:length], flags

    # -- scanning: which blocks does a key decrypt to a well-formed message that carries the expected tag? ----------------------------
    def _scan(self, call, rows, keys, tag, tagOffset, maxHits):
        N, W = self.N, self.bytesPerBlock
        if keys is None:
            if self.f is None:
                raise TypeError("Cannot read property 'map' of null")
            keys = [(self.f, self.fp)]
        f = [expandArray(list(k[0]), N) for k in keys]
        fp = [expandArray(list(k[1]), N) for k in keys]
        with self._lifted():
            count, rows_, data = call(self.engine, N, self.q, self.p, W, f, fp, rows, tag=tag, tag_off=tagOffset, max_hits=maxHits)
        return {"count": count, "rows": rows_, "bytes": data}

    def scanBytes(self, e, keys=None, tag=b"", tagOffset=0, maxHits=None):
        """Tries every key of `keys` -- (f, fp) pairs, f signed ternary; None: this instance's own key -- on every block of e
        [blocks][N] and keeps the hits: the blocks decryptBytes gives flag 0 for and whose bytes [tagOffset, tagOffset + len(tag)) equal
        `tag` (at most 32 bytes).  Decrypt, test and compaction run on the device; only the hits come back.  Returns {"count": [K] int64
        (every hit, may exceed maxHits), "rows", "bytes"}: per key the first min(count, maxHits) hits in ascending block order, block
        indices and [.][bytesPerBlock] uint8 messages.  maxHits None keeps every hit, 0 only counts."""
        return self._scan(scan_calls.scan_bytes_batch, np.asarray(e, dtype=np.uint16).reshape(-1, self.N), keys, tag, tagOffset, maxHits)

    def scanPacked(self, packed, keys=None, tag=b"", tagOffset=0, maxHits=None):
        """scanBytes on blocks in the wire format: rows of packOutput(q - 1, N, e), uint64 [blocks][outputSize][4]."""
        return self._scan(scan_calls.scan_bytes_packed_batch, packed, keys, tag, tagOffset, maxHits)

    # -- counting: how many blocks decrypt to each choice, per group? -----------------------------------------------------------------
    def _count(self, call, rows, firstChoice, nChoices, fieldOffset, fieldLength, tag, tagOffset, groups, G, classes):
        N = self.N
        if self.f is None:
            raise TypeError("Cannot read property 'map' of null")                  # what index.js:112 does
        with self._lifted():
            count, cls = call(self.engine, N, self.q, self.p, self.bytesPerBlock, expandArray(self.f, N), expandArray(self.fp, N), rows,
                              firstChoice, nChoices, fieldOffset, fieldLength, tag=tag, tag_off=tagOffset, groups=groups, G=G,
                              classes=classes)
        return {"count": count, "classes": cls}

    def countBytes(self, e, firstChoice, nChoices, fieldOffset, fieldLength, tag=b"", tagOffset=0, groups=None, G=1, classes=False):
        """Decrypts every block of e [blocks][N] once under this instance's key and counts the blocks by choice and group on the device.
        The class of a block is the first that applies of: decryptBytes gives it a flag -> nChoices + 2 (malformed); its bytes
        [tagOffset, tagOffset + len(tag)) differ from `tag` (at most 32 bytes) -> nChoices + 1 (wrong tag); v, the big-endian integer
        of its bytes [fieldOffset, fieldOffset + fieldLength) (1 to 4 bytes), lies outside [firstChoice, firstChoice + nChoices) ->
        nChoices (other); else v - firstChoice.  groups: [blocks] ids in [0, G), or None for one group.  Returns {"count": int64
        [G][nChoices + 3], "classes": int32 [blocks] or None (classes=False)}; only these cross the bus."""
        return self._count(count_calls.count_bytes_batch, np.asarray(e, dtype=np.uint16).reshape(-1, self.N), firstChoice, nChoices,
                           fieldOffset, fieldLength, tag, tagOffset, groups, G, classes)

    def countPacked(self, packed, firstChoice, nChoices, fieldOffset, fieldLength, tag=b"", tagOffset=0, groups=None, G=1, classes=False):
        """countBytes on blocks in the wire format: rows of packOutput(q - 1, N, e), uint64 [blocks][outputSize][4]."""
        return self._count(count_calls.count_bytes_packed_batch, packed, firstChoice, nChoices, fieldOffset, fieldLength, tag, tagOffset,
                           groups, G, classes)

    def encryptStr(self, inputPlain):
        return self.encryptBits(stringToBits(inputPlain))["value"]

    def decryptStr(self, encrypted):
        bits = self.decryptBits(encrypted)["value"]
        bits = bits + [0] * (-len(bits) % 8)                                     # expandArrayToMultiple(.., 8)
        return bitsToString(bits)


# ---- witness checks: VerifyEncrypt / VerifyDecrypt / VerifyInverse (circuits/ntru.circom) on the engine -------------------------
CHECK_SIGNALS = {"VerifyEncrypt": (("r", 0), ("m", 0), ("h", 0), ("quotientE", 1), ("remainderE", 1)),
                 "VerifyDecrypt": (("f", 0), ("fp", 0), ("e", 0), ("quotient1", 1), ("remainder1", 1), ("quotient2", 1),
                                   ("remainder2", 1)),
                 "VerifyInverse": (("f", 0), ("fq", 0), ("quotientI", 1), ("remainderI", 1))}
CHECK_PARAMS = {"VerifyEncrypt": 3, "VerifyDecrypt": 5, "VerifyInverse": 3}


def checkWitnesses(template, witnesses, engine=None):
    """Flags of each {inputs, params} witness (as encryptBits, decryptBits and verifyKeysInputs()[fq|fp|h] return them) against
    the circuit `template`: 0 = the constraint system is satisfied, else the NTRU_CHECK_* bits (EQ 1, TAIL 2, RANGE 4; VerifyDecrypt's
    mod-p stage shifted left by 3).  Every item must have the same params; every entry must be an integer in [0, 65535]."""
    if template not in CHECK_SIGNALS:
        raise ValueError("checkWitnesses: unknown template %r (VerifyEncrypt, VerifyDecrypt or VerifyInverse)" % (template,))
    witnesses = list(witnesses)
    if not witnesses:
        return []
    params = [int(x) for x in witnesses[0]["params"]]
    if len(params) != CHECK_PARAMS[template]:
        raise ValueError("checkWitnesses: %s takes %d params, got %d" % (template, CHECK_PARAMS[template], len(params)))
    N = params[-1]
    arrays = []
    for name, extra in CHECK_SIGNALS[template]:
        rows = []
        for i, w in enumerate(witnesses):
            if [int(x) for x in w["params"]] != params:
                raise ValueError("checkWitnesses: item %d has params %r, item 0 %r" % (i, list(w["params"]), params))
            v = w["inputs"].get(name)
            if v is None:
                raise ValueError("checkWitnesses: item %d: missing signal %s" % (i, name))
            if len(v) != N + extra:
                raise ValueError("checkWitnesses: item %d: %s has length %d, expected %d" % (i, name, len(v), N + extra))
            if not all(isinstance(x, (int, np.integer)) and not isinstance(x, bool) and 0 <= x <= 65535 for x in v):
                raise ValueError("checkWitnesses: item %d: %s holds an entry that is not an integer in [0, 65535]" % (i, name))
            rows.append(v)
        arrays.append(np.array(rows, np.uint16))
    eng = engine or default_engine()
    if template == "VerifyEncrypt":
        flags = eng.check_encrypt_batch(N, params[0], params[1], *arrays)
    elif template == "VerifyDecrypt":
        flags = eng.check_decrypt_batch(N, params[0], params[1], params[2], params[3], *arrays)
    else:
        flags = eng.check_inverse_batch(N, params[0], params[1], *arrays)
    return [int(x) for x in flags]
