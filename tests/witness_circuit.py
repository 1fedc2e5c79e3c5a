"""Two CPU evaluators of the reference's Verify* circuits (circuits/ntru.circom, circomlib 2.0.5), the yardsticks of the engine's
witness checks (ntru_check_*_batch).  Not a test module.

literal_*   follow the templates signal by signal over the BN254 scalar field: Modulus with its three LessThan / LessEqThan
            components, LessThan as Num2Bits(n + 1), IsEqual / IsZero, VerifyDividePolynomials on I = 1 + (M - 1) x^N.
numpy_*     the closed form of INTEGRATION.md ("Witness checks") on [B][N] int64 arrays: x < T(M, n), M - 2^n <= y < 2^n; exact
            because no signal of a witness with entries below 65536 reaches 2^43.

Both return flags with the bits of include/ntru_engine.h: EQ = 1, TAIL = 2, RANGE = 4, VerifyDecrypt's mod-p stage shifted by 3.
"""
import numpy as np

P = 21888242871839275222246405745257275088548364400416034343698204186575808495617   # BN254 scalar field (circom's default)
EQ, TAIL, RANGE = 1, 2, 4

TEMPLATES = ("VerifyEncrypt", "VerifyDecrypt", "VerifyInverse")
SIGNALS = {"VerifyEncrypt": (("r", 0), ("m", 0), ("h", 0), ("quotientE", 1), ("remainderE", 1)),
           "VerifyDecrypt": (("f", 0), ("fp", 0), ("e", 0), ("quotient1", 1), ("remainder1", 1), ("quotient2", 1), ("remainder2", 1)),
           "VerifyInverse": (("f", 0), ("fq", 0), ("quotientI", 1), ("remainderI", 1))}


# ---- literal evaluation --------------------------------------------------------------------------------------------------------
def num2bits_ok(v, n):
    """Num2Bits(n) on field element v is satisfiable iff v < 2^n (its bits sum back to v)."""
    return v % P < (1 << n)


def less_than(n, a, b):
    """circomlib LessThan(n): Num2Bits(n+1) of a + 2^n - b, out = 1 - bit n; returns (out, constraints satisfied).  When Num2Bits
    cannot be satisfied no assignment of its bits is valid and `out` is not defined by the constraints; the evaluator then takes
    the comparison the template stands for, [a < b] (what the flags contract of include/ntru_engine.h says for VerifyDecrypt's gt)."""
    assert n <= 252
    v = (a + (1 << n) - b) % P
    ok = num2bits_ok(v, n + 1)
    return (1 - ((v >> n) & 1)) if ok else int(a < b), ok


def less_eq_than(n, a, b):
    return less_than(n, a, b + 1)


def is_zero(x):
    return 1 if x % P == 0 else 0


def is_equal(a, b):
    return is_zero(b - a)


def modulus(M, n, x):
    """Modulus(M, n) of ntru.circom: y <-- x % M, q <-- x \\ M, x === q M + y, ltP.out === 1, gteZeroY.out === 1, ltQ.out === 0.
    Returns (y, satisfied)."""
    x %= P
    y, q = x % M, x // M
    ok = (q * M + y - x) % P == 0
    out, s = less_than(n, y, M); ok = ok and s and out == 1
    out, s = less_eq_than(n, 0, y); ok = ok and s and out == 1
    out, s = less_than(n, x, q); ok = ok and s and out == 0
    return y, ok


def multiply_polynomials(a, b):
    """MultiplyPolynomials(n): the linear product (field sums of integer products; exact in int64 for entries < 65536)."""
    return [int(v) % P for v in np.convolve(np.asarray(a, np.int64), np.asarray(b, np.int64))]


def verify_divide(M, n, Na, a, quotient, remainder):
    """VerifyDividePolynomials(M, n, Na, N+1)(a, I, quotient, remainder) with I = 1 + (M-1) x^N; returns the flag bits."""
    Nb = len(quotient)
    I = [0] * Nb
    I[0], I[Nb - 1] = 1, M - 1
    product = multiply_polynomials(I, quotient)
    fl = 0
    for i in range(2 * Nb - 1):
        y, ok = modulus(M, n, product[i] + (remainder[i] if i < Nb else 0))
        if not ok:
            fl |= RANGE
        if i < Na:
            fl |= 0 if is_equal(a[i], y) else EQ
        else:
            fl |= 0 if is_zero(y) else TAIL
    return fl


def _poly_mod(M, n, values):
    out, fl = [], 0
    for v in values:
        y, ok = modulus(M, n, v)
        out.append(y)
        fl |= 0 if ok else RANGE
    return out, fl


def literal_encrypt(params, inp):
    q, nq, N = params
    rhq = multiply_polynomials(inp["r"], inp["h"])
    a, fl = _poly_mod(q, nq, [rhq[i] + (inp["m"][i] if i < N else 0) for i in range(2 * N - 1)])
    return fl | verify_divide(q, nq, 2 * N - 1, a, inp["quotientE"], inp["remainderE"])


def literal_inverse(params, inp):
    M, n, N = params
    a, fl = _poly_mod(M, n, multiply_polynomials(inp["f"], inp["fq"]))
    return fl | verify_divide(M, n, 2 * N - 1, a, inp["quotientI"], inp["remainderI"])


def literal_decrypt(params, inp):
    q, nq, p, np_, N = params
    a, fl1 = _poly_mod(q, nq, multiply_polynomials(inp["f"], inp["e"]))
    fl1 |= verify_divide(q, nq, 2 * N - 1, a, inp["quotient1"], inp["remainder1"])
    assert q % 2 == 0
    b, fl2 = [], 0
    for i in range(N):
        x = inp["remainder1"][i]
        gt, ok = less_than(nq, q // 2, x)
        fl2 |= 0 if ok else RANGE
        y, ok = modulus(p, np_, x + gt)
        fl2 |= 0 if ok else RANGE
        b.append(y)
    c, f = _poly_mod(p, np_, multiply_polynomials(inp["fp"], b))
    fl2 |= f | verify_divide(p, np_, 2 * N - 1, c, inp["quotient2"], inp["remainder2"])
    return fl1 | (fl2 << 3)


LITERAL = {"VerifyEncrypt": literal_encrypt, "VerifyDecrypt": literal_decrypt, "VerifyInverse": literal_inverse}


def literal(template, witness):
    return LITERAL[template](witness["params"], witness["inputs"])


# ---- closed form, vectorised ---------------------------------------------------------------------------------------------------
def T_bound(M, n):
    """Modulus(M, n)(x) passes ltQ iff x < T(M, n)."""
    return (1 << n) + ((1 << n) - 1) // (M - 1)


def modulus_closed(M, n, x):
    """(y, ok) of Modulus(M, n) on int64 x >= 0 by the closed form."""
    x = np.asarray(x, np.int64)
    y = x % M
    T = T_bound(M, n)
    ok = (x < T) if T < (1 << 62) else np.ones(x.shape, bool)
    ok &= y < (1 << min(n, 62))
    if (1 << n) < M:
        ok &= y >= M - (1 << n)
    return y, ok


def less_than_closed(n, a, x):
    """(out, ok) of LessThan(n)(a, x) for integer x (a constant)."""
    x = np.asarray(x, np.int64)
    span = 1 << min(n, 40)
    return (x > a).astype(np.int64), (x > a - span) & (x <= a + span)


def _fft():
    try:
        import scipy.fft as sf
        return lambda a, n: sf.rfft(a, n, workers=-1), lambda a, n: sf.irfft(a, n, workers=-1)
    except ImportError:
        return np.fft.rfft, np.fft.irfft


def linear_product(a, b, chunk=4096):
    """Row-wise linear product of int64 [B][N] arrays with entries in [0, 65536): exact, through byte planes (each plane sum below
    2^27, so the float64 FFT rounds to the exact integer)."""
    a, b = np.asarray(a, np.int64), np.asarray(b, np.int64)
    B, N = a.shape
    L = 2 * N - 1
    if N <= 64:
        return np.stack([np.convolve(a[i], b[i]) for i in range(B)]) if B else np.zeros((0, L), np.int64)
    n = 1 << (L - 1).bit_length()
    rfft, irfft = _fft()
    out = np.empty((B, L), np.int64)
    for s in range(0, B, chunk):
        A = [rfft((a[s:s + chunk] >> (8 * j)) & 255, n) for j in (0, 1)]
        W = [rfft((b[s:s + chunk] >> (8 * j)) & 255, n) for j in (0, 1)]
        acc = np.zeros((min(chunk, B - s), L), np.int64)
        for sh, spec in ((0, A[0] * W[0]), (8, A[0] * W[1] + A[1] * W[0]), (16, A[1] * W[1])):
            v = irfft(spec, n)[:, :L]
            r = np.rint(v)
            assert np.abs(v - r).max(initial=0) < 0.25
            acc += r.astype(np.int64) << sh
        out[s:s + chunk] = acc
    return out


def _divide_closed(M, n, a, Q, R):
    """Division rule on [B][2N-1] reduced a, [B][N+1] Q, R: flag bits per item."""
    B, N1 = Q.shape
    N = N1 - 1
    Pk = np.zeros((B, 2 * N + 1), np.int64)
    Pk[:, :N + 1] += Q + R
    Pk[:, N:] += (M - 1) * Q
    y, ok = modulus_closed(M, n, Pk)
    fl = np.where(ok.all(1), 0, RANGE)
    fl |= np.where((y[:, :2 * N - 1] == a).all(1), 0, EQ)
    fl |= np.where((y[:, 2 * N - 1:] == 0).all(1), 0, TAIL)
    return fl


def _rows(x, n):
    return np.asarray(x, np.int64).reshape(-1, n)


def numpy_encrypt(q, nq, N, r, m, h, quotE, remE):
    x = linear_product(_rows(r, N), _rows(h, N))
    x[:, :N] += _rows(m, N)
    a, ok = modulus_closed(q, nq, x)
    return (np.where(ok.all(1), 0, RANGE) | _divide_closed(q, nq, a, _rows(quotE, N + 1), _rows(remE, N + 1))).astype(np.uint8)


def numpy_inverse(M, n, N, f, fq, quotI, remI):
    a, ok = modulus_closed(M, n, linear_product(_rows(f, N), _rows(fq, N)))
    return (np.where(ok.all(1), 0, RANGE) | _divide_closed(M, n, a, _rows(quotI, N + 1), _rows(remI, N + 1))).astype(np.uint8)


def numpy_decrypt(q, nq, p, np_, N, f, fp, e, quot1, rem1, quot2, rem2):
    fl1 = numpy_inverse(q, nq, N, f, e, quot1, rem1).astype(np.int64)
    R1 = _rows(rem1, N + 1)[:, :N]
    gt, ok_gt = less_than_closed(nq, q // 2, R1)
    b, ok_b = modulus_closed(p, np_, R1 + gt)
    fl2 = np.where((ok_gt & ok_b).all(1), 0, RANGE) | numpy_inverse(p, np_, N, fp, b, quot2, rem2)
    return (fl1 | (fl2 << 3)).astype(np.uint8)


def numpy_check(template, params, arrays):
    """arrays: the template's signals in SIGNALS order, each [B][N] or [B][N+1]."""
    fn = {"VerifyEncrypt": numpy_encrypt, "VerifyDecrypt": numpy_decrypt, "VerifyInverse": numpy_inverse}[template]
    return fn(*params, *arrays)


def stack(template, witnesses):
    """[witness] of one template and one parameter set -> (params, [B][len] int64 arrays in SIGNALS order)."""
    params = list(witnesses[0]["params"])
    return params, [np.array([w["inputs"][name] for w in witnesses], np.int64) for name, _ in SIGNALS[template]]


# ---- the reference-captured witnesses of tests/golden/scheme_*.json ------------------------------------------------------------
def golden_witnesses(load_golden, profiles):
    """{template: [witness]}: every encryptBits / decryptBits / verifyKeysInputs witness the reference recorded."""
    out = {t: [] for t in TEMPLATES}
    for prof in profiles:
        g = load_golden("scheme_%s.json" % prof)
        for key in g["keys"]:
            for case in key["cases"]:
                out["VerifyEncrypt"].append(case["encrypt"])
                out["VerifyDecrypt"].append(case["decrypt"])
            for extra in key.get("sums", []) + key.get("degenerate", []):
                out["VerifyDecrypt"].append(extra["decrypt"])
            for name in ("fq", "fp", "h"):
                out["VerifyInverse"].append(key["verifyKeysInputs"][name])
    return out


def by_params(witnesses):
    """Group witnesses of one template by their params (a batch call takes one parameter set)."""
    groups = {}
    for w in witnesses:
        groups.setdefault(tuple(w["params"]), []).append(w)
    return groups


# ---- honest witnesses from operands (the reference's encryptBits / decryptBits / verifyKeysInputs arithmetic, vectorised) ---------
def split_by_I(c, N, M):
    """dividePolynomials(c, 1 + (M - 1) x^N, M) for reduced [B][2N-1] c -> (quotient, remainder) as [B][N+1] rows (expandArray)."""
    B = c.shape[0]
    hi = np.zeros((B, N), np.int64)
    hi[:, :N - 1] = c[:, N:]
    quot = np.zeros((B, N + 1), np.int64)
    rem = np.zeros((B, N + 1), np.int64)
    quot[:, :N] = (M - hi) % M
    rem[:, :N] = (c[:, :N] + hi) % M
    return quot, rem


def honest_encrypt(q, N, r, m, h):
    r, m, h = _rows(r, N), _rows(m, N), _rows(h, N)
    c = linear_product(r, h)
    c[:, :N] += m
    quot, rem = split_by_I(c % q, N, q)
    return [r, m, h, quot, rem]


def honest_inverse(M, N, f, fq):
    f, fq = _rows(f, N), _rows(fq, N)
    quot, rem = split_by_I(linear_product(f, fq) % M, N, M)
    return [f, fq, quot, rem]


def honest_decrypt(q, p, N, f, fp, e):
    f, fp, e = _rows(f, N), _rows(fp, N), _rows(e, N)
    q1, r1 = split_by_I(linear_product(f, e) % q, N, q)
    b = r1[:, :N]
    b = (b + (b > q // 2)) % p
    q2, r2 = split_by_I(linear_product(fp, b) % p, N, p)
    return [f, fp, e, q1, r1, q2, r2]


def calc_nbits(mod, N):
    """calculateNq / calculateNp (index.js:201-206): ceil(log2(mod^2 N))."""
    v = mod * mod * N
    return (v - 1).bit_length()


def witness(template, params, arrays, i):
    """Item i of stacked arrays as a reference-style {inputs, params} object."""
    return {"params": list(params), "inputs": {name: [int(v) for v in arrays[j][i]] for j, (name, _) in enumerate(SIGNALS[template])}}


def mutations(template, w, rng, count=None):
    """Single-entry changes of witness w: +1, +M, set to 0, set to 65535, at indices 0, 1, N-1, N (the N+1-long signals) and a random
    one of every signal; at most `count` of them, in random order."""
    N, M = w["params"][-1], w["params"][0]
    out = []
    for name, extra in SIGNALS[template]:
        L = N + extra
        for idx in sorted({0, 1, L - 1, int(rng.integers(0, L))}):
            v = w["inputs"][name][idx]
            for nv in (v + 1, v + M, 0, 65535):
                if nv > 65535 or nv == v:
                    continue
                m = {"params": w["params"], "inputs": dict(w["inputs"])}
                m["inputs"][name] = list(w["inputs"][name])
                m["inputs"][name][idx] = nv
                out.append(m)
    rng.shuffle(out)
    return out if count is None else out[:count]
