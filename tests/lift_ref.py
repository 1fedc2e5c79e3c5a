"""Restatement of decryptBits (index.js:111-140) with the lift's addend as a parameter, without the engine: the oracle's decrypt_batch
for quotient1 / remainder1 (they do not depend on the lift), the lift in numpy, the oracle's polymul_split_batch(N, p, fp, b) for
quotient2 / value.  addend 1 is index.js:117 verbatim; (p - q % p) % p is the true centred lift (x - q for x > q/2).
tests/test_lift_cpu.py ties it to the captured decryptBits vectors."""
import numpy as np

from oracle import ntru_oracle as orc

REFERENCE, CENTRED = 0, 1


def addend(q, p, mode):
    return (p - q % p) % p if mode in (CENTRED, "centred") else 1


def lift(rem1, q, p, addend):
    """x > q/2 ? (x + addend) % p : x % p, the threshold strict: x = q/2 is lifted as positive."""
    x = np.asarray(rem1).astype(np.int64)
    return np.where(2 * x > q, (x + addend) % p, x % p).astype(np.uint16)


def decrypt(N, q, p, f, fp, e, mode):
    """(value u8, quot1 u16, rem1 u16, quot2 u8), each [B][N], of decryptBits under the lift `mode` (0 / 1 or the names)."""
    e = np.ascontiguousarray(np.asarray(e, dtype=np.uint16)).reshape(-1, N)
    _, q1, r1, _ = orc.decrypt_batch(N, q, p, f, fp, e)
    b = lift(r1, q, p, addend(q, p, mode))
    fp_rows = np.ascontiguousarray(np.broadcast_to(np.asarray(fp, dtype=np.uint16).reshape(1, N), b.shape))
    q2, value = orc.polymul_split_batch(N, p, fp_rows, b)
    return value.astype(np.uint8), q1, r1, q2.astype(np.uint8)


def decrypt_peritem(N, q, p, f, fp, e, mode):
    """The same with a key per row: f, fp [B][N]."""
    f, fp = np.asarray(f).reshape(-1, N), np.asarray(fp).reshape(-1, N)
    e = np.asarray(e).reshape(-1, N)
    rows = [decrypt(N, q, p, f[i], fp[i], e[i:i + 1], mode) for i in range(e.shape[0])]
    return tuple(np.concatenate([r[k] for r in rows]) for k in range(4))


# ---- a tally with room to count: p = 5 or 7, sums of p - 1 ciphertexts ------------------------------------------------------------------
def cyclic(a, b, N):
    """a (x) b in Z[x] / (x^N - 1) on int64."""
    full = np.convolve(np.asarray(a, np.int64), np.asarray(b, np.int64))
    out = np.zeros(N, np.int64)
    out[:min(N, full.size)] = full[:N]
    out[:full.size - N] += full[N:]
    return out


def tally_case(p, K, G=3, N=167, q=2048, d=5, seed=2024):
    """G groups of K ciphertexts of random bit messages under one key with df = dg = dr = d, drawn from `seed`; f is redrawn until it
    is a unit modulo 2 and p (oracle.ntru_keygen).  r is mapped -1 -> p - 1 as encryptBits does (index.js:89).  Returns a dict with the
    key (f signed, fp, h), the rows e [G K][N], the per-group sums of the plaintexts `counts` [G][N] and the integer polynomials
    T[g] = sum over the group of p (g (x) r_k) + f (x) m_k, of which f (x) sum(e_k) is the residue modulo q: a correct lift recovers
    T, hence counts = fp (x) T mod p, exactly when max |T| < q/2."""
    from oracle import ntru_keygen as kg
    rng = np.random.default_rng(seed)

    def ternary(n1, n2):
        a = np.zeros(N, np.int64)
        perm = rng.permutation(N)
        a[perm[:n1]], a[perm[n1:n1 + n2]] = 1, -1
        return a
    while True:
        f = ternary(d, d - 1)                                        # generatePrivateKeyF: df ones, df - 1 minus ones
        if kg.is_unit(f, N, 2) and kg.is_unit(f, N, p):
            fq, fp = kg.load_private_key(f, N, q, p)
            break
    g = ternary(d, d)
    h = (p * cyclic(fq, g, N)) % q
    assert np.array_equal(cyclic(f, h, N) % q, (p * g) % q)         # f h = p g modulo q
    B = G * K
    m = rng.integers(0, 2, (B, N)).astype(np.int64)
    r = np.array([ternary(d, d) for _ in range(B)])
    r[r == -1] = p - 1
    e = np.array([(cyclic(h, r[b], N) + m[b]) % q for b in range(B)])
    T = np.array([sum(p * cyclic(g, r[b], N) + cyclic(f, m[b], N) for b in range(k * K, (k + 1) * K)) for k in range(G)])
    counts = m.reshape(G, K, N).sum(axis=1)
    return {"N": N, "q": q, "p": p, "K": K, "G": G, "f": f.astype(np.int8), "fp": fp.astype(np.uint8), "h": h.astype(np.uint16),
            "e": e.astype(np.uint16), "counts": counts.astype(np.uint8), "T": T}
