"""One call of each entry point on the operand values where kernels go wrong, with the CPU reference of the same call: the runners
behind tests/test_kernel_variants_gpu.py (every row of tests/kernel_variants.py) and tests/test_valu_geometry_gpu.py (the vector-ALU
families across their lane geometries).  Not a test module.

A runner returns (got, want): the arrays the GPU call wrote and the oracle's, for assert_equal.  The runners of the five vector-ALU
entries (encrypt, decrypt, verify_keys, polymul_split, public_key) take two options: `guard` allocates every output through
Dev.guarded and asserts that the GUARD bytes on either side of it are still FILL after the call; `memo`, a dict the caller keeps,
holds the references by a digest of the call's operands, so that the same operands sent down several kernel paths are computed once."""
import hashlib

import numpy as np

import __graft_entry__ as ge
import ciphertext_sum_ref as sum_ref
import kernel_variants as kv
import keygen_ref
import lift_ref
import message_bytes_ref as bytes_ref
import packed_ref
import peritem_ref
import witness_circuit as wc
from oracle import ntru_keygen as kg
from oracle import ntru_oracle as orc

pkg = ge.load_package()
lift = pkg.lift

WAVES_PER_BLOCK = 4
P3_ONLY = ("k_decrypt_s", "k_decrypt_t", "k_decrypt_m", "k_verify_keys_t", "k_verify_keys_m")
GUARD = 16                       # bytes on either side of a guarded output that must stay FILL
FILL = 0xA5                      # output buffers start as this byte: an element the kernel should write and does not shows up



class Dev:
    """Device buffers of one call, freed on exit.  guard: every out() is a guarded() allocation, for guards_intact()."""

    def __init__(self, eng, guard=False):
        self.eng, self.ptrs, self.guard, self.guards = eng, [], guard, []

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.eng.synchronize()
        for p in self.ptrs:
            self.eng.dev_free(p)

    def up(self, arr, shift=0):
        """arr on the device, `shift` bytes into its allocation."""
        arr = np.ascontiguousarray(arr)
        p = self.eng.dev_alloc(max(arr.nbytes, 16) + shift)
        self.ptrs.append(p)
        if arr.nbytes:
            self.eng.dev_upload(p + shift, arr)
        return p + shift

    def out(self, shape, dtype, shift=0):
        nbytes = int(np.prod(shape)) * np.dtype(dtype).itemsize
        if self.guard:
            self.guards.append((self.guarded(nbytes, shift), nbytes))
            return self.guards[-1][0]
        return self.up(np.full(nbytes, FILL, np.uint8), shift)

    def guarded(self, nbytes, shift=0):
        """nbytes of FILL, `shift` bytes off a 16-byte boundary, with GUARD bytes of FILL on either side; the pointer to the payload."""
        return self.up(np.full(nbytes + 2 * GUARD, FILL, np.uint8), shift) + GUARD

    def get_guarded(self, p, nbytes):
        """[payload, the guard bytes in front, the guard bytes behind]"""
        raw = self.eng.dev_download(p - GUARD, (nbytes + 2 * GUARD,), np.uint8)
        return [raw[GUARD:GUARD + nbytes], raw[:GUARD], raw[GUARD + nbytes:]]

    def get(self, p, shape, dtype):
        return self.eng.dev_download(p, shape, dtype)

    def guards_intact(self, ctx):
        """The GUARD bytes in front of and behind every out() of a guarding Dev are still FILL (nothing to check otherwise)."""
        for i, (p, nbytes) in enumerate(self.guards):
            for side, at in (("in front of", p - GUARD), ("behind", p + nbytes)):
                g = self.eng.dev_download(at, (GUARD,), np.uint8)
                assert (g == FILL).all(), (ctx, "bytes written %s output %d (%d bytes)" % (side, i, nbytes), g.tolist())


def once(memo, what, fn, *operands):
    """fn(), or what `memo` (a dict, or None: no sharing) holds for `what` and these operands (scalars and arrays, by content)."""
    if memo is None:
        return fn()
    h = hashlib.blake2b(repr(what).encode(), digest_size=16)
    for x in operands:
        h.update(np.ascontiguousarray(x).tobytes() if isinstance(x, np.ndarray) else repr(x).encode())
    key = h.digest()
    if key not in memo:
        memo[key] = fn()
    return memo[key]


def ternary(rng, shape, lo=-1):
    return rng.integers(lo, lo + 3, shape)


def items_per_group(kernel, N):
    """Items one wave holds at a time (G) for the vector-ALU families: 64 / ceil(N / 2K)."""
    if "<" not in kernel or kernel.startswith(("k_invert_key", "k_sample", "k_pack", "k_add", "k_polymul_m", "k_product", "k_encrypt_wp")):
        return None
    K = int(kernel.split("<")[1].split(",")[0].rstrip(">"))
    if kernel.startswith(("k_encrypt_t", "k_decrypt_t", "k_verify_keys_t")):
        return 1
    return 64 // (-(-N // (2 * K)))


PERITEM_B = (1, 2, 3, 5)          # PI_WAVES = 2: a lone wave, a full workgroup, a partial last one, an item the grid-stride loop prefetches


def batch_sizes(kernel, shape):
    """B = 1, the row's own B, and the sizes that leave a partial last group / row block."""
    N, B = shape["N"], shape["B"]
    entry = kv.BY_KERNEL[kernel]["entry"]
    if entry in ("encrypt_peritem", "decrypt_peritem"):
        return sorted({B, *PERITEM_B})
    if entry in ("bytes_to_rows", "rows_to_bytes"):
        return sorted({1, 3, B})
    if entry in ("sum_groups", "sum_groups_packed"):
        return [B]                                   # the group layouts are the runner's
    if entry == "decrypt_packed":
        return sorted({1, B})
    if entry.startswith("check_") or entry == "keygen":
        return sorted({1, B})
    out = {1, B}
    G = items_per_group(kernel, N)
    if G:
        out |= {max(G - 1, 1), G + 1, WAVES_PER_BLOCK * G + 1}
    if kernel in ("k_encrypt_m", "k_encrypt_md", "k_decrypt_m", "k_decrypt_mp") or kernel.startswith("k_encrypt_wp"):
        out |= {31, 33}
    if kernel == "k_decrypt_m8":
        out |= {31, 95}                              # 1 and 3 row blocks: the second group of the last workgroup idles
    if kernel in ("k_polymul_m<true>", "k_polymul_m<false>", "k_verify_keys_m") or kernel.startswith("k_product_tern_m"):
        out |= {3, 33}
    if N >= 1024:
        out = {b for b in out if b <= 33}
    return sorted(out)


def rows_cycle(B, makers):
    return np.stack([makers[b % len(makers)](b) for b in range(B)])


# ---- one call of each entry point, compared with the oracle -----------------------------------------------------------------------

def run_encrypt(eng, N, q, B, rng, variant, witness=True, guard=False, memo=None):
    h = [np.full(N, q - 1), rng.integers(0, q, N), np.zeros(N, np.int64)][variant % 3].astype(np.uint16)
    r = rows_cycle(B, [lambda b: np.ones(N), lambda b: np.full(N, 2), lambda b: ternary(rng, N, 0),
                       lambda b: np.zeros(N)]).astype(np.uint8)
    m = rows_cycle(B, [lambda b: np.full(N, 2), lambda b: rng.integers(0, 2, N), lambda b: rng.integers(0, 3, N)]).astype(np.uint8)
    with Dev(eng, guard) as d:
        de, dq = d.out((B, N), np.uint16), (d.out((B, N), np.uint16) if witness else None)
        eng.encrypt_batch_dev(N, q, d.up(h), d.up(r), d.up(m), B, de, dq)
        got = [d.get(de, (B, N), np.uint16)] + ([d.get(dq, (B, N), np.uint16)] if witness else [])
        d.guards_intact(("encrypt", N, q, B, variant))
    e, quot = once(memo, "encrypt", lambda: orc.encrypt_batch(N, q, h, r, m), N, q, h, r, m)
    return got, [e] + ([quot] if witness else [])


def e_rows(rng, N, q, B):
    return rows_cycle(B, [lambda b: np.full(N, q - 1), lambda b: np.zeros(N), lambda b: np.full(N, q // 2),
                          lambda b: np.full(N, q // 2 + 1), lambda b: rng.integers(0, q, N),
                          lambda b: rng.choice([0, q - 1, q // 2, q // 2 + 1], N)]).astype(np.uint16)


def decrypt_key(rng, N, p, variant):
    f = [np.full(N, -1), np.ones(N), ternary(rng, N)][variant % 3].astype(np.int8)
    fp = (np.full(N, p - 1) if variant % 3 < 2 else rng.integers(0, p, N)).astype(np.uint8)
    return f, fp


LIFT_DIFFERED = []               # per call of in_both_lift_modes since the test last cleared it: did the two modes' outputs differ


def in_both_lift_modes(eng, q, p, call, centred_want, ctx, same_in_both=()):
    """call() once in the default mode and once inside lift.using(eng, "centred").  The centred outputs are compared here with
    centred_want() (tests/lift_ref.py); the default outputs are returned for the caller's comparison with the oracle, and the kernel
    must be the same one.  The outputs at the indices `same_in_both` (quotient1, remainder1) do not depend on the lift; where the
    centred addend is 1 nothing does.  Where it is not 1 the two references say which outputs differ, so the byte comparisons hold
    the kernel to it: whether they did goes into LIFT_DIFFERED, and test_variant_row_equals_oracle asserts that every shape with such
    an addend told the modes apart (a single call need not: B = 1 with e = q - 1 and f = -1 has remainder1 = N, below q/2)."""
    got = call()
    kernel = eng.last_kernel()
    with lift.using(eng, "centred"):
        assert lift.get_lift(eng) == 1
        centred = call()
        assert eng.last_kernel() == kernel, (ctx, kernel, eng.last_kernel())
    assert lift.get_lift(eng) == 0, ctx
    assert_equal(centred, centred_want(), (ctx, "centred"))
    for i in same_in_both:
        if i < len(got):
            assert got[i].tobytes() == centred[i].tobytes(), (ctx, "output %d depends on the lift mode" % i)
    differ = any(g.tobytes() != c.tobytes() for g, c in zip(got, centred))
    if lift_ref.addend(q, p, lift_ref.CENTRED) == 1:
        assert not differ, (ctx, "addend 1: the modes must give the same bytes")
    LIFT_DIFFERED.append(differ)
    return got


def run_decrypt(eng, N, q, p, B, rng, variant, witness=True, guard=False, memo=None):
    f, fp = decrypt_key(rng, N, p, variant)
    e = e_rows(rng, N, q, B)
    dts = (np.uint8, np.uint16, np.uint16, np.uint8)

    def call():
        with Dev(eng, guard) as d:
            outs = [d.out((B, N), dt) if witness or i == 0 else None for i, dt in enumerate(dts)]
            eng.decrypt_batch_dev(N, q, p, d.up(f), d.up(fp), d.up(e), B, *outs)
            got = [d.get(o, (B, N), dt) for o, dt in zip(outs, dts) if o]
            d.guards_intact(("decrypt", N, q, p, B, variant))
            return got

    centred = lambda: list(once(memo, "centred", lambda: lift_ref.decrypt(N, q, p, f, fp, e, lift_ref.CENTRED),
                                N, q, p, f, fp, e))[:4 if witness else 1]
    got = in_both_lift_modes(eng, q, p, call, centred, ("decrypt", N, q, p, B, variant), same_in_both=(1, 2))
    want = once(memo, "decrypt", lambda: orc.decrypt_batch(N, q, p, f, fp, e, want_witness=witness), N, q, p, f, fp, e, witness)
    return got, [w for w in want if w is not None]


def run_decrypt_pack(eng, N, q, p, B, rng, variant, fused=True):
    f, fp = decrypt_key(rng, N, p, variant)
    e = e_rows(rng, N, q, B)
    os_ = orc.pack_params(p - 1, N)["outputSize"]

    def call():
        with Dev(eng) as d:
            dv = None if fused else d.out((B, N), np.uint8)
            dp = d.out((B, os_, 4), np.uint64)
            eng.decrypt_pack_batch_dev(N, q, p, d.up(f), d.up(fp), d.up(e), B, dv, dp)
            return [d.get(dp, (B, os_, 4), np.uint64)] + ([] if fused else [d.get(dv, (B, N), np.uint8)])

    def centred():
        value = lift_ref.decrypt(N, q, p, f, fp, e, lift_ref.CENTRED)[0]
        return [orc.pack_batch(p - 1, N, value)] + ([] if fused else [value])

    got = in_both_lift_modes(eng, q, p, call, centred, ("decrypt_pack", N, q, p, B, variant))
    value = orc.decrypt_batch(N, q, p, f, fp, e, want_witness=False)[0]
    return got, [orc.pack_batch(p - 1, N, value)] + ([] if fused else [value])


def run_encrypt_pack(eng, N, q, B, rng, variant):
    h = [np.full(N, q - 1), rng.integers(0, q, N)][variant % 2].astype(np.uint16)
    r = rows_cycle(B, [lambda b: np.full(N, 2), lambda b: np.ones(N), lambda b: ternary(rng, N, 0)]).astype(np.uint8)
    m = rows_cycle(B, [lambda b: np.ones(N), lambda b: rng.integers(0, 2, N)]).astype(np.uint8)
    os_ = orc.pack_params(q - 1, N)["outputSize"]
    with Dev(eng) as d:
        dp = d.out((B, os_, 4), np.uint64)
        eng.encrypt_pack_batch_dev(N, q, d.up(h), d.up(r), d.up(m), B, None, dp)
        got = [d.get(dp, (B, os_, 4), np.uint64)]
    return got, [orc.pack_batch(q - 1, N, orc.encrypt_batch(N, q, h, r, m, want_quot=False)[0])]


def key_pairs(rng, N, q, p, B):
    """Rows of true key pairs (f = +-x^k: fq, fp its inverses, h = p fq g), the same with fq, fp, h or all three corrupted, and the
    shared extremes (f all -1, g all 1, fq and h all q-1, fp all p-1)."""
    f = np.zeros((B, N), np.int64); g = ternary(rng, (B, N)); fq = np.zeros((B, N), np.int64); fp = np.zeros((B, N), np.int64)
    for b in range(B):
        k, s = (3 * b) % N, (1 if b % 2 else -1)
        f[b, k] = s
        fq[b, (N - k) % N] = s % q
        fp[b, (N - k) % N] = s % p
    h = orc.public_key_batch(N, q, p, fq, g).astype(np.int64)
    kind = np.arange(B) % 7
    fq[kind == 1] = (fq[kind == 1] + 1) % q
    fp[kind == 2] = (fp[kind == 2] + 1) % p
    h[kind == 3] = (h[kind == 3] + 1) % q
    for arr, mod in ((fq, q), (fp, p), (h, q)):
        arr[kind == 4] = (arr[kind == 4] + 1) % mod
    f[kind == 5], g[kind == 5], fq[kind == 5], fp[kind == 5], h[kind == 5] = -1, 1, q - 1, p - 1, q - 1
    f[kind == 6], g[kind == 6] = ternary(rng, (np.sum(kind == 6), N)), -1
    fq[kind == 6], fp[kind == 6], h[kind == 6] = (rng.integers(0, q, (np.sum(kind == 6), N)), rng.integers(0, p, (np.sum(kind == 6), N)),
                                                  rng.integers(0, q, (np.sum(kind == 6), N)))
    return (f.astype(np.int8), g.astype(np.int8), fq.astype(np.uint16), fp.astype(np.uint8), h.astype(np.uint16))


VK_OUT = (("quot_fq", np.uint16), ("rem_fq", np.uint16), ("quot_fp", np.uint8), ("rem_fp", np.uint8), ("quot_h", np.uint16),
          ("rem_h", np.uint16))


def run_verify_keys(eng, N, q, p, B, rng, variant, guard=False, memo=None):
    ins = key_pairs(rng, N, q, p, B)
    with Dev(eng, guard) as d:
        outs = [d.out((B, N), dt) for _, dt in VK_OUT] + [d.out((B,), np.uint8)]
        eng.verify_keys_batch_dev(N, q, p, *[d.up(x) for x in ins], B, *outs)
        got = [d.get(o, (B, N), dt) for o, (_, dt) in zip(outs, VK_OUT)] + [d.get(outs[-1], (B,), np.uint8)]
        d.guards_intact(("verify_keys", N, q, p, B, variant))
    want = once(memo, "verify_keys", lambda: orc.verify_keys_batch(N, q, p, *ins), N, q, p, *ins)
    if B >= 7:
        flags = want["flags"]
        assert flags[0] == 0 and flags[1] & 1 and flags[2] & 2 and flags[3] & 4 and flags[4] == 7, flags[:7]
    return got, [want[k] for k, _ in VK_OUT] + [want["flags"]]


def run_polymul_split(eng, N, mod, B, rng, variant, guard=False, memo=None):
    a = rows_cycle(B, [lambda b: np.full(N, mod - 1), lambda b: rng.integers(0, mod, N)]).astype(np.uint16)
    b_ = rows_cycle(B, [lambda b: np.full(N, mod - 1), lambda b: rng.integers(0, mod, N), lambda b: np.ones(N)]).astype(np.uint16)
    if variant % 2:
        a, b_ = b_, a
    with Dev(eng, guard) as d:
        dq, dr = d.out((B, N), np.uint16), d.out((B, N), np.uint16)
        eng.polymul_split_dev(N, mod, d.up(a), d.up(b_), B, dq, dr)
        got = [d.get(dq, (B, N), np.uint16), d.get(dr, (B, N), np.uint16)]
        d.guards_intact(("polymul_split", N, mod, B, variant))
    return got, list(once(memo, "polymul_split", lambda: orc.polymul_split_batch(N, mod, a, b_), N, mod, a, b_))


def run_public_key(eng, N, q, p, B, rng, variant, guard=False, memo=None):
    fq = rows_cycle(B, [lambda b: np.full(N, q - 1), lambda b: rng.integers(0, q, N)]).astype(np.uint16)
    g = rows_cycle(B, [lambda b: [np.ones(N), np.full(N, -1), ternary(rng, N)][(b + variant) % 3]]).astype(np.int8)
    with Dev(eng, guard) as d:
        dh = d.out((B, N), np.uint16)
        eng.public_key_batch_dev(N, q, p, d.up(fq), d.up(g), B, dh)
        got = [d.get(dh, (B, N), np.uint16)]
        d.guards_intact(("public_key", N, q, p, B, variant))
    return got, [once(memo, "public_key", lambda: orc.public_key_batch(N, q, p, fq, g), N, q, p, fq, g)]


def run_invert_key(eng, N, q, p, B, rng, variant):
    """Inverses are unique: a unit's row must satisfy fq f = 1 (mod q) and fp f = 1 (mod 3); a flagged row must be a non-unit and
    zero."""
    f = rows_cycle(B, [lambda b: ternary(rng, N), lambda b: np.ones(N), lambda b: np.eye(1, N, b % N)[0]]).astype(np.int8)
    with Dev(eng) as d:
        dq, dp, dfl = d.out((B, N), np.uint16), d.out((B, N), np.uint8), d.out((B,), np.uint8)
        eng.invert_key_batch_dev(N, q, p, d.up(f), B, dq, dp, dfl)
        fq, fp, flags = d.get(dq, (B, N), np.uint16), d.get(dp, (B, N), np.uint8), d.get(dfl, (B,), np.uint8)
    one = np.eye(1, N, 0, dtype=np.uint16)[0]
    for b in range(B):
        assert int(flags[b]) & ~24 == 0, flags[b]
        if b % 3 == 1:                                        # f = 1 + x + ... + x^(N-1) is a zero divisor modulo 2 and 3
            assert flags[b] == 24 and not fq[b].any() and not fp[b].any(), (b, flags[b])
            continue
        for bit, inv, mod, prime in ((8, fq[b], q, 2), (16, fp[b], p, p)):
            if flags[b] & bit:
                assert not inv.any() and not kg.is_unit(f[b], N, prime), (b, bit)
            else:
                rem = orc.polymul_split_batch(N, mod, inv.astype(np.uint16), (f[b].astype(np.int64) % mod).astype(np.uint16))[1][0]
                assert np.array_equal(rem, one), (b, mod)
    return [], []


def run_sample_ternary(eng, N, rounds, B, rng, variant):
    key = rng.integers(0, 1 << 32, 8, dtype=np.uint64).astype(np.uint32)
    n1, n2 = [(N // 3, N // 3), (N, 0), (0, N)][variant % 3]
    eng.set_sampler_rounds(rounds)
    try:
        with Dev(eng) as d:
            do = d.out((B, N), np.uint8)
            eng.sample_ternary_dev(N, n1, n2, 2, key, 5 + variant, B, do)
            got = [d.get(do, (B, N), np.uint8)]
    finally:
        eng.set_sampler_rounds(20)
    return got, [orc.sample_ternary_batch(N, n1, n2, 2, key, 5 + variant, B, rounds)]


def run_pack(eng, N, max_val, B, rng, variant, dtype):
    data = rows_cycle(B, [lambda b: np.full(N, max_val), lambda b: rng.integers(0, max_val + 1, N)]).astype(dtype)
    os_ = orc.pack_params(max_val, N)["outputSize"]
    with Dev(eng) as d:
        dp = d.out((B, os_, 4), np.uint64)
        fn = eng._lib.ntru_pack_bytes_batch_dev if dtype == np.uint8 else eng._lib.ntru_pack_batch_dev
        eng._chk(fn(eng._h, max_val, N, eng._dp(d.up(data)), B, eng._dp(dp)))
        got = [d.get(dp, (B, os_, 4), np.uint64)]
    return got, [orc.pack_batch(max_val, N, data)]


def run_unpack(eng, S, max_val, B, rng, variant):
    bits = max_val.bit_length()
    per = 252 // bits
    vals = rows_cycle(B, [lambda b: np.full(S * per, max_val), lambda b: rng.integers(0, max_val + 1, S * per)])
    limbs = orc.pack_batch(max_val, S * per, vals)[:, :S]
    with Dev(eng) as d:
        do = d.out((B, S * per), np.uint16)
        eng._chk(eng._lib.ntru_unpack_batch_dev(eng._h, max_val, 252, eng._dp(d.up(limbs)), S, B, eng._dp(do)))
        got = [d.get(do, (B, S * per), np.uint16)]
    return got, [orc.unpack_batch(max_val, 252, limbs)]


def run_add(eng, N, mod, B, rng, variant):
    a = rows_cycle(B, [lambda b: np.full(N, mod - 1), lambda b: rng.integers(0, mod, N)]).astype(np.uint16)
    b_ = rows_cycle(B, [lambda b: np.full(N, mod - 1), lambda b: rng.integers(0, mod, N)]).astype(np.uint16)
    with Dev(eng) as d:
        do = d.out((B, N), np.uint16)
        eng.add_batch_dev(N, mod, d.up(a), d.up(b_), B, do)
        got = [d.get(do, (B, N), np.uint16)]
    return got, [((a.astype(np.int64) + b_) % mod).astype(np.uint16)]


def run_split_by_I(eng, N, mod, B, rng, variant):
    a = rows_cycle(B, [lambda b: np.full(2 * N, mod - 1), lambda b: rng.integers(0, mod, 2 * N)]).astype(np.uint16)
    with Dev(eng) as d:
        dq, dr = d.out((B, N), np.uint16), d.out((B, N), np.uint16)
        eng.split_by_I_dev(N, mod, d.up(a), B, dq, dr)
        got = [d.get(dq, (B, N), np.uint16), d.get(dr, (B, N), np.uint16)]
    lo, hi = a[:, :N].astype(np.int64), a[:, N:].astype(np.int64)
    return got, [((mod - hi) % mod).astype(np.uint16), ((lo + hi) % mod).astype(np.uint16)]


def run_generic_multiply(eng, N, mod, B, rng, variant):
    a = rows_cycle(B, [lambda b: np.full(N, mod - 1), lambda b: rng.integers(-(1 << 26), 1 << 26, N)])
    b_ = rows_cycle(B, [lambda b: np.full(N, -(1 << 26)), lambda b: rng.integers(0, mod, N)])
    got = eng.generic_multiply(a, b_, mod)
    return [got], [[kg._multiply(a[i], b_[i], mod).tolist() for i in range(B)]]



# ---- the five newer kernel files ------------------------------------------------------------------------------------------------------

def run_encrypt_peritem(eng, N, q, B, rng, variant):
    h, r, m = peritem_ref.encrypt_operands(rng, N, q, B, variant)
    witness = variant != 1
    with Dev(eng) as d:
        de, dq = d.out((B, N), np.uint16), (d.out((B, N), np.uint16) if witness else None)
        eng.encrypt_peritem_batch_dev(N, q, d.up(h), d.up(r), d.up(m), B, de, dq)
        got = [d.get(de, (B, N), np.uint16)] + ([d.get(dq, (B, N), np.uint16)] if witness else [])
    e, quot = peritem_ref.oracle_encrypt(N, q, h, r, m)
    return got, [e] + ([quot] if witness else [])


PI_OUT = (np.uint8, np.uint16, np.uint16, np.uint8)           # value, quot1, rem1, quot2


def decrypt_peritem_call(eng, N, q, p, f, fp, e, witness=True):
    B = f.shape[0]
    with Dev(eng) as d:
        outs = [d.out((B, N), dt) for dt in PI_OUT]
        if not witness:
            outs[1:] = [None] * 3
        eng.decrypt_peritem_batch_dev(N, q, p, d.up(f), d.up(fp), d.up(e), B, *outs)
        return [d.get(o, (B, N), dt) for o, dt in zip(outs, PI_OUT) if o]


def run_decrypt_peritem(eng, N, q, p, B, rng, variant):
    f, fp, e = peritem_ref.decrypt_operands(rng, N, q, p, B, variant)
    witness = variant != 1
    want = peritem_ref.oracle_decrypt(N, q, p, f, fp, e)
    peritem_ref.assert_lift_edges_met(N, q, f, want[2])
    centred = lambda: list(lift_ref.decrypt_peritem(N, q, p, f, fp, e, lift_ref.CENTRED))[:4 if witness else 1]
    got = in_both_lift_modes(eng, q, p, lambda: decrypt_peritem_call(eng, N, q, p, f, fp, e, witness), centred,
                             ("decrypt_peritem", N, q, p, B, variant), same_in_both=(1, 2))
    return got, list(want if witness else want[:1])


def csr_offsets(B):
    """Empty groups first, last and in the middle, a single row, one group over most of the rows; rows behind the last offset."""
    a, b = min(5, B // 2), B - min(2, B // 3)
    return np.array([0, 0, a, a, a, min(a + 1, b), b, b], np.int64)


def run_sum_groups(eng, N, mod, B, rng, variant, extra):
    """The row's own layout, uniform groups of K = 1, 3, 40 (one group and two), and the offsets form with empty groups; variant:
    the weights (all mod - 1, zero, random) and, at 2, every row and output pointer 2 bytes off 4-byte alignment."""
    weighted = extra.get("weights", variant != 1)
    layouts = [(B, extra.get("K"), csr_offsets(B) if extra.get("csr") else None)]
    layouts += [(K * G, K, None) for K in (1, 3, 40) for G in (1, 2)] + [(47, None, csr_offsets(47))]
    shift = 2 if variant == 2 else 0
    got, want = [], []
    for nrows, K, off in layouts:
        rows = peritem_ref.rows_cycle(nrows + variant, [lambda b: np.full(N, mod - 1), lambda b: rng.integers(0, mod, N)])[variant:]
        rows = rows.astype(np.uint16)
        w = None
        if weighted:
            w = [np.full(nrows, mod - 1), np.zeros(nrows), rng.integers(0, mod, nrows)][variant].astype(np.uint16)
        G = nrows // K if off is None else len(off) - 1
        with Dev(eng) as d:
            do = d.out((G, N), np.uint16, shift)
            eng.sum_groups_dev(N, mod, d.up(rows, shift), do, G, d_offsets=None if off is None else d.up(off), K=K,
                               d_weights=None if w is None else d.up(w, shift))
            got.append(d.get(do, (G, N), np.uint16))
        assert eng.last_kernel() == "k_sum_groups<%d,%d>" % (mod & (mod - 1) == 0, weighted), eng.last_kernel()
        want.append(sum_ref.np_sum(rows, mod, offsets=off, K=K, weights=w).astype(np.uint16))
    return got, want


# ---- packed ciphertexts (packed_ciphertexts.hip) -----------------------------------------------------------------------------------------

_packed_pool = {}                 # (bits, N) -> (rows, packed) of the width last used: shared by the rows and moduli of that width
_packed_want = {}                 # the unweighted reference sums of the large launch: they do not depend on the variant


def packed_pool(bits, N, nrows):
    """nrows raw rows and their packed form with every ignored bit set.  Row 0 is all ones, the others are random fields below 2^bits
    (not below mod).  The dense rows are packed_ref.unpack_rows of the packed ones, unpacked once: np_sum_packed is np_sum on them."""
    if (bits, N) not in _packed_pool or len(_packed_pool[bits, N][0]) < nrows:
        for k in [k for k in _packed_pool if k[0] != bits]:
            del _packed_pool[k]
        for k in [k for k in _packed_want if k[0] != bits]:
            del _packed_want[k]
        rng = np.random.default_rng(1000 * bits + N)
        rows = rng.integers(0, 1 << bits, (nrows, N), dtype=np.uint16)
        rows[0] = (1 << bits) - 1
        mod = 1 << bits                                  # the format depends on the width alone
        packed = packed_ref.set_ignored_bits(mod, N, packed_ref.pack_rows(mod, rows))
        assert np.array_equal(packed_ref.unpack_rows(mod, N, packed), rows)
        assert packed_ref.params(mod - 1, N)[0] == bits
        _packed_pool[bits, N] = (rows, packed)
    return _packed_pool[bits, N]


def run_sum_groups_packed(eng, N, mod, rng, variant, extra):
    """k_sum_groups_packed against packed_ref.np_sum_packed, bit for bit.  The small layouts of run_sum_groups (one row per block:
    k_sum_groups_finish does the adding) and one launch with many rows per block (many_rows_per_block).  variant: the weights (all
    mod - 1, zero, random) and, at 2, the packed base 8 bytes off 16-byte alignment, weights and output 2 bytes off 4-byte alignment."""
    bits = (mod - 1).bit_length()
    lay = kv.packed_layout(bits, N)
    assert lay["layout"] == extra["layout"], (lay, extra)
    weighted = extra["weights"]
    pow2 = mod & (mod - 1) == 0
    import torch
    first, T, R, Pb, big_off = kv.many_rows_per_block(bits, N, torch.cuda.get_device_properties(0).multi_processor_count)
    side = lay["side"]
    # sized from this card's CU count: were the launch cut into more blocks than assumed, every block would hold one row again
    assert -(-T // Pb) == R and R > kv.SP_BATCH * side + side, (T, Pb, R, side)
    rows, packed = packed_pool(bits, N, first + T + 2)                      # two rows behind the last offset
    layouts = [(K * G, K, None) for K in (1, 3, 40) for G in (1, 2)] + [(47, None, csr_offsets(47)), (first + T + 2, None, big_off)]
    shift = 2 if variant == 2 else 0
    got, want = [], []
    for nrows, K, off in layouts:
        w = None
        if weighted:
            w = [np.full(nrows, mod - 1), np.zeros(nrows), rng.integers(0, mod, nrows)][variant].astype(np.uint16)
        G = nrows // K if off is None else len(off) - 1
        with Dev(eng) as d:
            do = d.out((G, N), np.uint16, shift)
            pkg.sum_groups_packed_dev(eng, N, mod, d.up(packed[:nrows], 8 if variant == 2 else 0), do, G,
                                      d_offsets=None if off is None else d.up(off), K=K, d_weights=None if w is None else d.up(w, shift))
            got.append(d.get(do, (G, N), np.uint16))
        assert eng.last_kernel() == "k_sum_groups_packed<%d,%d,%d>" % (bits, pow2, weighted), eng.last_kernel()
        key = (bits, N, mod)
        if off is big_off and w is None and key in _packed_want:
            want.append(_packed_want[key])
            continue
        want.append(sum_ref.np_sum(rows[:nrows], mod, offsets=off, K=K, weights=w).astype(np.uint16))
        if off is big_off and w is None:
            _packed_want[key] = want[-1]
    return got, want


def run_decrypt_packed(eng, N, q, p, B, rng, variant):
    """k_unpack_rows through ntru_decrypt_packed_batch_dev: packed rows of raw fields with every ignored bit set, against the oracle's
    decrypt of packed_ref.unpack_rows; the four outputs, and at variant 1 the value alone."""
    witness = variant != 1
    f, fp = decrypt_key(rng, N, p, variant)
    e = rows_cycle(B, [lambda b: np.full(N, q - 1), lambda b: rng.integers(0, q, N), lambda b: np.zeros(N)]).astype(np.uint16)
    packed = packed_ref.set_ignored_bits(q, N, packed_ref.pack_rows(q, e))
    assert not np.array_equal(packed, packed_ref.pack_rows(q, e))
    dense = packed_ref.unpack_rows(q, N, packed)
    assert np.array_equal(dense, e)
    dts = (np.uint8, np.uint16, np.uint16, np.uint8)
    with Dev(eng) as d:
        outs = [d.out((B, N), dt) for dt in dts]
        if not witness:
            outs[1:] = [None] * 3
        pkg.decrypt_packed_batch_dev(eng, N, q, p, d.up(f), d.up(fp), d.up(packed), B, *outs)
        got = [d.get(o, (B, N), dt) for o, dt in zip(outs, dts) if o]
    want = orc.decrypt_batch(N, q, p, f, fp, dense, want_witness=witness)
    return got, [w for w in want if w is not None]


def message_bytes(rng, nbytes, B):
    return peritem_ref.rows_cycle(B, [lambda b: np.full(nbytes, 0x00), lambda b: np.full(nbytes, 0xFF), lambda b: np.full(nbytes, 0x80),
                                      lambda b: np.full(nbytes, 0x01), lambda b: rng.integers(0, 256, nbytes)]).astype(np.uint8)


BYTE_SHIFTS = (0, 1, 15)          # the output pointer's offset from a 16-byte boundary, by variant
GUARDS = [np.full(GUARD, FILL, np.uint8)] * 2


def run_bytes_to_rows(eng, N, nbytes, B, rng, variant):
    data = np.roll(message_bytes(rng, nbytes, B + variant), -variant, axis=0)[:B]
    with Dev(eng) as d:
        out = d.guarded(B * N, BYTE_SHIFTS[variant])
        eng.bytes_to_rows_dev(N, nbytes, d.up(data, variant), B, out)
        got = d.get_guarded(out, B * N)
    return got, [bytes_ref.np_bytes_to_rows(data, N).reshape(-1)] + GUARDS


def run_rows_to_bytes(eng, N, nbytes, B, rng, variant):
    """Rows of bits; at variant 2 a 2 in the first message coefficient of row 0 and, where the row has a pad, a 1 in the last
    coefficient of the last row (both flagged); at variant 1 without the flags array."""
    rows = bytes_ref.np_bytes_to_rows(np.roll(message_bytes(rng, nbytes, B + variant), -variant, axis=0)[:B], N)
    if variant == 2:
        rows[0, 0] = 2
        if 8 * nbytes < N:
            rows[B - 1, N - 1] = 1
    want, want_flags = bytes_ref.np_rows_to_bytes(rows, nbytes)
    if variant == 2:
        assert want_flags[0] & bytes_ref.FLAG_NOT_BITS and (8 * nbytes == N or want_flags[B - 1] & bytes_ref.FLAG_PAD_NONZERO)
    with Dev(eng) as d:
        out = d.guarded(B * nbytes, BYTE_SHIFTS[variant])
        fl = None if variant == 1 else d.guarded(B, BYTE_SHIFTS[variant])
        eng.rows_to_bytes_dev(N, nbytes, d.up(rows, variant), B, out, fl)
        got = d.get_guarded(out, B * nbytes) + (d.get_guarded(fl, B) if fl else [])
    return got, [want.reshape(-1)] + GUARDS + ([want_flags] + GUARDS if variant != 1 else [])


CHECK_TEMPLATE = {"check_encrypt": "VerifyEncrypt", "check_decrypt": "VerifyDecrypt", "check_inverse": "VerifyInverse"}


def run_check(eng, entry, N, q, p, B, rng, variant):
    """B accepted witnesses (operands at their extremes in item 0 of variant 0), then item 0 again with a single coefficient off by
    one: at index 0 and at the last index of each array in turn.  Flags against the closed-form evaluator."""
    template = CHECK_TEMPLATE[entry]
    nq, np_ = wc.calc_nbits(q, N), wc.calc_nbits(p, N)
    tern = lambda: rng.choice([0, 1, q - 1], (B, N))
    if entry == "check_encrypt":
        params, r, m, h = (q, nq, N), rng.integers(0, 3, (B, N)), rng.integers(0, 3, (B, N)), rng.integers(0, q, (B, N))
        r[0, 0], h[0, 0] = 1, 1                                   # item 0 is mutated below: no operand row of it is zero
        if variant == 0:
            r[0], m[0], h[0] = 2, 2, q - 1
        arrays = wc.honest_encrypt(q, N, r, m, h)
    elif entry == "check_decrypt":
        params, f, fp, e = (q, nq, p, np_, N), tern(), rng.integers(0, p, (B, N)), rng.integers(0, q, (B, N))
        f[0, 0], fp[0, 0], e[0, 0] = 1, 1, 1
        if variant == 0:
            f[0], fp[0], e[0] = q - 1, p - 1, q - 1
        arrays = wc.honest_decrypt(q, p, N, f, fp, e)
    else:
        params, f, fq = (q, nq, N), tern(), rng.integers(0, q, (B, N))
        f[0, 0], fq[0, 0] = 1, 1
        if variant == 0:
            f[0], fq[0] = q - 1, q - 1
        arrays = wc.honest_inverse(q, N, f, fq)
    arrays = [np.asarray(a, np.int64) for a in arrays]
    spots = [(j, idx) for j, a in enumerate(arrays) for idx in (0, a.shape[1] - 1)]
    arrays = [np.concatenate([a, np.repeat(a[:1], len(spots), axis=0)]) for a in arrays]
    for k, (j, idx) in enumerate(spots):
        arrays[j][B + k, idx] += 1
    total = B + len(spots)
    want = wc.numpy_check(template, params, arrays)
    assert not want[:B].any() and want[B:].any(), (entry, want.tolist())            # accepted witnesses, then flagged ones
    with Dev(eng) as d:
        fl = d.out((total,), np.uint8)
        ptrs = [d.up(a.astype(np.uint16)) for a in arrays]
        if entry == "check_encrypt":
            eng.check_encrypt_batch_dev(N, q, nq, *ptrs, total, fl)
        elif entry == "check_decrypt":
            eng.check_decrypt_batch_dev(N, q, nq, p, np_, *ptrs, total, fl)
        else:
            eng.check_inverse_batch_dev(N, q, nq, *ptrs, total, fl)
        got = [d.get(fl, (total,), np.uint8)]
    return got, [want]


KEYGEN_KEY = np.array([0x9E3779B9 * (i + 1) & 0xFFFFFFFF for i in range(8)], np.uint32)
KEYGEN_OUT = (("f", np.int8), ("g", np.int8), ("fq", np.uint16), ("fp", np.uint8), ("h", np.uint16))
_keygen_want = {}                 # the CPU replay of a call, computed once and shared by the four rows


def run_keygen(eng, N, q, B, rng, variant, extra):
    df, dg = extra["df"], extra["dg"]
    first = extra["first"] - variant
    args = (N, q, df, dg, first, B)
    if args not in _keygen_want:
        _keygen_want[args] = keygen_ref.key_pairs(N, q, df, dg, KEYGEN_KEY, first, B, 100)
    want = _keygen_want[args]
    if B > 1:
        assert (want["tries"] > 1).any() and not want["flags"].any(), args       # the call does redraw, and every item ends as a unit
    with Dev(eng) as d:
        outs = [d.out((B, N), dt) for _, dt in KEYGEN_OUT] + [d.out((B,), np.uint8), d.out((B,), np.uint8)]
        work = d.out((eng.keygen_workspace_bytes(N, B),), np.uint8)
        eng.keygen_batch_dev(N, q, 3, df, dg, KEYGEN_KEY, first, 100, B, work, *outs)
        got = [d.get(o, (B, N), dt) for o, (_, dt) in zip(outs, KEYGEN_OUT)] + [d.get(o, (B,), np.uint8) for o in outs[5:]]
    return got, [want[k] for k, _ in KEYGEN_OUT] + [want["tries"], want["flags"]]


def run_shape(eng, entry, s, B, rng, variant):
    N, q, p = s["N"], s["q"], s["p"]
    if entry == "encrypt_peritem":
        return run_encrypt_peritem(eng, N, q, B, rng, variant)
    if entry == "decrypt_peritem":
        return run_decrypt_peritem(eng, N, q, p, B, rng, variant)
    if entry == "sum_groups":
        return run_sum_groups(eng, N, q, B, rng, variant, s["extra"])
    if entry == "sum_groups_packed":
        return run_sum_groups_packed(eng, N, q, rng, variant, s["extra"])
    if entry == "decrypt_packed":
        return run_decrypt_packed(eng, N, q, p, B, rng, variant)
    if entry == "bytes_to_rows":
        return run_bytes_to_rows(eng, N, s["extra"]["nbytes"], B, rng, variant)
    if entry == "rows_to_bytes":
        return run_rows_to_bytes(eng, N, s["extra"]["nbytes"], B, rng, variant)
    if entry in CHECK_TEMPLATE:
        return run_check(eng, entry, N, q, p, B, rng, variant)
    if entry == "keygen":
        return run_keygen(eng, N, q, B, rng, variant, s["extra"])
    if entry == "encrypt":
        return run_encrypt(eng, N, q, B, rng, variant, witness=variant != 1)
    if entry == "decrypt":
        return run_decrypt(eng, N, q, p, B, rng, variant, witness=variant != 1)
    if entry == "decrypt_pack":
        return run_decrypt_pack(eng, N, q, p, B, rng, variant, fused=variant != 1)
    if entry == "encrypt_pack":
        return run_encrypt_pack(eng, N, q, B, rng, variant)
    if entry == "verify_keys":
        return run_verify_keys(eng, N, q, p, B, rng, variant)
    if entry == "polymul_split":
        return run_polymul_split(eng, N, q, B, rng, variant)
    if entry == "public_key":
        return run_public_key(eng, N, q, p, B, rng, variant)
    if entry == "invert_key":
        return run_invert_key(eng, N, q, p, B, rng, variant)
    if entry == "sample_ternary":
        return run_sample_ternary(eng, N, p, B, rng, variant)
    if entry in ("pack", "pack_bytes"):
        return run_pack(eng, N, q, B, rng, variant, np.uint8 if entry == "pack_bytes" else np.uint16)
    if entry == "unpack":
        return run_unpack(eng, N, q, B, rng, variant)
    if entry == "add":
        return run_add(eng, N, q, B, rng, variant)
    if entry == "split_by_I":
        return run_split_by_I(eng, N, q, B, rng, variant)
    if entry == "generic_multiply":
        return run_generic_multiply(eng, N, q, B, rng, variant)
    raise AssertionError("no runner for " + entry)


def assert_equal(got, want, ctx):
    assert len(got) == len(want), ctx
    for i, (g, w) in enumerate(zip(got, want)):
        if isinstance(w, list):
            assert g == w, (ctx, i)
            continue
        bad = np.argwhere(np.asarray(g) != np.asarray(w))
        assert bad.size == 0, (ctx, "output %d" % i, "first differing index", bad[0].tolist(), np.asarray(g)[tuple(bad[0])],
                               np.asarray(w)[tuple(bad[0])], "differing", len(bad))
