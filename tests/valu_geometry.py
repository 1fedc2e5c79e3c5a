"""The launch geometry of the vector-ALU families (csrc/valu_families.hip), which kernel their launchers pick, and the N at which that
geometry changes.

Plain data, imported by tests/test_valu_geometry_cpu.py (the restatement against the variant table, the sweep's coverage and size),
tests/test_valu_geometry_gpu.py (every output of the sweep against the oracle) and the dispatch sweep of
tests/test_kernel_variants_gpu.py.  Not a test module.

A Python restatement of the host side of valu_families.hip (pick_K, make_geom, add_path_me, shared_path_K, the dot8 condition) and of
the order in which abi.hip and the launchers try the families:
  an item is owned by nl = ceil(N / 2K) lanes, K the smallest odd K with nl <= 64; G = 64 // nl items share a wave; the last lane of an
  item holds N - 2K (nl - 1) coefficients, between 1 and 2K; lanes at or beyond G nl idle.
  encrypt      the matrix cores (kernel path 0, q <= 8192, 64 <= N <= 1024); else k_encrypt_t<K,ME> where add_path_me gives a mask
               interval; else k_encrypt<K>
  decrypt      the matrix cores (as encrypt, p == 3); else k_decrypt_s[+dot8]<K,ME> where shared_path_K gives a K; else, at kernel path
               2 and p == 3, k_decrypt_t<K,ME> where add_path_me gives an interval; else k_decrypt<K>
  verify_keys  the per-item matrix kernels (kernel path 0, p == 3, q <= 8192, 128 <= N <= 1024); else, at p == 3, k_verify_keys_t<K,ME>
               where add_path_me gives an interval; else k_verify_keys<K>
  polymul_split, public_key   the per-item matrix kernels (kernel path 0, a power of two <= 8192, 128 <= N <= 1024); else
               k_polymul_split<K>, k_public_key<K>
"""
import kernel_variants as kv

ENTRIES = ("encrypt", "decrypt", "verify_keys", "polymul_split", "public_key")
QS = (2048, 8192, 16384, 32768, 65536)
PATHS = (0, 1, 2, 3)
MAXN = 1920


# ---- the host-side selection --------------------------------------------------------------------------------------------------------

def pick_K(N):
    for K in range(1, 16, 2):
        if -(-N // (2 * K)) <= 64:
            return K
    raise ValueError("N = %d is beyond the families' range" % N)


def geom(N, K=None):
    """(K, nl, G) of make_geom(N, K); K = pick_K(N) unless given (the shared stepping brings its own)."""
    K = K or pick_K(N)
    nl = -(-N // (2 * K))
    return K, nl, 64 // nl


def last_lane_fill(N, K=None):
    """Coefficients the item's last lane holds: 1 .. 2K."""
    K, nl, _ = geom(N, K)
    return N - 2 * K * (nl - 1)


def add_path_me(N, q, path):
    """The mask interval of the per-item add path (2K or K), or 0: one item per wave, K <= 7, ME values below q on a masked field."""
    if path == 1:
        return 0
    K, nl, G = geom(N)
    if K > 7 or G != 1:
        return 0
    limit = 65535 // (q - 1) - 1
    return 2 * K if limit >= 2 * K else (K if limit >= K else 0)


def shared_path(N, q, p, path):
    """(K, ME, dot8) of the shared stepping, or None: odd N, K = ceil(N / 64) made odd in 9..13, ME = K or 7 (not at K = 13); the dot8
    second product where the item takes 32 lanes, K >= 11, not at kernel path 3."""
    if path == 1 or p != 3 or N % 2 == 0:
        return None
    K = (N + 63) // 64
    K += 1 - K % 2
    if K < 9 or K > 13 or 4 * N >= 65536:
        return None
    limit = 65535 // (q - 1) - 1
    if limit >= K:
        me = K
    elif limit >= 7 and K != 13:
        me = 7
    else:
        return None
    return K, me, geom(N, K)[1] == 32 and K >= 11 and path != 3


def matrix_may_apply(entry, N, q, p, path):
    """Whether abi.hip may hand the call to a matrix-core kernel (which can still decline: its LDS budget).  Kernel paths 1-3 force the
    vector-ALU families; 4 and 5 are not this module's."""
    if path != 0 or q > 8192 or q & (q - 1) or N > 1024:
        return False
    if entry == "encrypt":
        return N >= 64
    if entry == "decrypt":
        return N >= 64 and p == 3
    if entry == "verify_keys":
        return N >= 128 and p == 3
    return N >= 128                                             # polymul_split (q is its modulus), public_key


def accepted(entry, N, q, p):
    """The ABI's documented parameter rules, for the moduli this module uses (q a power of two <= 65536, or polymul_split's 3)."""
    if not 2 <= N <= MAXN:
        return False
    if entry in ("decrypt", "verify_keys") and (p & (p - 1) == 0 or N * (p - 1) ** 2 >= 65536):
        return False
    if entry in ("verify_keys", "public_key") and p * (q - 1) > 65535:
        return False
    if entry == "polymul_split" and q & (q - 1):
        return N * (q - 1) ** 2 < 65536
    return True


def expected_last(entry, N, q, p, path):
    """What ntru_engine_last_kernel() returns after `entry` at kernel path 0-3; None where a matrix-core kernel may take the call."""
    assert entry in ENTRIES and path in PATHS, (entry, path)
    if matrix_may_apply(entry, N, q, p, path):
        return None
    K = pick_K(N)
    if entry == "encrypt":
        me = add_path_me(N, q, path)
        return "k_encrypt_t<%d,%d>" % (K, me) if me else "k_encrypt<%d>" % K
    if entry == "decrypt":
        s = shared_path(N, q, p, path)
        if s:
            return "k_decrypt_s%s<%d,%d>" % ("+dot8" if s[2] else "", s[0], s[1])
        me = add_path_me(N, q, path) if p == 3 and path == 2 else 0
        return "k_decrypt_t<%d,%d>" % (K, me) if me else "k_decrypt<%d>" % K
    if entry == "verify_keys":
        me = add_path_me(N, q, path) if p == 3 else 0
        return "k_verify_keys_t<%d,%d>" % (K, me) if me else "k_verify_keys<%d>" % K
    return ("k_polymul_split<%d>" if entry == "polymul_split" else "k_public_key<%d>") % K


def kernel_tuple(last):
    """("k_decrypt_s+dot8", 11, 7) of "k_decrypt_s+dot8<11,7>"; ME is None for the multiply-accumulate kernels."""
    family, args = last.rstrip(">").split("<")
    nums = [int(x) for x in args.split(",")]
    return family, nums[0], (nums[1] if len(nums) > 1 else None)


def kernel_geom(last, N):
    """(K, nl, G) the kernel named `last` runs N with: the shared stepping's K is its own, every other family's is pick_K(N)."""
    return geom(N, kernel_tuple(last)[1])


# ---- the N of the sweep ---------------------------------------------------------------------------------------------------------------
SHARED_KS = (9, 11, 13)


def shared_boundary_ns():
    """Odd N on either side of the two ends of each nl == 32 stretch of the shared stepping (K = 9, 11, 13: N = 62 K + 1 .. 64 K), two
    on each side: nl = 31 | 32 with one and three coefficients in the last lane, and the step to the next K."""
    out = set()
    for K in SHARED_KS:
        for edge in (62 * K, 64 * K):
            out |= {edge - 3, edge - 1, edge + 1, edge + 3}
    return out


def sweep_ns(K):
    """The N of kv.K_RANGES[K] at which the geometry is an edge.
    A, several items per wave: K = 1: every N from 2 to 64 (nl = 1..32); K = 3: N = 129..134 and 187..192 (nl = 22, 23, 32; G = 2).
    B, one item per wave: the range's lo, lo + 1, hi - 1, hi; for nl in {the range's smallest with G = 1, the middle one, 63, 64} the
    four fills of the last lane N = 2K (nl - 1) + t, t in {1, 2, 2K - 1, 2K}; the odd N around the shared stepping's nl == 32 stretches."""
    lo, hi = kv.K_RANGES[K]
    ns = {lo, lo + 1, hi - 1, hi}
    if K == 1:
        ns |= set(range(2, 65))
    if K == 3:
        ns |= set(range(129, 135)) | set(range(187, 193))
    nl_min = max(33, -(-lo // (2 * K)))
    for nl in (nl_min, (nl_min + 64) // 2, 63, 64):
        ns |= {2 * K * (nl - 1) + t for t in (1, 2, 2 * K - 1, 2 * K)}
    ns |= shared_boundary_ns()
    return sorted(n for n in ns if lo <= n <= hi)


# ---- the calls of the sweep -----------------------------------------------------------------------------------------------------------
# (p, kernel paths) per entry: decrypt's p = 5 on the multiply-accumulate path alone (no other family takes p != 3)
ENTRY_P = {"encrypt": ((0, PATHS),), "decrypt": ((3, PATHS), (5, (1,))), "verify_keys": ((3, PATHS), (5, PATHS)),
           "polymul_split": ((0, PATHS),), "public_key": ((3, PATHS), (8, PATHS))}


def moduli(entry, N, p, path):
    """The q to launch at (entry, N, p, path): the first of QS, taken in an order that rotates with N, for every distinct kernel name
    the ABI-accepted q reach there (none where only a matrix-core kernel may apply).  verify_keys at p = 5 keeps to q <= 8192, and
    polymul_split also takes modulus 3 (the finish that is no power of two)."""
    qs = QS[N % len(QS):] + QS[:N % len(QS)]
    first = {}
    for q in qs:
        if not accepted(entry, N, q, p) or (entry == "verify_keys" and p == 5 and q > 8192):
            continue
        name = expected_last(entry, N, q, p, path)
        if name is not None:
            first.setdefault(name, q)
    out = sorted(first.values())
    if entry == "polymul_split":
        out.append(3)
    return out


def batch_sizes(entry, G):
    """B = 1, G + 1, 4 G + 1: a lone item, a second wave with one item, a second workgroup with one.  verify_keys: at least 7 where a
    wave holds several items, so that the five flag kinds of its key pairs sit in different slots of one wave."""
    return [1, max(G + 1, 7) if entry == "verify_keys" and G > 1 else G + 1, 4 * G + 1]


def calls(entry, K):
    """Every call of the sweep for `entry` at the N of sweep_ns(K): dicts of N, q, p, path, last (the kernel name to expect), B,
    variant (the runners' edge operands: rotates with N and with B, so each (N, q, path) meets all three) and witness (decrypt also
    runs value-only at its middle B)."""
    out = []
    for N in sweep_ns(K):
        for p, paths in ENTRY_P[entry]:
            for path in paths:
                for q in moduli(entry, N, p, path):
                    last = expected_last(entry, N, q, p, path)
                    G = kernel_geom(last, N)[2]
                    for i, B in enumerate(batch_sizes(entry, G)):
                        c = dict(N=N, q=q, p=p, path=path, last=last, B=B, variant=(N + i) % 3, witness=True)
                        out.append(c)
                        if entry == "decrypt" and p == 3 and i == 1:
                            out.append(dict(c, witness=False))
    return out


def cases(entry, K):
    """The distinct (entry, N, path, q, p) of calls(entry, K)."""
    return sorted({(entry, c["N"], c["path"], c["q"], c["p"]) for c in calls(entry, K)})
