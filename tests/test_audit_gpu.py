"""Auditing a mix on the GPU (ntru_check_links_batch, csrc/mix_audit.hip): every comparison is flags.tobytes() and n_bad against the numpy
restatement (tests/audit_ref.py).  The fixture of the unmodified reference through the three interfaces, every shape that takes another
path, every coefficient of a row block, the reduction mod q, the extremes, the domain of r, indices that must not be followed, the
kernel paths, the pass edge of the vector-ALU route, a round of randomized partial checking end to end, and the refusals.  Every _dev
call of this module runs between guard rows that must come back unchanged (run_links)."""
import ctypes as C

import numpy as np
import pytest

import __graft_entry__ as ge
import audit_ref as ref
import mix_ref

pytestmark = pytest.mark.gpu
pkg = ge.load_package()
U16, U8 = np.uint16, np.uint8
OK, BAD_INDEX, BAD_R, MISMATCH = 0, ref.BAD_INDEX, ref.BAD_R, ref.MISMATCH


@pytest.fixture(scope="module")
def eng():
    e = pkg.Engine(0)
    yield e
    e.set_kernel_path(0)


@pytest.fixture(scope="module")
def cases():
    return mix_ref.load_cases()


class Dev:
    """Device copies of host arrays through the engine's own allocator (256-byte aligned); `shift` elements off that boundary."""

    def __init__(self, eng):
        self.eng, self.held = eng, []

    def put(self, a, shift=0):
        a = np.ascontiguousarray(a)
        p = self.eng.dev_alloc(a.nbytes + 64)
        self.held.append(p)
        p += shift * a.itemsize
        if a.nbytes:
            self.eng.dev_upload(p, a)
        return p

    def guarded(self, a, fill, shift=0):
        """a with one guard row of `fill` before and after it: (pointer to a, (pointer to the whole, the whole as uploaded))."""
        a = np.ascontiguousarray(a)
        guard = np.full((1,) + a.shape[1:], fill, a.dtype) if a.ndim == 2 else np.full(16, fill, a.dtype)
        whole = np.concatenate([guard, a, guard])
        p = self.put(whole, shift)
        return p + guard.nbytes, (p, whole)

    def free(self):
        self.eng.synchronize()
        for p in self.held:
            self.eng.dev_free(p)
        self.held = []


def run_links(eng, d, N, q, h, r, e_in, e_out, in_idx=None, out_idx=None, shifts=(0, 0, 0), same=False, check=True, **kw):
    """One _dev call on fresh device copies, every array between guard rows; shifts: byte offset of d_r, element offsets of d_e_in and
    d_e_out; same: e_out IS e_in on the device (one array).  r, e_in, e_out and every guard must come back unchanged, flags beyond L
    untouched.  Returns (flags, n_bad), compared with the restatement unless check is False."""
    r, e_in = np.asarray(r).astype(U8), np.asarray(e_in).astype(U16)
    e_out = e_in if same else np.asarray(e_out).astype(U16)
    L = r.shape[0]
    d_h = d.put(np.asarray(h).astype(U16))
    d_r, keep_r = d.guarded(r, 0xA5, shifts[0])
    d_in, keep_in = d.guarded(e_in, 0xABCD, shifts[1])
    d_out, keep_out = (d_in, None) if same else d.guarded(e_out, 0xDCBA, shifts[2])
    d_flags, keep_fl = d.guarded(np.full(L, 0x5A, U8), 0x5A, 1)
    d_nbad = d.put(np.array([-7], np.int64))
    d_i = None if in_idx is None else d.put(np.asarray(in_idx, np.int64))
    d_o = None if out_idx is None else d.put(np.asarray(out_idx, np.int64))
    pkg.check_links_dev(eng, N, q, d_h, d_r, d_in, e_in.shape[0], d_out, e_out.shape[0], L, d_flags, d_n_bad=d_nbad, d_in_idx=d_i,
                        d_out_idx=d_o, **kw)
    for keep in (keep_r, keep_in, keep_out):
        if keep is not None:
            p, whole = keep
            assert eng.dev_download(p, whole.shape, whole.dtype).tobytes() == whole.tobytes()
    got = eng.dev_download(keep_fl[0], keep_fl[1].shape, U8)
    assert got[:16].tobytes() == got[16 + L:].tobytes() == np.full(16, 0x5A, U8).tobytes()
    flags, n_bad = got[16:16 + L], int(eng.dev_download(d_nbad, (1,), np.int64)[0])
    if check:
        want, want_bad = ref.check_links(N, q, h, r, e_in, e_out, in_idx, out_idx, **kw)
        assert flags.tobytes() == want.tobytes(), (N, q, L, shifts, np.flatnonzero(flags != want)[:8], flags[flags != want][:8])
        assert n_bad == want_bad
    return flags, n_bad


def honest(N, q, h, r, e_in, in_idx, B_out, out_idx, g):
    """e_out [B_out][N] with e_out[out_idx[l]] the re-encryption of e_in[in_idx[l]] (random rows elsewhere, 16-bit values)."""
    L = r.shape[0]
    i = np.arange(L) if in_idx is None else np.asarray(in_idx)
    o = np.arange(L) if out_idx is None else np.asarray(out_idx)
    e_out = g.integers(0, 65536, (B_out, N))
    e_out[o] = mix_ref.reencrypt(N, q, h, r, e_in, i)[0]
    return e_out


def ternary(g, L, N, dr):
    """[L][N] with dr ones and dr twos per row."""
    r = np.zeros((L, N), np.int64)
    for l in range(L):
        at = g.permutation(N)[:2 * dr]
        r[l, at[:dr]], r[l, at[dr:]] = 1, 2
    return r


# ---- 1. the fixture ---------------------------------------------------------------------------------------------------------------------
def test_fixture_through_every_form(eng, cases):
    eng.set_kernel_path(0)
    for c in cases:
        o = c["options"]
        N, q, p, dr = o["N"], o["q"], o["p"], o["dr"]
        h = c["key"]["h"].astype(U16)
        ntru = pkg.NTRU({**o, "h": h.tolist()}, engine=eng)
        cur = c["e"]
        d = Dev(eng)
        try:
            for rd in c["rounds"]:
                src, r, out = rd["src"], rd["r"], rd["remainder"].copy()
                for mutate in (False, True):
                    if mutate:
                        out[len(src) // 2, N // 3] ^= 1
                    kw = dict(other=p - 1, n1=dr, n2=dr)
                    want, want_bad = ref.check_links(N, q, h, r, cur, out, src, None, **kw)
                    assert want_bad == int(mutate)
                    a = pkg.audit.check_links(eng, N, q, h, r, cur, out, in_idx=src, **kw)
                    b = ntru.auditLinks(cur, out, r, in_idx=src)
                    cdev = run_links(eng, d, N, q, h, r, cur, out, src, None, **kw)
                    for flags, n_bad in (a, (b["flags"], b["bad"]), cdev):
                        assert flags.tobytes() == want.tobytes() and n_bad == want_bad, c["set"]
                cur = rd["remainder"]
        finally:
            d.free()


# ---- 2. shapes --------------------------------------------------------------------------------------------------------------------------
# N, q, kernel path, the kernel a dword-aligned call must report
SHAPES = [(17, 32, 4, "k_linkcheck_m"), (64, 64, 0, "k_linkcheck_md"), (167, 128, 0, "k_linkcheck_md"), (509, 2048, 0, "k_linkcheck_md"),
          (701, 8192, 0, "k_linkcheck_md"), (821, 4096, 0, "k_linkcheck_md"), (1022, 8192, 0, "k_linkcheck_m"),
          (1024, 8192, 0, "k_linkcheck_md"), (167, 65536, 0, "k_compare_links"), (1100, 2048, 0, "k_compare_links")]


@pytest.mark.parametrize("N,q,path,kernel", SHAPES)
def test_shapes_equal_the_restatement(eng, N, q, path, kernel):
    g = np.random.default_rng(N * 37 + q)
    eng.set_kernel_path(path)
    h = g.integers(0, q, N)
    d = Dev(eng)
    try:
        for L in (1, 31, 32, 33, 97):
            r = g.integers(0, 3, (L, N))
            # identity on both sides, B_in != B_out != L
            e_in = g.integers(0, 65536, (L + 2, N))
            e_out = honest(N, q, h, r, e_in, None, L + 5, None, g)
            e_out[L // 2, (7 * L) % N] ^= 1                                         # one link that does not hold
            run_links(eng, d, N, q, h, r, e_in, e_out)
            assert eng.last_kernel() == kernel
            # a permutation on each side
            pi, po = g.permutation(L), g.permutation(L)
            e_out = honest(N, q, h, r, e_in[:L], pi, L, po, g)
            run_links(eng, d, N, q, h, r, e_in[:L], e_out, pi, po)
            # a gather with repeats on the input side and two links to one output row; r off the dword, both arrays at odd elements
            gi, go = g.integers(0, 5, L), g.permutation(L + 3)[:L]
            r2 = r.copy()
            if L > 1:
                gi[-1], go[-1], r2[-1] = gi[0], go[0], r2[0]
            e_out = honest(N, q, h, r2, e_in[:5], gi, L + 3, go, g)
            e_in2 = e_in[:5].copy()
            if L > 2:
                e_in2[gi[1], N - 1] ^= 0x40 if q > 64 else 1                         # every link that reads this row
            run_links(eng, d, N, q, h, r2, e_in2, e_out, gi, go, shifts=(1 + L % 3, 1, 1))
            if N == 1024:                                                           # rows of r off the dword: too long for the one-instruction DMA
                assert eng.last_kernel() == "k_linkcheck_m"
            # e_in is e_out: rows 0 .. L-1 are the inputs, rows L .. 2L-1 the outputs of one array
            both = np.concatenate([e_in[:L], np.zeros((L, N), np.int64)])
            both[L + po] = mix_ref.reencrypt(N, q, h, r, e_in[:L], pi)[0]
            both[L + po[0], 0] ^= 1
            run_links(eng, d, N, q, h, r, both, None, pi, L + po, same=True, shifts=(2, 1, 0))
    finally:
        eng.set_kernel_path(0)
        d.free()


# ---- 3. every coefficient can be caught, and only its own row is --------------------------------------------------------------------------
@pytest.mark.parametrize("N,q", [(167, 128), (821, 4096), (1024, 8192)])
def test_every_coefficient_is_compared_and_flags_only_its_row(eng, N, q):
    """ceil(N / 48) calls on L = 97 links; call c changes the rows l with l % 2 == c % 2, each at the one column (48 c + l) mod N,
    alternately in e_out (+1 mod q) and in e_in (-1 mod q).  At an odd N the walk changes parity where it wraps and those calls leave
    a few columns out (11 at N = 167, 2 at N = 821), so the calls go on -- one more is enough -- until every column has been hit: 0, 31,
    32, N - 1 and the last partial tile among them, in rows of the first, a middle and the last (partial) row block.  The rows in
    between must come out 0."""
    L = 97
    g = np.random.default_rng(N)
    eng.set_kernel_path(0)
    h, r, e_in = g.integers(0, q, N), g.integers(0, 3, (L, N)), g.integers(0, q, (L, N))
    pi = g.permutation(L)
    e_out = mix_ref.reencrypt(N, q, h, r, e_in, pi)[0].astype(np.int64)
    hit = np.zeros(N, bool)
    d = Dev(eng)
    try:
        c = -1
        while c + 1 < -(-N // 48) or not hit.all():
            c += 1
            assert c <= -(-N // 48)
            a, b = e_in.copy(), e_out.copy()
            want = np.zeros(L, U8)
            for l in range(c % 2, L, 2):
                col = (48 * c + l) % N
                hit[col] = True
                if (l // 2) % 2:
                    a[pi[l], col] = (a[pi[l], col] - 1) % q
                else:
                    b[l, col] = (b[l, col] + 1) % q
                want[l] = MISMATCH
            flags, n_bad = run_links(eng, d, N, q, h, r, a, b, pi, None)
            assert flags.tobytes() == want.tobytes() and n_bad == int(np.count_nonzero(want)), c
            d.free()
        assert eng.last_kernel() == "k_linkcheck_md"
        assert hit.all()
    finally:
        d.free()


# ---- 4. reduction mod q -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("N,q", [(167, 128), (821, 4096), (1024, 8192), (167, 65536), (1100, 2048)])
def test_both_sides_are_reduced_mod_q(eng, N, q):
    L = 70
    g = np.random.default_rng(q + N)
    eng.set_kernel_path(0)
    h, r, e_in = g.integers(0, q, N), g.integers(0, 3, (L, N)), g.integers(0, q, (L, N))
    e_out = mix_ref.reencrypt(N, q, h, r, e_in)[0].astype(np.int64)
    step = q if q < 65536 else 128                       # q = 65536: nothing can be added to 16 bits; what is added instead is a real change
    a = (e_in + step * g.integers(0, 2, (L, N)) * ((65535 - e_in) // step > 0)) % 65536
    b = (e_out + step * g.integers(0, 2, (L, N)) * ((65535 - e_out) // step > 0)) % 65536
    assert (a != e_in).any() and (b != e_out).any()
    d = Dev(eng)
    try:
        flags, n_bad = run_links(eng, d, N, q, h, r, a, b)
        if q < 65536:
            assert not flags.any() and n_bad == 0
        else:
            assert (flags == MISMATCH).all() and n_bad == L
    finally:
        d.free()


# ---- 5. extremes ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("N,q,other", [(167, 128, 2), (821, 4096, 2), (1024, 8192, 3), (701, 8192, 3), (167, 65536, 2)])
def test_largest_accumulators_and_addend(eng, N, q, other):
    L = 33
    g = np.random.default_rng(1)
    eng.set_kernel_path(0)
    h, r, e_in = np.full(N, q - 1), np.full((L, N), other), np.full((L, N), 65535)
    e_out = mix_ref.reencrypt(N, q, h, r, e_in)[0].astype(np.int64)
    d = Dev(eng)
    try:
        flags, n_bad = run_links(eng, d, N, q, h, r, e_in, e_out, other=other)
        assert not flags.any() and n_bad == 0
        e_out[:, N - 1] = (e_out[:, N - 1] + 1) % q
        e_out[7, N - 1] = (e_out[7, N - 1] - 1) % q
        flags, n_bad = run_links(eng, d, N, q, h, r, e_in, e_out, g.permutation(L), other=other)      # (every input row is the same)
        assert flags[7] == OK and (np.delete(flags, 7) == MISMATCH).all() and n_bad == L - 1
    finally:
        d.free()


# ---- 6. the domain of r and its counts --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("N,q,path", [(167, 128, 0), (167, 128, 4), (821, 4096, 0), (1024, 8192, 0), (167, 65536, 0), (167, 128, 2)])
def test_r_domain_and_counts(eng, N, q, path):
    L, dr = 97, 11
    g = np.random.default_rng(N + path)
    eng.set_kernel_path(path)
    h, e_in = g.integers(0, q, N), g.integers(0, q, (L, N))
    r = ternary(g, L, N, dr)
    outside = {3: (3, 0), 34: (4, N // 2), 64: (255, N - 1), 96: (3, N - 1), 31: (255, 0), 33: (4, 1)}       # row: (byte, position)
    counts = {}                                           # rows whose counts are off by one, in either direction, in the domain
    for row, (frm, to) in {10: (1, 0), 12: (0, 1), 50: (2, 0), 52: (0, 2)}.items():
        at = int(np.flatnonzero(r[row] == frm)[0])
        r[row, at] = to
        counts[row] = True
    e_out = mix_ref.reencrypt(N, q, h, r, e_in)[0].astype(np.int64)          # the count rows are links that hold
    for row, (byte, pos) in outside.items():
        r[row, pos] = byte
    d = Dev(eng)
    try:
        want = np.zeros(L, U8)
        want[list(outside)] = BAD_R
        flags, n_bad = run_links(eng, d, N, q, h, r, e_in, e_out)                                   # counts not asked for
        assert flags.tobytes() == want.tobytes() and n_bad == len(outside)
        want[list(counts)] = BAD_R
        flags, n_bad = run_links(eng, d, N, q, h, r, e_in, e_out, n1=dr, n2=dr)
        assert flags.tobytes() == want.tobytes() and n_bad == len(outside) + len(counts)
        for n1, n2 in ((dr + 1, -1), (dr - 1, dr), (-1, dr + 1), (dr, dr - 1)):                    # the counts asked for are off instead
            flags, _ = run_links(eng, d, N, q, h, r, e_in, e_out, n1=n1, n2=n2)
            clean = [l for l in range(L) if l not in outside and l not in counts]
            assert (flags[clean] == BAD_R).all() and (flags[list(outside)] == BAD_R).all()
        d.free()
        # other = 1: the ones number n1 + n2
        r1 = (ternary(g, L, N, dr) != 0).astype(np.int64)
        r1[40, int(np.flatnonzero(r1[40])[0])] = 0
        e1 = mix_ref.reencrypt(N, q, h, r1, e_in)[0].astype(np.int64)
        r1[41, 5] = 2
        want = np.zeros(L, U8)
        want[41] = BAD_R
        assert run_links(eng, d, N, q, h, r1, e_in, e1, other=1)[0].tobytes() == want.tobytes()
        want[40] = BAD_R
        assert run_links(eng, d, N, q, h, r1, e_in, e1, other=1, n1=dr + 2, n2=dr - 2)[0].tobytes() == want.tobytes()
        assert run_links(eng, d, N, q, h, r1, e_in, e1, other=1, n1=dr, n2=-1)[0][40] == OK
    finally:
        eng.set_kernel_path(0)
        d.free()


# ---- 7. indices the kernels must not follow -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("N,q,path", [(167, 128, 0), (167, 128, 4), (821, 4096, 0), (167, 65536, 0)])
def test_out_of_range_indices_are_flagged_and_not_followed(eng, N, q, path):
    """-1, B_in, B_out and 2^40 on either side give exactly BAD_INDEX, the links around them are judged as usual, and the guard rows
    before and after both arrays are not mistaken for rows (run_links)."""
    g = np.random.default_rng(q + N + path)
    B_in, B_out, L = 5, 7, 40
    eng.set_kernel_path(path)
    h, r, e_in = g.integers(0, q, N), g.integers(0, 3, (L, N)), g.integers(0, q, (B_in, N))
    i, o = g.integers(0, B_in, L), np.concatenate([g.permutation(B_out), g.integers(0, B_out, L - B_out)])
    e_out = g.integers(0, q, (B_out, N))
    e_out[o[:B_out]] = mix_ref.reencrypt(N, q, h, r[:B_out], e_in, i[:B_out])[0]            # the first 7 links hold, the others do not
    i[[0, 9, 31, 32]] = [-1, B_in, 1 << 40, -1]
    o[[2, 9, 33, 39]] = [B_out, -1, 1 << 40, B_out]
    r[32, 4] = 77                                                                          # a bad index and a bad r: both bits
    d = Dev(eng)
    try:
        flags, n_bad = run_links(eng, d, N, q, h, r, e_in, e_out, i, o)
        assert flags[[0, 2, 9, 31, 33, 39]].tolist() == [BAD_INDEX] * 6 and flags[32] == BAD_INDEX | BAD_R
        assert flags[[1, 3, 4, 5, 6]].tolist() == [OK] * 5 and (flags[10:31] == MISMATCH).all()
        host = pkg.audit.check_links(eng, N, q, h, r, e_in, e_out, in_idx=i, out_idx=o)
        assert host[0].tobytes() == flags.tobytes() and host[1] == n_bad
    finally:
        eng.set_kernel_path(0)
        d.free()


# ---- 8. kernel paths ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("N,q", [(167, 128), (821, 4096)])
def test_kernel_paths_agree(eng, N, q):
    L = 97
    g = np.random.default_rng(5 + N)
    h, r, e_in = g.integers(0, q, N), g.integers(0, 3, (L, N)), g.integers(0, 65536, (40, N))
    i, o = g.integers(0, 40, L), g.permutation(L)
    e_out = honest(N, q, h, r, e_in, i, L, o, g)
    i[3], o[70] = 40, -1
    r[50, N - 1], r[96, 0] = 3, 200
    e_out[o[20], 33] ^= 1
    e_out[o[64], N - 1] ^= 1
    want, want_bad = ref.check_links(N, q, h, r, e_in, e_out, i, o)
    assert sorted(set(want.tolist())) == [OK, BAD_INDEX, BAD_R, MISMATCH] and want_bad == 6
    d = Dev(eng)
    try:
        for path, kernel in ((0, "k_linkcheck_md"), (1, "k_compare_links"), (2, "k_compare_links"), (3, "k_compare_links"),
                             (4, "k_linkcheck_m"), (5, "k_linkcheck_md")):
            eng.set_kernel_path(path)
            flags, n_bad = run_links(eng, d, N, q, h, r, e_in, e_out, i, o, check=False)
            assert eng.last_kernel() == kernel
            assert flags.tobytes() == want.tobytes() and n_bad == want_bad, path
            host = pkg.audit.check_links(eng, N, q, h, r, e_in, e_out, in_idx=i, out_idx=o)
            assert host[0].tobytes() == want.tobytes() and host[1] == want_bad, path
            d.free()
    finally:
        eng.set_kernel_path(0)
        d.free()


# ---- 9. the pass edge of the vector-ALU route ---------------------------------------------------------------------------------------------
def test_pass_edge_of_the_vector_alu_route(eng):
    N, q, L = 17, 32, 65536 + 33
    g = np.random.default_rng(9)
    eng.set_kernel_path(0)
    h, r, e_in = g.integers(0, q, N), g.integers(0, 3, (L, N)), g.integers(0, q, (64, N))
    i = g.integers(0, 64, L)
    e_out = mix_ref.reencrypt(N, q, h, r, e_in, i)[0].astype(np.int64)
    e_out[65535, 16] ^= 1
    e_out[65536, 0] ^= 1
    r[L - 1, 3] = 9
    d = Dev(eng)
    try:
        flags, n_bad = run_links(eng, d, N, q, h, r, e_in, e_out, i, None, check=False)
        assert eng.last_kernel() == "k_compare_links"
        want = np.zeros(L, U8)
        want[[65535, 65536]], want[L - 1] = MISMATCH, BAD_R
        assert flags.tobytes() == want.tobytes() and n_bad == 3
        rows = np.array([0, 65534, 65535, 65536, 65537, L - 2, L - 1])                     # the restatement on the rows around the edge
        assert ref.check_links(N, q, h, r[rows], e_in, e_out[rows], i[rows], None)[0].tobytes() == want[rows].tobytes()
    finally:
        d.free()


# ---- 10. a round of randomized partial checking ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("N,q", [(167, 128), (821, 4096)])
def test_rpc_round_end_to_end(eng, N, q):
    B, p, dr = 97, 3, 9
    g = np.random.default_rng(N)
    eng.set_kernel_path(0)
    h, e0 = g.integers(0, q, N).astype(U16), g.integers(0, q, (B, N)).astype(U16)
    key = g.integers(0, 1 << 32, 8, dtype=np.uint64).astype(np.uint32)
    e1, _, r1, src1 = pkg.mix.mix_batch(eng, N, q, p, h, key, 0, dr, dr, 1, e0, want_quot=False)
    e2, _, r2, src2 = pkg.mix.mix_batch(eng, N, q, p, h, key, B, dr, dr, 2, e1, want_quot=False)
    side = g.integers(0, 2, B)
    kw = dict(other=p - 1, n1=dr, n2=dr)
    left, right = pkg.audit.open_links(side, src1, r1, src2, r2)
    ref_left, ref_right = ref.open_links(side, src1, r1, src2, r2)
    assert all(np.array_equal(np.asarray(a), b) for a, b in zip(tuple(left) + tuple(right), ref_left + ref_right))
    res = pkg.audit.verify_rpc(eng, N, q, h, e0, e1, e2, side, left, right, **kw)
    assert res.ok and res.structure == [] and res.bad == []
    for links, a, b in ((left, e0, e1), (right, e1, e2)):
        assert not ref.check_links(N, q, h, links.r, a, b, links.in_idx, links.out_idx, **kw)[0].any()
    # the mixer replaces output row k by a fresh encryption: caught exactly when the challenge opened the right link of its source
    k = 41
    j = int(src2[k])
    forged = e2.copy()
    forged[k] = mix_ref.reencrypt(N, q, h, ternary(g, 1, N, dr), g.integers(0, 2, (1, N)))[0][0]
    for opened in (1, 0):
        side[j] = opened
        left, right = pkg.audit.open_links(side, src1, r1, src2, r2)
        res = pkg.audit.verify_rpc(eng, N, q, h, e0, e1, forged, side, left, right, **kw)
        assert res.structure == []
        if opened:
            pos = int(np.flatnonzero(right.in_idx == j)[0])
            assert not res.ok and res.bad == [("right", pos, MISMATCH)]
            assert ref.check_links(N, q, h, right.r, e1, forged, right.in_idx, right.out_idx, **kw)[0][pos] == MISMATCH
        else:
            assert res.ok and res.bad == []


# ---- 11. refusals -----------------------------------------------------------------------------------------------------------------------
def test_bad_arguments_launch_nothing(eng):
    lib = pkg.load_library()
    N, q, L = 17, 32, 4
    ptr = lambda a: None if a is None else a.ctypes.data_as(C.c_void_p)
    h, r = np.ones(N, U16), np.ones((L, N), U8)
    e_in, e_out = np.full((L, N), 7, U16), np.full((L, N), 9, U16)
    idx, flags, n_bad = np.arange(L, dtype=np.int64), np.full(L + 2, 0x5A, U8), np.full(1, -7, np.int64)
    eng.set_kernel_path(0)
    eng.add_batch(2, 4, [[1, 1]], [[1, 1]])
    before = eng.last_kernel()

    def host(N=N, q=q, other=2, n1=-1, n2=-1, h=h, r=r, e_in=e_in, B_in=L, i=idx, e_out=e_out, B_out=L, o=idx, L=L, flags=flags, n_bad=n_bad):
        return lib.ntru_check_links_batch(eng._h, N, q, other, n1, n2, ptr(h), ptr(r), ptr(e_in), B_in, ptr(i), ptr(e_out), B_out, ptr(o), L,
                                          ptr(flags), ptr(n_bad))

    for bad in (dict(h=None), dict(r=None), dict(e_in=None), dict(e_out=None), dict(flags=None), dict(B_in=-1), dict(B_out=-1),
                dict(L=-1), dict(other=0), dict(other=4), dict(n1=9, n2=9), dict(n1=18), dict(flags=r.reshape(-1)),
                dict(flags=e_out.view(U8).reshape(-1)[3:]), dict(flags=idx.view(U8)), dict(n_bad=idx[1:2])):
        assert host(**bad) == 2, bad
        assert lib.ntru_last_error()
    assert host(q=48) != 0 and host(N=1) != 0                                              # what every batch call refuses
    assert flags.tobytes() == np.full(L + 2, 0x5A, U8).tobytes() and n_bad[0] == -7
    assert r.tobytes() == np.ones((L, N), U8).tobytes() and e_out.tobytes() == np.full((L, N), 9, U16).tobytes()
    d = Dev(eng)
    try:
        d_h, d_r, d_in, d_out, d_idx = d.put(h), d.put(r), d.put(e_in), d.put(e_out), d.put(idx)
        d_flags, d_nbad = d.put(flags), d.put(n_bad)

        def dev(other=2, n1=-1, n2=-1, h=d_h, r=d_r, e_in=d_in, B_in=L, i=d_idx, e_out=d_out, B_out=L, o=d_idx, L=L, flags=d_flags, n_bad=d_nbad):
            return lib.ntru_check_links_batch_dev(eng._h, N, q, other, n1, n2, h, r, e_in, B_in, i, e_out, B_out, o, L, flags, n_bad)

        for bad in (dict(h=None), dict(r=None), dict(e_in=None), dict(e_out=None), dict(flags=None), dict(B_in=-1), dict(B_out=-1),
                    dict(L=-1), dict(other=0), dict(other=4), dict(n1=9, n2=9), dict(flags=d_r + 1), dict(flags=d_out + 2 * N * L - 1),
                    dict(flags=d_idx), dict(n_bad=d_in), dict(n_bad=d_flags)):
            assert dev(**bad) == 2, bad
        eng.synchronize()
        assert eng.last_kernel() == before
        assert eng.dev_download(d_flags, (L + 2,), U8).tobytes() == flags.tobytes()
        assert eng.dev_download(d_nbad, (1,), np.int64)[0] == -7
        assert eng.dev_download(d_r, (L, N), U8).tobytes() == r.tobytes()
        assert eng.dev_download(d_out, (L, N), U16).tobytes() == e_out.tobytes()
        # L == 0 launches nothing and sets n_bad
        assert dev(L=0, r=None, flags=None) == 0 and host(L=0, r=None, flags=None) == 0
        eng.synchronize()
        assert eng.last_kernel() == before
        assert eng.dev_download(d_nbad, (1,), np.int64)[0] == 0 and n_bad[0] == 0
        assert dev(L=0, n_bad=None) == 0
    finally:
        d.free()
    got, bad = pkg.audit.check_links(eng, N, q, h, r[:0], e_in, e_out)                       # L = 0 through the binding
    assert got.shape == (0,) and bad == 0
    with pytest.raises(ValueError):
        pkg.audit.check_links(eng, N, q, h, r, e_in, e_out, in_idx=[0, 1])
