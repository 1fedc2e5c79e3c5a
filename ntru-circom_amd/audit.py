"""Auditing a mix (include/ntru_engine.h "auditing a mix"): checking revealed re-encryption links on the device, and the host layer that
makes a round of randomized partial checking (RPC) out of it.  Link l claims e_out[out_idx[l]] == r[l] * h + e_in[in_idx[l]] modulo
(x^N - 1, q); check_links returns one flag byte per link (0: the link holds) and the number of links that do not.  For a pair of mix steps
e0 -> e1 -> e2 a public challenge `side` picks, for every middle item, whether its incoming or its outgoing link is opened: open_links is
the prover's half, verify_rpc the auditor's.  The challenge is an input: a beacon or a hash of the published batches is the caller's
affair.  Functions on an Engine: its class keeps the methods it had."""
import collections

import numpy as np

from .engine import _np, _ptr

LINK_BAD_INDEX, LINK_BAD_R, LINK_MISMATCH = 1, 2, 4          # NTRU_LINK_* (include/ntru_engine.h)

Links = collections.namedtuple("Links", "in_idx out_idx r")
RpcResult = collections.namedtuple("RpcResult", "ok structure bad")


def _idx(a, L, what):
    if a is None:
        return None
    a = _np(a, np.int64).reshape(-1)
    if a.shape[0] != L:
        raise ValueError("check_links: r has %d rows, %s %d entries" % (L, what, a.shape[0]))
    return a


def check_links(eng, N, q, h, r, e_in, e_out, in_idx=None, out_idx=None, other=2, n1=-1, n2=-1):
    """h (N,) uint16; r [L][N] uint8; e_in [B_in][N], e_out [B_out][N] uint16 (any value, compared mod q); in_idx / out_idx [L] int64 or
    None (link l uses row l).  other: the third value of r (p - 1); n1 / n2: the ones and the `other` entries a row of r must hold (-1:
    not tested).  Returns (flags [L] uint8, n_bad): LINK_BAD_INDEX | LINK_BAD_R, or LINK_MISMATCH alone, or 0."""
    h = _np(h, np.uint16, (N,))
    r = _np(r, np.uint8).reshape(-1, N)
    e_in, e_out = _np(e_in, np.uint16).reshape(-1, N), _np(e_out, np.uint16).reshape(-1, N)
    L = r.shape[0]
    in_idx, out_idx = _idx(in_idx, L, "in_idx"), _idx(out_idx, L, "out_idx")
    flags = np.empty(L, np.uint8)
    n_bad = np.zeros(1, np.int64)
    eng._chk(eng._lib.ntru_check_links_batch(eng._h, N, q, int(other), int(n1), int(n2), _ptr(h), _ptr(r), _ptr(e_in), e_in.shape[0],
                                             _ptr(in_idx), _ptr(e_out), e_out.shape[0], _ptr(out_idx), L, _ptr(flags), _ptr(n_bad)))
    return flags, int(n_bad[0])


def check_links_dev(eng, N, q, d_h, d_r, d_e_in, B_in, d_e_out, B_out, L, d_flags, d_n_bad=None, d_in_idx=None, d_out_idx=None, other=2,
                    n1=-1, n2=-1):
    """The same on DEVICE pointers, enqueued on the engine's stream; d_in_idx / d_out_idx: int64 [L] in device memory; d_n_bad: one
    int64 in device memory, set by the call, or None.  An index outside its array is flagged and no row of that link is read."""
    dp = eng._dp
    eng._chk(eng._lib.ntru_check_links_batch_dev(eng._h, N, q, int(other), int(n1), int(n2), dp(d_h), dp(d_r), dp(d_e_in), int(B_in),
                                                 dp(d_in_idx), dp(d_e_out), int(B_out), dp(d_out_idx), int(L), dp(d_flags), dp(d_n_bad)))


# ---- randomized partial checking of a pair of mix steps e0 -> e1 -> e2 -----------------------------------------------------------------
def open_links(side, src1, r1, src2, r2):
    """The prover's half.  src1, r1 / src2, r2: what mix_batch returned for the two steps (e1[j] re-randomises e0[src1[j]] with r1[j],
    e2[k] re-randomises e1[src2[k]] with r2[k]; src2 a permutation).  side[j] == 0 opens the left link of middle item j, (in = src1[j],
    out = j, r1[j]); side[j] != 0 the right one, (in = j, out = k, r2[k]) with src2[k] == j.  Returns (left, right), each a Links
    (in_idx, out_idx, r) in ascending order of j."""
    side = np.asarray(side).reshape(-1)
    src1, src2 = np.asarray(src1, np.int64).reshape(-1), np.asarray(src2, np.int64).reshape(-1)
    B = side.shape[0]
    if src1.shape[0] != B or src2.shape[0] != B:
        raise ValueError("open_links: side, src1 and src2 need one entry per item")
    r1, r2 = np.asarray(r1).reshape(B, -1), np.asarray(r2).reshape(B, -1)
    dst2 = np.empty(B, np.int64)
    dst2[src2] = np.arange(B, dtype=np.int64)                    # dst2[j] = the k with src2[k] == j
    jl, jr = np.flatnonzero(side == 0), np.flatnonzero(side != 0)
    return Links(src1[jl], jl.astype(np.int64), r1[jl]), Links(jr.astype(np.int64), dst2[jr], r2[dst2[jr]])


def _structure(side, left, right):
    """What the opened lists must look like whatever the rows hold: messages, empty when all is well."""
    side = np.asarray(side).reshape(-1)
    B, out = side.shape[0], []
    want_left, want_right = np.flatnonzero(side == 0), np.flatnonzero(side != 0)
    if not np.array_equal(np.sort(np.asarray(left.out_idx, np.int64)), want_left):
        out.append("left: the opened outputs are not exactly the middle items with side == 0")
    if not np.array_equal(np.sort(np.asarray(right.in_idx, np.int64)), want_right):
        out.append("right: the opened inputs are not exactly the middle items with side != 0")
    for name, links in (("left", left), ("right", right)):
        for what, idx in (("input", links.in_idx), ("output", links.out_idx)):
            idx = np.asarray(idx, np.int64).reshape(-1)
            if np.unique(idx).size != idx.size:
                out.append("%s: an %s index occurs twice" % (name, what))
        if len(links.in_idx) != len(links.out_idx) or len(links.in_idx) != len(links.r):
            out.append("%s: in_idx, out_idx and r differ in length" % name)
    if len(left.in_idx) + len(right.in_idx) != B:
        out.append("the two lists do not open one link per middle item")
    return out


def verify_rpc(eng, N, q, h, e0, e1, e2, side, left, right, other=2, n1=-1, n2=-1):
    """The auditor's half: the structure of the opening on the host (left.out_idx is exactly {j : side[j] == 0}, right.in_idx exactly
    {j : side[j] != 0}, no index twice within a list), then every left link against (e0, e1) and every right link against (e1, e2).
    Returns RpcResult(ok, structure, bad): structure the messages of the host checks, bad the (list, position, flag) of every link
    whose flag is not 0.  A cheating mixer that replaced one output is caught only when the challenge opened that link: one round halves
    its chance, and says nothing about items whose links stayed closed."""
    structure = _structure(side, left, right)
    bad = []
    for name, links, a, b in (("left", left, e0, e1), ("right", right, e1, e2)):
        if len(links.r) == 0 or len(links.in_idx) != len(links.r) or len(links.out_idx) != len(links.r):
            continue
        flags, n_bad = check_links(eng, N, q, h, links.r, a, b, in_idx=links.in_idx, out_idx=links.out_idx, other=other, n1=n1, n2=n2)
        if n_bad:
            bad += [(name, int(i), int(flags[i])) for i in np.flatnonzero(flags)]
    return RpcResult(not structure and not bad, structure, bad)
