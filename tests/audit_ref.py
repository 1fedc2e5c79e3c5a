"""numpy restatement of ntru_check_links_batch (include/ntru_engine.h "auditing a mix") and of the host layer of audit.py, written
independently of it on top of mix_ref.reencrypt / mix_ref.gather_rows: the checker the GPU tests of the link-check kernels use, tied to
the reference's fixture by tests/test_audit_cpu.py.  Not a test module."""
import numpy as np

import mix_ref

BAD_INDEX, BAD_R, MISMATCH = 1, 2, 4


def r_is_bad(r, other, n1, n2):
    """[L] bool: a byte outside {0, 1, other}, or a count that is asked for and differs."""
    r = np.asarray(r).astype(np.int64)
    bad = ((r != 0) & (r != 1) & (r != other)).any(axis=1)
    ones, others = (r == 1).sum(axis=1), (r == other).sum(axis=1)
    if other == 1:
        if n1 >= 0 and n2 >= 0:
            bad |= ones != n1 + n2
    else:
        if n1 >= 0:
            bad |= ones != n1
        if n2 >= 0:
            bad |= others != n2
    return bad


def check_links(N, q, h, r, e_in, e_out, in_idx=None, out_idx=None, other=2, n1=-1, n2=-1):
    """(flags [L] uint8, n_bad): BAD_INDEX and BAD_R wherever they apply, MISMATCH only on a link with neither."""
    r = np.asarray(r).astype(np.int64).reshape(-1, N)
    L = r.shape[0]
    e_in, e_out = np.asarray(e_in).reshape(-1, N), np.asarray(e_out).reshape(-1, N)
    i = np.arange(L, dtype=np.int64) if in_idx is None else np.asarray(in_idx, np.int64).reshape(-1)
    o = np.arange(L, dtype=np.int64) if out_idx is None else np.asarray(out_idx, np.int64).reshape(-1)
    assert i.shape[0] == L and o.shape[0] == L
    flags = np.zeros(L, np.uint8)
    flags[(i < 0) | (i >= e_in.shape[0]) | (o < 0) | (o >= e_out.shape[0])] |= BAD_INDEX
    flags[r_is_bad(r, other, n1, n2)] |= BAD_R
    clean = np.flatnonzero(flags == 0)
    if clean.size:
        got, _ = mix_ref.reencrypt(N, q, h, r[clean], e_in, i[clean])
        want = mix_ref.gather_rows(e_out, o[clean], clean.size, q)
        flags[clean[(got.astype(np.int64) != want).any(axis=1)]] = MISMATCH
    return flags, int(np.count_nonzero(flags))


def open_links(side, src1, r1, src2, r2):
    """(left, right), each (in_idx, out_idx, r), ascending in the middle index j: a loop over the middle items."""
    side, src1, src2 = np.asarray(side), np.asarray(src1), np.asarray(src2)
    where = {int(j): k for k, j in enumerate(src2.tolist())}
    left, right = ([], [], []), ([], [], [])
    for j in range(len(side)):
        if side[j] == 0:
            left[0].append(int(src1[j])), left[1].append(j), left[2].append(np.asarray(r1)[j])
        else:
            k = where[j]
            right[0].append(j), right[1].append(k), right[2].append(np.asarray(r2)[k])
    pack = lambda t: (np.array(t[0], np.int64), np.array(t[1], np.int64), np.array(t[2]).reshape(len(t[0]), -1))
    return pack(left), pack(right)


def structure_ok(side, left, right):
    """The structural checks of an opening, as sets: True when it is well formed."""
    side = np.asarray(side)
    want_left = {j for j in range(len(side)) if side[j] == 0}
    want_right = set(range(len(side))) - want_left
    lo, ri = [int(x) for x in left[1]], [int(x) for x in right[0]]
    if set(lo) != want_left or len(lo) != len(want_left) or set(ri) != want_right or len(ri) != len(want_right):
        return False
    for links in (left, right):
        for idx in links[:2]:
            if len({int(x) for x in idx}) != len(idx):
                return False
    return True
