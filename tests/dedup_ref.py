"""Reference of "removing duplicates" (include/ntru_engine.h) in numpy, without the engine and without a sort of its own: numpy.unique over
the prior and the new rows together, reduced modulo `mod`; packed rows go through packed_ref.unpack_rows first.  Also the row
families the tests plant, and the fixture the Node shim and NTRU.dedupBatch run on."""
import json
import os

import numpy as np

import packed_ref

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "dedup_cases.json")


def want(mod, rows, prior=None):
    """(first [B] int64, unique int64) for dense rows [B][N] and prior [S][N] (or None): first = index[inverse] of numpy.unique over
    the S + B reduced rows."""
    rows = np.asarray(rows, np.int64)
    B, N = rows.shape
    prior = np.zeros((0, N), np.int64) if prior is None else np.asarray(prior, np.int64).reshape(-1, N)
    S = prior.shape[0]
    if B == 0:
        return np.zeros(0, np.int64), np.zeros(0, np.int64)
    both = (np.concatenate([prior, rows]) % mod).astype(np.uint16 if mod <= 65536 else np.int64)
    _, index, inverse = np.unique(both, axis=0, return_index=True, return_inverse=True)
    first = index[np.asarray(inverse).reshape(-1)][S:].astype(np.int64)
    unique = np.nonzero(first == S + np.arange(B))[0].astype(np.int64)
    return first, unique


def want_packed(mod, N, packed, prior=None):
    """The same for rows in the wire format: uint64 [.][os][4]."""
    os_ = packed_ref.params(mod - 1, N)[3]
    packed = np.asarray(packed, np.uint64).reshape(-1, os_, 4)
    up = None if prior is None else packed_ref.unpack_rows(mod, N, prior)
    return want(mod, packed_ref.unpack_rows(mod, N, packed) if packed.shape[0] else np.zeros((0, N), np.uint16), up)


def by_dictionary(mod, rows, prior=None):
    """first and unique from a plain dictionary: the reduced row -> the index that saw it first."""
    seen, first = {}, []
    S = 0 if prior is None else len(prior)
    for i, row in enumerate(list([] if prior is None else prior) + list(rows)):
        key = tuple(int(c) % mod for c in row)
        seen.setdefault(key, i)
        if i >= S:
            first.append(seen[key])
    return first, [b for b, f in enumerate(first) if f == S + b]


def family_rows(rng, N, mod, B):
    """B dense rows (uint16, raw values below 65536) that mix the families: distinct random rows, the all-zero row, adjacent copies,
    copies at b and B - 1 - b, copies with mod or 2 mod added to some coefficients, rows that differ by 1 in the first or in the last
    coefficient only, cyclic rotations and coefficient permutations of one row."""
    rows = rng.integers(0, mod, (B, N)).astype(np.int64)
    if B >= 2:
        rows[B // 2] = 0
    base = rows[0].copy()
    b = np.arange(B)
    kind = np.where(b > 0, b % 11, 0)
    at = lambda k: np.nonzero(kind == k)[0]
    i = at(3)                                                              # the same row modulo mod: mod or 2 mod added
    cand = base + rng.integers(0, 3, (len(i), N)) * mod
    rows[i] = np.where(cand < 65536, cand, base)
    i = at(4)                                                              # differs in the first coefficient only
    rows[i] = base
    rows[i, 0] = (base[0] + 1) % mod
    i = at(5)                                                              # differs in the last coefficient only
    rows[i] = base
    rows[i, N - 1] = (base[N - 1] + 1) % mod
    i = at(6)                                                              # rotations
    rows[i] = base[(np.arange(N)[None, :] - (1 + i % max(N - 1, 1))[:, None]) % N]
    i = at(7)                                                              # permutations of the coefficients
    rows[i] = rng.permuted(np.tile(base, (len(i), 1)), axis=1)
    rows[at(8)] = 0                                                        # the all-zero row again
    i = at(1)                                                              # adjacent copies (of a random row: kind 0)
    rows[i] = rows[i - 1]
    i = at(2)                                                              # copies at b and B - 1 - b
    rows[i] = rows[B - 1 - i]
    return rows.astype(np.uint16)


def load_cases():
    with open(GOLDEN) as fh:
        return json.load(fh)["cases"]
