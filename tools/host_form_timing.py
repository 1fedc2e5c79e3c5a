#!/usr/bin/env python3
"""Wall time of the host-pointer forms ntru_encrypt_batch / ntru_decrypt_batch (all witness arrays) at N = 821, q = 4096 for a
single item and for 2^18 items, pageable and pinned arrays: the median of the calls after a warm-up, one JSON line per case.
NTRU_ENGINE_LIB selects the build, so two builds are compared by running this alternately, one process per run."""
import ctypes as C
import json
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import __graft_entry__ as ge  # noqa: E402
import bench  # noqa: E402

pkg = ge.load_package()
eng = pkg.Engine(0)
lib, H = eng._lib, eng._h
o, h, f, fp = bench.load_key("n821_q4096")
N, q, p = o["N"], o["q"], o["p"]
P = lambda a: a.ctypes.data_as(C.c_void_p)


def array(n, dt, pin):
    if not pin:
        return np.zeros(n, dt)
    nbytes = n * np.dtype(dt).itemsize
    a = np.ctypeslib.as_array((C.c_uint8 * nbytes).from_address(lib.ntru_host_alloc(nbytes))).view(dt)
    a[:] = 0
    return a


def median_ms(call, warm, reps):
    times = []
    for k in range(warm + reps):
        t0 = time.perf_counter()
        rc = call()
        dt = time.perf_counter() - t0
        assert rc == 0, lib.ntru_last_error().decode()
        if k >= warm:
            times.append(dt * 1e3)
    return statistics.median(times)


for B, warm, reps in ((1, 50, 500), (1 << 18, 2, 7)):
    for pin in (False, True):
        rng = np.random.default_rng(5)
        r, m = array(B * N, np.uint8, pin), array(B * N, np.uint8, pin)
        r[:] = rng.integers(0, 3, B * N, dtype=np.uint8)
        m[:] = rng.integers(0, 2, B * N, dtype=np.uint8)
        e, quotE, q1, r1 = (array(B * N, np.uint16, pin) for _ in range(4))
        value, q2 = array(B * N, np.uint8, pin), array(B * N, np.uint8, pin)
        enc = median_ms(lambda: lib.ntru_encrypt_batch(H, N, q, P(h), P(r), P(m), B, P(e), P(quotE)), warm, reps)
        dec = median_ms(lambda: lib.ntru_decrypt_batch(H, N, q, p, P(f), P(fp), P(e), B, P(value), P(q1), P(r1), P(q2)), warm, reps)
        print(json.dumps({"lib": os.path.basename(os.path.dirname(pkg.library_path())), "B": B, "pinned": pin,
                          "encrypt_ms": round(enc, 4), "decrypt_ms": round(dec, 4), "check": int(value.sum()) ^ int(e[:N].sum())}))
