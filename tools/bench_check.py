#!/usr/bin/env python3
"""Rates of the witness checks (ntru_check_*_batch_dev) on honest engine-made witnesses, HIP events around the kernels.
    python tools/bench_check.py [--log-items 18] [--reps 20]
One JSON line per (template, N, q): items/s, the bytes a check must read (+ one flags byte) per second and that rate over the 8 TB/s
HBM peak.  Every item is checked to be accepted before it is timed."""
import argparse
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402

import __graft_entry__ as ge  # noqa: E402

HBM_PEAK = 8.0e12
ap = argparse.ArgumentParser()
ap.add_argument("--log-items", type=int, default=18)
ap.add_argument("--reps", type=int, default=20)
args = ap.parse_args()

pkg = ge.load_package()
eng = pkg.Engine(0)
dev = torch.device("cuda:0")
eng.set_stream(torch.cuda.current_stream().cuda_stream)
B = 1 << args.log_items


def nbits(mod, N):
    return (mod * mod * N - 1).bit_length()


def u16(shape, hi):
    return torch.randint(0, hi, shape, dtype=torch.int32, device=dev).to(torch.int16)


def pad(t):
    """[B][N] -> [B][N+1] int16 rows with a trailing 0 (the reference's expandArray)."""
    return torch.cat([t.to(torch.int16), torch.zeros((t.shape[0], 1), dtype=torch.int16, device=dev)], 1).contiguous()


def ternary(N, hi_val):
    t = torch.randint(0, 3, (B, N), dtype=torch.int32, device=dev)
    return torch.where(t == 2, torch.full_like(t, hi_val), t)


def timed(fn):
    for _ in range(3):
        fn()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(args.reps):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / args.reps / 1e3


def report(template, N, q, secs, bytes_per_item):
    print(json.dumps({"template": template, "N": N, "q": q, "items": B, "kernel": eng.last_kernel(), "ms": round(secs * 1e3, 4),
                      "items_per_s": round(B / secs), "bytes_per_item": bytes_per_item,
                      "bytes_per_s": round(B * bytes_per_item / secs), "hbm_roof": round(B * bytes_per_item / secs / HBM_PEAK, 4)}),
          flush=True)


for N, q in ((821, 4096), (701, 8192)):
    p, nq = 3, nbits(q, N)
    np_ = nbits(p, N)
    flags = torch.empty(B, dtype=torch.uint8, device=dev)
    P = lambda t: t.data_ptr()

    # VerifyEncrypt: r in {0,1,2}, m bits, one public key row per item
    h = u16((N,), q)
    r8 = torch.randint(0, 3, (B, N), dtype=torch.uint8, device=dev)
    m8 = torch.randint(0, 2, (B, N), dtype=torch.uint8, device=dev)
    e = torch.empty((B, N), dtype=torch.int16, device=dev)
    qe = torch.empty((B, N), dtype=torch.int16, device=dev)
    eng.encrypt_batch_dev(N, q, P(h), P(r8), P(m8), B, P(e), P(qe))
    r, m, hh, quotE, remE = r8.to(torch.int16), m8.to(torch.int16), h.expand(B, N).contiguous(), pad(qe), pad(e)
    enc = lambda: eng.check_encrypt_batch_dev(N, q, nq, P(r), P(m), P(hh), P(quotE), P(remE), B, P(flags))
    enc(); torch.cuda.synchronize()
    assert int(flags.max()) == 0, "VerifyEncrypt: an honest witness was rejected"
    report("VerifyEncrypt", N, q, timed(enc), 6 * N + 4 * (N + 1) + 1)

    # VerifyDecrypt: f in {0, 1, q-1} (one key), fp < p, the ciphertexts above
    f8 = torch.randint(-1, 2, (N,), dtype=torch.int8, device=dev)
    fp8 = torch.randint(0, p, (N,), dtype=torch.uint8, device=dev)
    value = torch.empty((B, N), dtype=torch.uint8, device=dev)
    q1 = torch.empty((B, N), dtype=torch.int16, device=dev)
    r1 = torch.empty((B, N), dtype=torch.int16, device=dev)
    q2 = torch.empty((B, N), dtype=torch.uint8, device=dev)
    eng.decrypt_batch_dev(N, q, p, P(f8), P(fp8), P(e), B, P(value), P(q1), P(r1), P(q2))
    f, fp = torch.remainder(f8.to(torch.int32), q).to(torch.int16).expand(B, N).contiguous(), fp8.to(torch.int16).expand(B, N).contiguous()
    Q1, R1, Q2, R2 = pad(q1), pad(r1), pad(q2), pad(value)
    dec = lambda: eng.check_decrypt_batch_dev(N, q, nq, p, np_, P(f), P(fp), P(e), P(Q1), P(R1), P(Q2), P(R2), B, P(flags))
    dec(); torch.cuda.synchronize()
    assert int(flags.max()) == 0, "VerifyDecrypt: an honest witness was rejected"
    report("VerifyDecrypt", N, q, timed(dec), 6 * N + 8 * (N + 1) + 1)

    # VerifyInverse (the fq case's shape): f in {0, 1, q-1}, fq < q, per item; quotient / remainder from the engine's product + split
    del r8, m8, value, q2
    fi = ternary(N, q - 1).to(torch.int16)
    fqi = u16((B, N), q)
    qi = torch.empty((B, N), dtype=torch.int16, device=dev)
    ri = torch.empty((B, N), dtype=torch.int16, device=dev)
    eng.polymul_split_dev(N, q, P(fi), P(fqi), B, P(qi), P(ri))
    QI, RI = pad(qi), pad(ri)
    inv = lambda: eng.check_inverse_batch_dev(N, q, nq, P(fi), P(fqi), P(QI), P(RI), B, P(flags))
    inv(); torch.cuda.synchronize()
    assert int(flags.max()) == 0, "VerifyInverse: an honest witness was rejected"
    report("VerifyInverse", N, q, timed(inv), 4 * N + 4 * (N + 1) + 1)
    del fi, fqi, qi, ri, QI, RI, r, m, hh, quotE, remE, f, fp, Q1, R1, Q2, R2, e, qe, q1, r1
    torch.cuda.empty_cache()
