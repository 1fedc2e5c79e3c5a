#!/usr/bin/env python3
"""decryptBits in the two lift modes (ntru_engine_set_lift), device-resident, at the headline set N = 821, q = 4096, p = 3 with the golden
key and 2^20 rows: the ntru_decrypt_batch_dev launch (every witness array: k_decrypt_m8; value only: k_decrypt_m) and the round trip
encrypt + decrypt on r sampled on the device (what bench.py --sample-r times), each in reference and in centred mode, and for each mode how
many rows came back equal to their plaintext.  From the code: none in reference mode (-q = 2 mod 3 here, index.js:117 adds 1), all in
centred mode; and equal times, since the modes run the same kernels with one argument different.  The method of tools/bench_tally.py: one
process, HIP events after a warm-up, the calls alternating within every repeat, the median and the spread of the repeats reported.
    python tools/bench_lift.py [--reps 7] [--iters 5] [--log-rows 20] [--jsonl out.jsonl]"""
import argparse
import json
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np  # noqa: E402
import torch  # noqa: E402

import __graft_entry__ as ge  # noqa: E402

MODES = ("reference", "centred")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=7, help="alternating repeats (>= 3)")
    ap.add_argument("--iters", type=int, default=5, help="launches per timed call")
    ap.add_argument("--log-rows", type=int, default=20)
    ap.add_argument("--jsonl", default=None)
    a = ap.parse_args()
    pkg = ge.load_package()
    lift = pkg.lift
    eng = pkg.Engine(0)
    dev = torch.device("cuda:0")
    eng.set_stream(torch.cuda.current_stream().cuda_stream)
    with open(os.path.join(ge.ROOT, "tests", "golden", "scheme_n821_q4096.json")) as fh:
        gold = json.load(fh)
    o, key = gold["options"], gold["keys"][0]
    N, q, p, d = o["N"], o["q"], o["p"], o["dr"]
    B = 1 << a.log_rows
    pad = lambda x, dt: np.array(list(x) + [0] * (N - len(x)), dtype=dt)
    h = torch.from_numpy(pad(key["h"], np.uint16).view(np.int16)).to(dev)
    f, fp = torch.from_numpy(pad(key["f"], np.int8)).to(dev), torch.from_numpy(pad(key["fp"], np.uint8)).to(dev)
    gen = torch.Generator(device=dev).manual_seed(1)
    m = torch.randint(0, 2, (B, N), generator=gen, device=dev, dtype=torch.uint8)
    r = torch.empty((B, N), dtype=torch.uint8, device=dev)
    eng.sample_ternary_dev(N, d, d, p - 1, np.arange(8, dtype=np.uint32) * 0x9E3779B1 + 20240, 0, B, r.data_ptr())
    b16 = lambda: torch.empty((B, N), dtype=torch.int16, device=dev)
    b8 = lambda: torch.empty((B, N), dtype=torch.uint8, device=dev)
    e, quotE, value, q1, r1, q2 = b16(), b16(), b8(), b16(), b16(), b8()
    P = lambda t: t.data_ptr()

    def encrypt():
        eng.encrypt_batch_dev(N, q, P(h), P(r), P(m), B, P(e), P(quotE))

    def decrypt(witness=True):
        if witness:
            eng.decrypt_batch_dev(N, q, p, P(f), P(fp), P(e), B, P(value), P(q1), P(r1), P(q2))
        else:
            eng.decrypt_batch_dev(N, q, p, P(f), P(fp), P(e), B, P(value))

    def in_mode(mode, fn):
        def call():
            with lift.using(eng, mode):             # read when the call enqueues: set around the launch, nothing waits
                fn()
        return call

    encrypt()
    torch.cuda.synchronize()
    calls, kernels, equal = {}, {}, {}
    for mode in MODES:
        calls["decrypt, witness, " + mode] = in_mode(mode, decrypt)
        calls["decrypt, value only, " + mode] = in_mode(mode, lambda: decrypt(False))
        calls["round trip, " + mode] = in_mode(mode, lambda: (encrypt(), decrypt()))
    for name, fn in calls.items():
        for _ in range(3):
            fn()
        kernels[name] = eng.last_kernel()
        torch.cuda.synchronize()
        equal[name] = int((value == m).all(dim=1).sum().item())
    ms = {name: [] for name in calls}
    for _ in range(max(3, a.reps)):
        for name, fn in calls.items():
            t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            t0.record()
            for _ in range(a.iters):
                fn()
            t1.record()
            torch.cuda.synchronize()
            ms[name].append(t0.elapsed_time(t1) / a.iters)
    results = []
    for name in calls:
        med = statistics.median(ms[name])
        row = {"N": N, "q": q, "p": p, "rows": B, "call": name, "kernel": kernels[name], "ms": round(med, 4),
               "ms_spread": [round(min(ms[name]), 4), round(max(ms[name]), 4)], "M_rows_per_s": round(B / med / 1e3, 1),
               "rows_equal_to_plaintext": equal[name]}
        results.append(row)
        print("%-34s %-14s %8.4f ms  [%8.4f .. %8.4f]  %8.1f M rows/s  %8d of %d rows equal their plaintext"
              % (name, kernels[name], med, row["ms_spread"][0], row["ms_spread"][1], row["M_rows_per_s"], equal[name], B), flush=True)
    if a.jsonl:
        with open(a.jsonl, "w") as fh:
            for row in results:
                fh.write(json.dumps(row) + "\n")


if __name__ == "__main__":
    main()
