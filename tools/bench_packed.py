#!/usr/bin/env python3
"""Sums of packed ciphertexts (ntru_sum_groups_packed_dev), device-resident, beside the only way to sum packed rows on the device without
it: ntru_unpack_batch_dev into rows of arr_len coefficients, then ntru_sum_groups_dev run at N = arr_len.  N = 821, q = 4096
(bits 12, 21 fields per element, 40 elements = 1280 bytes per row; arr_len 840), 2^20 rows, for K = 16 and for one group.  The method of
tools/bench_tally.py: one process, HIP events after a warm-up, the calls alternating within every repeat, the median reported as ms,
rows/s and achieved bytes/s over the 1280 packed bytes per row (the detour moves 1280 + 2 x 1680 more).  No result is checked here:
tests/test_packed_ciphertexts_gpu.py does that.
    python tools/bench_packed.py [--what both|baseline|packed] [--reps 7] [--iters 5] [--jsonl out.jsonl]
--what baseline uses nothing of the packed calls: a copy of this file runs it in a checkout from before they existed, for
alternating processes."""
import argparse
import json
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402

import __graft_entry__ as ge  # noqa: E402

N, Q, LOG_B = 821, 4096, 20


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--what", choices=("both", "baseline", "packed"), default="both")
    ap.add_argument("--reps", type=int, default=7, help="alternating repeats (>= 3)")
    ap.add_argument("--iters", type=int, default=5, help="launches per timed call")
    ap.add_argument("--jsonl", default=None)
    a = ap.parse_args()
    pkg = ge.load_package()
    eng = pkg.Engine(0)
    dev = torch.device("cuda:0")
    eng.set_stream(torch.cuda.current_stream().cuda_stream)
    B = 1 << LOG_B
    pr = eng.pack_params(Q - 1, N)
    bits, per, arr_len, os_ = pr["maxInputBits"], pr["numInputsPerOutput"], pr["arrLen"], pr["outputSize"]
    row_bytes = 32 * os_
    gen = torch.Generator(device=dev).manual_seed(1)
    rows = torch.randint(0, Q, (B, N), generator=gen, device=dev, dtype=torch.int32).to(torch.int16)
    packed = torch.empty((B, os_, 4), dtype=torch.int64, device=dev)
    P = lambda t: t.data_ptr()
    dp = eng._dp
    eng._chk(eng._lib.ntru_pack_batch_dev(eng._h, Q - 1, N, dp(P(rows)), B, dp(P(packed))))
    torch.cuda.synchronize()
    del rows
    wide = torch.empty((B, arr_len), dtype=torch.int16, device=dev) if a.what != "packed" else None
    out = torch.empty((B // 16, arr_len), dtype=torch.int16, device=dev)

    def detour(K):
        eng._chk(eng._lib.ntru_unpack_batch_dev(eng._h, Q - 1, per * bits, dp(P(packed)), os_, B, dp(P(wide))))
        eng.sum_groups_dev(arr_len, Q, P(wide), P(out), B // K, K=K)

    calls = {}
    for K in (16, B):
        if a.what != "packed":
            calls["unpack + sum_groups K=%d" % K] = lambda K=K: detour(K)
        if a.what != "baseline":
            calls["sum_groups_packed K=%d" % K] = lambda K=K: pkg.sum_groups_packed_dev(eng, N, Q, P(packed), P(out), B // K, K=K)
    kernels = {}
    for name, fn in calls.items():
        for _ in range(3):
            fn()
        kernels[name] = ("k_unpack + " if name.startswith("unpack") else "") + eng.last_kernel()
    torch.cuda.synchronize()
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
        row = {"N": N, "q": Q, "rows": B, "call": name, "kernel": kernels[name], "ms": round(med, 4),
               "ms_spread": [round(min(ms[name]), 4), round(max(ms[name]), 4)], "G_rows_per_s": round(B / med / 1e6, 3),
               "packed_bytes": row_bytes * B, "packed_TB_per_s": round(row_bytes * B / (med * 1e-3) / 1e12, 3)}
        results.append(row)
        print("%-32s %-38s %8.3f ms  %7.3f G rows/s  %6.3f TB/s over %d bytes per row" % (name, kernels[name], med, row["G_rows_per_s"],
                                                                                         row["packed_TB_per_s"], row_bytes), flush=True)
    if a.what == "both":
        for K in (16, B):
            base = next(r for r in results if r["call"] == "unpack + sum_groups K=%d" % K)
            new = next(r for r in results if r["call"] == "sum_groups_packed K=%d" % K)
            print("K = %d: detour %.3f ms / packed %.3f ms = %.2fx (slowest packed repeat %.3f ms, fastest detour repeat %.3f ms)"
                  % (K, base["ms"], new["ms"], base["ms"] / new["ms"], new["ms_spread"][1], base["ms_spread"][0]))
    if a.jsonl:
        with open(a.jsonl, "w") as fh:
            for r in results:
                fh.write(json.dumps(r) + "\n")


if __name__ == "__main__":
    main()
