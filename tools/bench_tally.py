#!/usr/bin/env python3
"""Sums of ciphertexts in groups (ntru_sum_groups_dev), device-resident, beside what they are measured against, at N = 821, q = 4096 and
2^20 rows: (a) the new call for G = 1 / G = 2^14 (K = 64) / G = 2^18 (K = 4), with and without weights; (b) ntru_add_batch_dev on 2^20
rows, the streaming yardstick of this device; (c) the fold a caller had to write before -- log2 K passes of ntru_add_batch_dev over the
halves of the array -- for the G = 1 case.  All timings in one process with HIP events after a warm-up, the calls alternating within
every repeat; the median is reported as ms, rows/s and achieved bytes/s over the ALGORITHMIC bytes 2 N B + 2 N G (weights add 2 B; add:
6 N B; the fold is rated on the same 2 N B + 2 N as the call it replaces, and on the bytes it really moves).  No result is checked here:
tests/test_ciphertext_sum_gpu.py does that.
    python tools/bench_tally.py [--reps 7] [--iters 5] [--jsonl out.jsonl]"""
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
    ap.add_argument("--reps", type=int, default=7, help="alternating repeats (>= 3)")
    ap.add_argument("--iters", type=int, default=5, help="launches per timed call")
    ap.add_argument("--jsonl", default=None)
    a = ap.parse_args()
    pkg = ge.load_package()
    eng = pkg.Engine(0)
    dev = torch.device("cuda:0")
    eng.set_stream(torch.cuda.current_stream().cuda_stream)
    B = 1 << LOG_B
    gen = torch.Generator(device=dev).manual_seed(1)
    rows = torch.randint(0, Q, (B, N), generator=gen, device=dev, dtype=torch.int32).to(torch.int16)
    other = torch.randint(0, Q, (B, N), generator=gen, device=dev, dtype=torch.int32).to(torch.int16)
    w = torch.randint(0, Q, (B,), generator=gen, device=dev, dtype=torch.int32).to(torch.int16)
    out = torch.empty((B, N), dtype=torch.int16, device=dev)
    fold_buf = torch.empty((B // 2, N), dtype=torch.int16, device=dev)
    P = lambda t: t.data_ptr()

    def fold():
        """rows -> fold_buf[: B / 2] -> ... -> fold_buf[0]: pass k adds the two halves of what pass k - 1 left."""
        src, n = rows, B
        while n > 1:
            n //= 2
            eng.add_batch_dev(N, Q, P(src), P(src) + 2 * N * n, n, P(fold_buf))
            src = fold_buf

    calls = {}
    for G in (1, 1 << 14, 1 << 18):
        K = B // G
        for weighted in (False, True):
            name = "sum_groups G=%d K=%d%s" % (G, K, " weighted" if weighted else "")
            calls[name] = (2 * N * B + 2 * N * G + (2 * B if weighted else 0), None,
                           (lambda G=G, K=K, weighted=weighted: eng.sum_groups_dev(N, Q, P(rows), P(out), G, K=K, d_weights=P(w) if weighted else None)))
    calls["add_batch 2^20 rows"] = (6 * N * B, None, lambda: eng.add_batch_dev(N, Q, P(rows), P(other), B, P(out)))
    calls["fold of add_batch G=1"] = (2 * N * B + 2 * N, 6 * N * (B - 1), fold)
    kernels = {}
    for name, (_, _, fn) in calls.items():
        for _ in range(3):
            fn()
        kernels[name] = eng.last_kernel() if name.startswith("sum_groups") else "k_add_mod_vec"
    torch.cuda.synchronize()
    ms = {name: [] for name in calls}
    for _ in range(max(3, a.reps)):
        for name, (_, _, fn) in calls.items():
            t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            t0.record()
            for _ in range(a.iters):
                fn()
            t1.record()
            torch.cuda.synchronize()
            ms[name].append(t0.elapsed_time(t1) / a.iters)
    results = []
    for name, (algo, moved, _) in calls.items():
        med = statistics.median(ms[name])
        row = {"N": N, "q": Q, "rows": B, "call": name, "kernel": kernels[name], "ms": round(med, 4),
               "ms_spread": [round(min(ms[name]), 4), round(max(ms[name]), 4)], "G_rows_per_s": round(B / med / 1e6, 3),
               "algo_bytes": algo, "algo_TB_per_s": round(algo / (med * 1e-3) / 1e12, 3)}
        if moved:
            row["moved_bytes"] = moved
            row["moved_TB_per_s"] = round(moved / (med * 1e-3) / 1e12, 3)
        results.append(row)
        print("%-34s %-22s %8.3f ms  %7.3f G rows/s  %6.3f TB/s algorithmic" % (name, kernels[name], med, row["G_rows_per_s"],
                                                                               row["algo_TB_per_s"]), flush=True)
    base = next(r for r in results if r["call"].startswith("fold"))["ms"]
    new = next(r for r in results if r["call"] == "sum_groups G=1 K=%d" % B)["ms"]
    print("G = 1: fold %.3f ms / sum_groups %.3f ms = %.2fx" % (base, new, base / new))
    if a.jsonl:
        with open(a.jsonl, "w") as fh:
            for r in results:
                fh.write(json.dumps(r) + "\n")


if __name__ == "__main__":
    main()
