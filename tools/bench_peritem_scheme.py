#!/usr/bin/env python3
"""Per-item-key encrypt / decrypt (ntru_encrypt_peritem_batch_dev, ntru_decrypt_peritem_batch_dev), device-resident, beside what they are
measured against: the shared-key ntru_encrypt_batch_dev / ntru_decrypt_batch_dev and one ntru_polymul_split_dev over the same batch.  All
timings in one process, with HIP events after a warm-up, the calls alternating within every repeat (a drift of clocks or power hits all
of them alike); the median launch of each is reported as M items/s and as the fraction of the 8 TB/s HBM roof from ALGORITHMIC bytes
per item: per-item encrypt 8N (h, e, quotE 2N each; r, m N each), full-witness per-item decrypt 10N (e, quot1, rem1 2N each; f, fp,
value, quot2 N each), value-only per-item decrypt 5N, shared-key encrypt 6N, shared-key decrypt 8N, polymul 8N.  Operands are random
inside the symbol preconditions (no result is checked here: tests/test_peritem_scheme_gpu.py does that).
    python tools/bench_peritem_scheme.py [--reps 5] [--iters 10] [--json out.json]"""
import argparse
import json
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402

import __graft_entry__ as ge  # noqa: E402

HBM_PEAK_GBS = 8000.0
CONFIGS = [(821, 4096), (701, 8192)]
LOG_B = [18, 20]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5, help="alternating repeats (>= 3)")
    ap.add_argument("--iters", type=int, default=10, help="launches per timed call")
    ap.add_argument("--json", default=None)
    a = ap.parse_args()
    pkg = ge.load_package()
    eng = pkg.Engine(0)
    dev = torch.device("cuda:0")
    eng.set_stream(torch.cuda.current_stream().cuda_stream)
    results = []
    for N, q in CONFIGS:
        for lb in LOG_B:
            B = 1 << lb
            gen = torch.Generator(device=dev).manual_seed(N + lb)
            rnd = lambda hi, dt, shape=(B, N): torch.randint(0, hi, shape, generator=gen, device=dev, dtype=torch.int32).to(dt)
            h, r, m = rnd(q, torch.int16), rnd(3, torch.uint8), rnd(3, torch.uint8)
            f, fp = (rnd(3, torch.int8) - 1), rnd(3, torch.uint8)
            e16 = lambda: torch.empty((B, N), dtype=torch.int16, device=dev)
            e8 = lambda: torch.empty((B, N), dtype=torch.uint8, device=dev)
            e, qe, q1, r1, pq, pr = e16(), e16(), e16(), e16(), e16(), e16()
            v, q2 = e8(), e8()
            P = lambda t: t.data_ptr()
            calls = {
                "peritem_encrypt": (8, lambda: eng.encrypt_peritem_batch_dev(N, q, P(h), P(r), P(m), B, P(e), P(qe))),
                "peritem_decrypt": (10, lambda: eng.decrypt_peritem_batch_dev(N, q, 3, P(f), P(fp), P(e), B, P(v), P(q1), P(r1), P(q2))),
                "peritem_decrypt_value": (5, lambda: eng.decrypt_peritem_batch_dev(N, q, 3, P(f), P(fp), P(e), B, P(v))),
                "shared_encrypt": (6, lambda: eng.encrypt_batch_dev(N, q, P(h[0]), P(r), P(m), B, P(e), P(qe))),
                "shared_decrypt": (8, lambda: eng.decrypt_batch_dev(N, q, 3, P(f[0]), P(fp[0]), P(e), B, P(v), P(q1), P(r1), P(q2))),
                "polymul_split": (8, lambda: eng.polymul_split_dev(N, q, P(h), P(e), B, P(pq), P(pr))),
            }
            kernels = {}
            for name, (_, fn) in calls.items():          # warm-up (first launches, occupancy queries, clocks)
                for _ in range(3):
                    fn()
                kernels[name] = eng.last_kernel()
            torch.cuda.synchronize()
            ms = {name: [] for name in calls}
            for _ in range(max(3, a.reps)):
                for name, (_, fn) in calls.items():
                    t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                    t0.record()
                    for _ in range(a.iters):
                        fn()
                    t1.record()
                    torch.cuda.synchronize()
                    ms[name].append(t0.elapsed_time(t1) / a.iters)
            for name, (per, _) in calls.items():
                med = statistics.median(ms[name])
                gbs = per * N * B / (med * 1e-3) / 1e9
                row = {"N": N, "q": q, "B": B, "call": name, "kernel": kernels[name], "ms": round(med, 4),
                       "ms_spread": [round(min(ms[name]), 4), round(max(ms[name]), 4)], "M_items_per_s": round(B / med / 1e3, 1),
                       "algo_bytes_per_item": per * N, "hbm_frac": round(gbs / HBM_PEAK_GBS, 3)}
                results.append(row)
                print("N=%4d q=%5d B=2^%d  %-22s %-16s %8.3f ms  %7.1f M/s  %5.1f%% of HBM" % (
                    N, q, lb, name, kernels[name], med, row["M_items_per_s"], 100 * row["hbm_frac"]), flush=True)
            del h, r, m, f, fp, e, qe, q1, r1, pq, pr, v, q2
            torch.cuda.empty_cache()
    if a.json:
        with open(a.json, "w") as fh:
            json.dump(results, fh, indent=1)


if __name__ == "__main__":
    main()
