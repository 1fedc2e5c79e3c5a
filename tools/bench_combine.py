#!/usr/bin/env python3
"""Combining ciphertexts by a weight matrix, measured at N = 821, q = 4096 with rows and weights resident on one device, for
B = 2^20 and 2^16 rows and G = 1, 3, 16, 32, 64, 256 outputs.  Three arms, interleaved in the same run on the same device:
  m     ntru_combine_batch_dev on kernel path 0 (k_combine_m, the int8 matrix cores)
  v     the same on kernel path 1 (k_combine_v, the vector ALU)
  sums  what there was before: G calls of ntru_sum_groups_dev (K = B, one group), each with a contiguous weight column that was
        prepared outside the timed region
Device events around each arm, every arm warmed up first, min / median / max over the repeats; beside the times, the bytes of `rows`
read ONCE per second against the 8 TB/s HBM roof of bench.py --full (for an arm that reads the rows G times this is 1 / G of its
traffic: the figure says what the call is worth, not what the kernel moves).  Nothing is checked here (tests/test_combine_gpu.py does
that) and nothing is retried: any failure ends the run, and so does the time limit.
    python tools/bench_combine.py [--reps 7] [--timeout 540] [--jsonl out.jsonl]"""
import argparse
import json
import os
import signal
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402

import __graft_entry__ as ge  # noqa: E402

N, Q = 821, 4096
HBM_PEAK_GBS = 8000.0          # bench.py
LOG_BS = (20, 16)
GS = (1, 3, 16, 32, 64, 256)


def clock_mhz():
    try:
        return int(torch.cuda.clock_rate())
    except Exception:
        return None


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=7, help="interleaved repeats (>= 5)")
    ap.add_argument("--timeout", type=int, default=540, help="seconds after which the run gives up")
    ap.add_argument("--jsonl", default=None)
    a = ap.parse_args()
    signal.signal(signal.SIGALRM, lambda *_: sys.exit("bench_combine: time limit of %d s reached" % a.timeout))
    signal.alarm(a.timeout)
    reps = max(5, a.reps)
    pkg = ge.load_package()
    eng = pkg.Engine(0)
    dev = torch.device("cuda:0")
    eng.set_stream(torch.cuda.current_stream().cuda_stream)
    props = torch.cuda.get_device_properties(0)
    report = {"device": props.name, "cus": props.multi_processor_count, "N": N, "q": Q}
    print("%s, %d CUs; shader clock before / after each table is printed where the driver reports it" % (props.name, report["cus"]))
    gen = torch.Generator(device=dev).manual_seed(1)
    ptr = lambda t: t.data_ptr()
    results = []
    for log_b in LOG_BS:
        B = 1 << log_b
        d_rows = torch.randint(0, Q, (B, N), generator=gen, device=dev, dtype=torch.int32).to(torch.int16)
        row_bytes = 2.0 * N * B
        print("B = 2^%d rows (%.1f MB of rows), clock %s MHz" % (log_b, row_bytes / 1e6, clock_mhz()))
        for G in GS:
            d_w = torch.randint(0, Q, (B, G), generator=gen, device=dev, dtype=torch.int32).to(torch.int16)
            d_cols = d_w.t().contiguous()                                   # [G][B]: one contiguous weight column per output
            d_out = torch.empty((G, N), dtype=torch.int16, device=dev)
            torch.cuda.synchronize()
            kernels = {}

            def combine(path):
                eng.set_kernel_path(path)
                pkg.combine_batch_dev(eng, N, Q, ptr(d_rows), ptr(d_w), B, G, ptr(d_out))
                kernels[path] = eng.last_kernel()

            def sums():
                eng.set_kernel_path(0)
                for g in range(G):
                    eng.sum_groups_dev(N, Q, ptr(d_rows), ptr(d_out) + 2 * N * g, 1, K=B, d_weights=ptr(d_cols) + 2 * B * g)
            arms = {"m": lambda: combine(0), "v": lambda: combine(1), "sums": sums}
            for fn in arms.values():
                fn()
                fn()
            torch.cuda.synchronize()
            ms = {name: [] for name in arms}
            for _ in range(reps):
                for name, fn in arms.items():
                    t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                    t0.record()
                    fn()
                    t1.record()
                    torch.cuda.synchronize()
                    ms[name].append(t0.elapsed_time(t1))
            eng.set_kernel_path(0)
            rec = dict(report, items=B, G=G, clock_mhz=clock_mhz(), kernels={"m": kernels[0], "v": kernels[1]})
            line = "  G = %3d " % G
            for name in arms:
                med = statistics.median(ms[name])
                gbs = row_bytes / (med * 1e-3) / 1e9
                rec[name] = {"ms": round(med, 4), "ms_spread": [round(min(ms[name]), 4), round(max(ms[name]), 4)],
                             "rows_once_GBs": round(gbs, 1), "rows_once_frac_of_hbm": round(gbs / HBM_PEAK_GBS, 4)}
                line += " %-4s %9.3f ms [%9.3f .. %9.3f] %7.1f GB/s (%4.1f %%) " % (name, med, min(ms[name]), max(ms[name]), gbs,
                                                                                  100 * gbs / HBM_PEAK_GBS)
            rec["m_over_sums"] = round(statistics.median(ms["sums"]) / statistics.median(ms["m"]), 3)
            results.append(rec)
            print(line + " sums / m = %.2f" % rec["m_over_sums"], flush=True)
            del d_w, d_cols, d_out
        del d_rows
    if a.jsonl:
        with open(a.jsonl, "w") as fh:
            for r in results:
                fh.write(json.dumps(r) + "\n")
    signal.alarm(0)


if __name__ == "__main__":
    main()
