#!/usr/bin/env python3
"""A batch times one shared full-range polynomial, measured with everything resident on one device, 2^20 rows at (N, q) = (821, 4096),
(509, 2048) and (701, 8192).  Arms, interleaved in the same run on the same device:
  shared      ntru_mul_shared_batch_dev on kernel path 4 (k_mul_shared_m, forced), quotient and remainder
  shared_rem  the same without the quotient
  auto        the same call on kernel path 0: whatever the launcher's rule picks (the record names the kernel)
  peritem     what there was before: ntru_polymul_split_dev on s replicated per row (the replication is outside the timed region)
  decrypt     value-only ntru_decrypt_batch_dev on the same rows: the shared-key yardstick (as many matrix instructions per row block)
Device events around each arm, every arm warmed up first, min / median / max over the repeats.  --arms restricts the run, so that
NTRU_ENGINE_LIB=<another build> can supply the arms that exist there (peritem, decrypt) from the code as it was.  Nothing is checked here
(tests/test_mulshared_gpu.py does that) and nothing is retried: any failure ends the run, and so does the time limit.
    python tools/bench_mulshared.py [--reps 5] [--log-b 20] [--arms shared,shared_rem,auto,peritem,decrypt] [--label text] [--timeout 540]
                                    [--jsonl out.jsonl]"""
import argparse
import json
import os
import signal
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402

import __graft_entry__ as ge  # noqa: E402

SETS = ((821, 4096), (509, 2048), (701, 8192))
ARMS = ("shared", "shared_rem", "auto", "peritem", "decrypt")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5, help="interleaved repeats (>= 3)")
    ap.add_argument("--log-b", type=int, default=20)
    ap.add_argument("--arms", default=",".join(ARMS))
    ap.add_argument("--timeout", type=int, default=540, help="seconds after which the run gives up")
    ap.add_argument("--label", default="working tree", help="what the records call the build that was measured")
    ap.add_argument("--jsonl", default=None)
    a = ap.parse_args()
    signal.signal(signal.SIGALRM, lambda *_: sys.exit("bench_mulshared: time limit of %d s reached" % a.timeout))
    signal.alarm(a.timeout)
    reps, B = max(3, a.reps), 1 << a.log_b
    names = [n for n in a.arms.split(",") if n]
    assert set(names) <= set(ARMS), names
    pkg = ge.load_package()
    eng = pkg.Engine(0)
    dev = torch.device("cuda:0")
    eng.set_stream(torch.cuda.current_stream().cuda_stream)
    props = torch.cuda.get_device_properties(0)
    report = {"device": props.name, "cus": props.multi_processor_count, "build": a.label, "items": B}
    print("%s, %d CUs, library %s, B = 2^%d" % (props.name, report["cus"], pkg.library_path(), a.log_b))
    gen = torch.Generator(device=dev).manual_seed(1)
    ptr = lambda t: t.data_ptr()
    u16 = lambda shape, hi: torch.randint(0, hi, shape, generator=gen, device=dev, dtype=torch.int32).to(torch.int16)
    results = []
    for N, q in SETS:
        d_rows, d_s = u16((B, N), q), u16((N,), q)
        d_srep = d_s.repeat(B, 1).contiguous() if "peritem" in names else None
        d_quot, d_rem = (torch.empty((B, N), dtype=torch.int16, device=dev) for _ in range(2))
        d_f = (torch.randint(0, 3, (N,), generator=gen, device=dev, dtype=torch.int32) - 1).to(torch.int8)
        d_fp = torch.randint(0, 3, (N,), generator=gen, device=dev, dtype=torch.int32).to(torch.uint8)
        d_value = torch.empty((B, N), dtype=torch.uint8, device=dev)
        torch.cuda.synchronize()
        kernels = {}

        def shared(name, path, quot):
            eng.set_kernel_path(path)
            pkg.mul_shared_batch_dev(eng, N, q, ptr(d_s), ptr(d_rows), B, ptr(d_quot) if quot else None, ptr(d_rem))
            kernels[name] = eng.last_kernel()

        def peritem():
            eng.set_kernel_path(0)
            eng.polymul_split_dev(N, q, ptr(d_rows), ptr(d_srep), B, ptr(d_quot), ptr(d_rem))
            kernels["peritem"] = eng.last_kernel()

        def decrypt():
            eng.set_kernel_path(0)
            eng.decrypt_batch_dev(N, q, 3, ptr(d_f), ptr(d_fp), ptr(d_rows), B, ptr(d_value))
            kernels["decrypt"] = eng.last_kernel()
        every = {"shared": lambda: shared("shared", 4, True), "shared_rem": lambda: shared("shared_rem", 4, False),
                 "auto": lambda: shared("auto", 0, True), "peritem": peritem, "decrypt": decrypt}
        arms = {n: every[n] for n in names}
        for fn in arms.values():
            fn()
            fn()
        torch.cuda.synchronize()
        ms = {n: [] for n in arms}
        for _ in range(reps):
            for n, fn in arms.items():
                t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                t0.record()
                fn()
                t1.record()
                torch.cuda.synchronize()
                ms[n].append(t0.elapsed_time(t1))
        eng.set_kernel_path(0)
        rec = dict(report, N=N, q=q, kernels=kernels)
        line = "N = %4d q = %4d " % (N, q)
        for n in arms:
            med = statistics.median(ms[n])
            rec[n] = {"ms": round(med, 4), "ms_spread": [round(min(ms[n]), 4), round(max(ms[n]), 4)], "Mrows_per_s": round(B / med / 1e3, 1)}
            line += " %-10s %8.3f ms [%8.3f .. %8.3f] %6.1f M rows/s " % (n, med, min(ms[n]), max(ms[n]), B / med / 1e3)
        if "shared" in arms and "peritem" in arms:
            rec["peritem_over_shared"] = round(rec["peritem"]["ms"] / rec["shared"]["ms"], 3)
            line += " peritem / shared = %.2f" % rec["peritem_over_shared"]
        results.append(rec)
        print(line, flush=True)
        del d_rows, d_srep, d_quot, d_rem, d_value
    if a.jsonl:
        with open(a.jsonl, "w") as fh:
            for r in results:
                fh.write(json.dumps(r) + "\n")
    signal.alarm(0)


if __name__ == "__main__":
    main()
