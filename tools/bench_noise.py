#!/usr/bin/env python3
"""The decryption noise of a batch under one key, measured with everything resident on one device, 2^20 rows at (N, q) = (821, 4096),
(509, 2048) and (701, 8192).  Arms, interleaved in the same run on the same device:
  noise       ntru_noise_batch_dev on kernel path 4 (k_noise_m, forced), peak and energy
  noise_peak  the same with energy NULL
  auto        the same call on kernel path 0: whatever the launcher's rule picks (the record names the kernel)
  composed    what a caller had before: ntru_decrypt_batch_dev with value and rem1, then the torch reduction of rem1 to the same two
              arrays on the same device (centre at q/2, max of the absolute values, sum of the squares in 64 bits)
  decrypt     value-only ntru_decrypt_batch_dev on the same rows: the yardstick (both products)
  packed      ntru_noise_packed_batch_dev on kernel path 0, on the same rows in the wire format
Device events around each arm, every arm warmed up first, min / median / max over the repeats.  The claim the records carry:
`noise` beats `composed` by more than composed's own max - min over the interleaved repeats (tools/bench_scan.py's rule).  Nothing is
checked here (tests/test_noise_gpu.py does that) and nothing is retried: any failure ends the run, and so does the time limit.
    python tools/bench_noise.py [--reps 5] [--log-b 20] [--arms noise,noise_peak,auto,composed,decrypt,packed] [--label text]
                                [--timeout 540] [--jsonl out.jsonl]"""
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
ARMS = ("noise", "noise_peak", "auto", "composed", "decrypt", "packed")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5, help="interleaved repeats (>= 3)")
    ap.add_argument("--log-b", type=int, default=20)
    ap.add_argument("--arms", default=",".join(ARMS))
    ap.add_argument("--timeout", type=int, default=540, help="seconds after which the run gives up")
    ap.add_argument("--label", default="working tree", help="what the records call the build that was measured")
    ap.add_argument("--jsonl", default=None)
    a = ap.parse_args()
    signal.signal(signal.SIGALRM, lambda *_: sys.exit("bench_noise: time limit of %d s reached" % a.timeout))
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
    results = []
    for N, q in SETS:
        d_e = torch.randint(0, q, (B, N), generator=gen, device=dev, dtype=torch.int32).to(torch.int16)
        d_f = (torch.randint(0, 3, (N,), generator=gen, device=dev, dtype=torch.int32) - 1).to(torch.int8)
        d_fp = torch.randint(0, 3, (N,), generator=gen, device=dev, dtype=torch.int32).to(torch.uint8)
        d_peak = torch.empty((B,), dtype=torch.int16, device=dev)
        d_energy = torch.empty((B,), dtype=torch.int64, device=dev)
        d_value = torch.empty((B, N), dtype=torch.uint8, device=dev)
        d_rem1 = torch.empty((B, N), dtype=torch.int16, device=dev) if "composed" in names else None
        d_packed = None
        if "packed" in names:
            os_ = eng.pack_params(q - 1, N)["outputSize"]
            d_packed = torch.empty((B, os_, 4), dtype=torch.int64, device=dev)
            eng._chk(eng._lib.ntru_pack_batch_dev(eng._h, q - 1, N, eng._dp(ptr(d_e)), B, eng._dp(ptr(d_packed))))
        torch.cuda.synchronize()
        kernels = {}

        def noise(name, path, energy):
            eng.set_kernel_path(path)
            pkg.noise_batch_dev(eng, N, q, ptr(d_f), ptr(d_e), B, ptr(d_peak), ptr(d_energy) if energy else None)
            kernels[name] = eng.last_kernel()

        def composed():
            eng.set_kernel_path(0)
            eng.decrypt_batch_dev(N, q, 3, ptr(d_f), ptr(d_fp), ptr(d_e), B, ptr(d_value), None, ptr(d_rem1), None)
            kernels["composed"] = eng.last_kernel() + " + torch"
            x = d_rem1.to(torch.int32)
            c = torch.where(x > q // 2, q - x, x)
            d_peak.copy_(c.amax(dim=1))
            d_energy.copy_((c * c).sum(dim=1, dtype=torch.int64))

        def decrypt():
            eng.set_kernel_path(0)
            eng.decrypt_batch_dev(N, q, 3, ptr(d_f), ptr(d_fp), ptr(d_e), B, ptr(d_value))
            kernels["decrypt"] = eng.last_kernel()

        def packed():
            eng.set_kernel_path(0)
            pkg.noise_packed_batch_dev(eng, N, q, ptr(d_f), ptr(d_packed), B, ptr(d_peak), ptr(d_energy))
            kernels["packed"] = "k_unpack_rows + " + eng.last_kernel()
        every = {"noise": lambda: noise("noise", 4, True), "noise_peak": lambda: noise("noise_peak", 4, False),
                 "auto": lambda: noise("auto", 0, True), "composed": composed, "decrypt": decrypt, "packed": packed}
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
            line += " %-10s %8.3f ms [%8.3f .. %8.3f] " % (n, med, min(ms[n]), max(ms[n]))
        if "noise" in arms and "composed" in arms:
            gain = rec["composed"]["ms"] - rec["noise"]["ms"]
            spread = rec["composed"]["ms_spread"][1] - rec["composed"]["ms_spread"][0]
            rec["composed_over_noise"] = round(rec["composed"]["ms"] / rec["noise"]["ms"], 3)
            rec["noise_beats_composed"] = bool(gain > spread)      # the gain against composed's own max - min
            line += " composed / noise = %.2f (gain %.3f ms against a spread of %.3f ms: %s)" % (
                rec["composed_over_noise"], gain, spread, "holds" if rec["noise_beats_composed"] else "does NOT hold")
        results.append(rec)
        print(line, flush=True)
        del d_e, d_value, d_rem1, d_packed
    if a.jsonl:
        with open(a.jsonl, "w") as fh:
            for r in results:
                fh.write(json.dumps(r) + "\n")
    signal.alarm(0)


if __name__ == "__main__":
    main()
