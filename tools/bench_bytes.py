#!/usr/bin/env python3
"""Byte messages as packed bits, measured at N = 821, q = 4096, nbytes = 102 and 2^20 blocks on one device:
  (a) the two codec kernels (ntru_bytes_to_rows_dev, ntru_rows_to_bytes_dev) in TB/s over the bytes they must move, beside
      ntru_add_batch_dev on 2^20 rows, the streaming yardstick of this device, in the same run;
  (b) ntru_encrypt_bytes_batch_dev / ntru_decrypt_bytes_batch_dev against ntru_encrypt_batch_dev (e only) / value-only
      ntru_decrypt_batch_dev on pre-expanded rows: what the expansion and the collection cost on top of the scheme kernels;
  (c) host arrays in and out: ntru_pipeline_bytes_batch (msg in, msg_out + flags out) against ntru_pipeline_batch (m in, value out) with
      the same sampler key, decrypt on, value only -- 2 x 102 (+ 1) bytes per item over the bus against 2 x 821 -- with pinned and with
      pageable host arrays.
(a) and (b) are timed with device events, (c) with the host clock around calls that return synchronised; every call is warmed up first
and the calls of a group alternate within every repeat; the median and the spread over the repeats are reported.  Nothing is checked
here (tests/test_message_bytes_gpu.py does that) and nothing is retried: any failure ends the run, and so does the time limit.
    python tools/bench_bytes.py [--reps 7] [--iters 5] [--log-b 20] [--timeout 540] [--jsonl out.jsonl]"""
import argparse
import ctypes
import json
import os
import signal
import statistics
import subprocess
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np  # noqa: E402
import torch  # noqa: E402

import __graft_entry__ as ge  # noqa: E402

N, Q, P_MOD = 821, 4096, 3
W = N // 8


def device_report():
    props = torch.cuda.get_device_properties(0)
    rep = {"device": props.name, "cus": props.multi_processor_count}
    try:                                                     # read-only query; absent tool or odd output is not an error of the benchmark
        out = subprocess.run(["rocm-smi", "--showclocks"], capture_output=True, text=True, timeout=30).stdout
        rep["clocks"] = [ln.strip() for ln in out.splitlines() if "GPU[0]" in ln and ("sclk" in ln or "mclk" in ln or "fclk" in ln)]
    except (OSError, subprocess.SubprocessError):
        rep["clocks"] = "not read"
    return rep


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=7, help="alternating repeats (>= 3)")
    ap.add_argument("--iters", type=int, default=5, help="launches per timed device call")
    ap.add_argument("--log-b", type=int, default=20)
    ap.add_argument("--timeout", type=int, default=540, help="seconds after which the run gives up")
    ap.add_argument("--jsonl", default=None)
    a = ap.parse_args()
    signal.signal(signal.SIGALRM, lambda *_: sys.exit("bench_bytes: time limit of %d s reached" % a.timeout))
    signal.alarm(a.timeout)
    reps = max(3, a.reps)
    pkg = ge.load_package()
    eng = pkg.Engine(0)
    dev = torch.device("cuda:0")
    eng.set_stream(torch.cuda.current_stream().cuda_stream)
    report = device_report()
    B = 1 << a.log_b
    with open(os.path.join(ge.ROOT, "tests", "golden", "scheme_n821_q4096.json")) as fh:
        gold = json.load(fh)
    k, dr = gold["keys"][0], gold["options"]["dr"]
    pad = lambda v, dt: np.array(list(v) + [0] * (N - len(v)), dtype=dt)
    h, f, fp = pad(k["h"], np.uint16), pad(k["f"], np.int8), pad(k["fp"], np.uint8)
    key = np.arange(1, 9, dtype=np.uint32) * 0x9E3779B1
    gen = torch.Generator(device=dev).manual_seed(1)
    ptr = lambda t: t.data_ptr()
    d_h, d_f, d_fp = (torch.from_numpy(x.view(np.uint8)).to(dev) for x in (h, f, fp))
    d_msg = torch.randint(0, 256, (B, W), generator=gen, device=dev, dtype=torch.int32).to(torch.uint8)
    d_rows = torch.empty((B, N), dtype=torch.uint8, device=dev)
    d_r = torch.empty((B, N), dtype=torch.uint8, device=dev)
    d_e = torch.empty((B, N), dtype=torch.int16, device=dev)
    d_e2 = torch.empty((B, N), dtype=torch.int16, device=dev)
    d_e3 = torch.empty((B, N), dtype=torch.int16, device=dev)
    d_value = torch.empty((B, N), dtype=torch.uint8, device=dev)
    d_out = torch.empty((B, W), dtype=torch.uint8, device=dev)
    d_flags = torch.empty((B,), dtype=torch.uint8, device=dev)
    eng.sample_ternary_dev(N, dr, dr, P_MOD - 1, key, 0, B, ptr(d_r))
    eng.bytes_to_rows_dev(N, W, ptr(d_msg), B, ptr(d_rows))
    eng.encrypt_batch_dev(N, Q, ptr(d_h), ptr(d_r), ptr(d_rows), B, ptr(d_e))
    eng.decrypt_batch_dev(N, Q, P_MOD, ptr(d_f), ptr(d_fp), ptr(d_e), B, ptr(d_value))
    d_e2.copy_(d_e)
    torch.cuda.synchronize()

    # name -> (group, algorithmic bytes, call)
    dev_calls = {
        "bytes_to_rows": ("a", B * (N + W), lambda: eng.bytes_to_rows_dev(N, W, ptr(d_msg), B, ptr(d_rows))),
        "rows_to_bytes": ("a", B * (N + W + 1), lambda: eng.rows_to_bytes_dev(N, W, ptr(d_value), B, ptr(d_out), ptr(d_flags))),
        "add_batch": ("a", 6 * N * B, lambda: eng.add_batch_dev(N, Q, ptr(d_e), ptr(d_e2), B, ptr(d_e3))),
        "encrypt_bytes_batch": ("b", B * (N + W + 2 * N), lambda: eng.encrypt_bytes_batch_dev(N, Q, W, ptr(d_h), ptr(d_r), ptr(d_msg), B, ptr(d_e2))),
        "encrypt_batch on rows": ("b", B * (N + N + 2 * N), lambda: eng.encrypt_batch_dev(N, Q, ptr(d_h), ptr(d_r), ptr(d_rows), B, ptr(d_e2))),
        "decrypt_bytes_batch": ("b", B * (2 * N + W + 1), lambda: eng.decrypt_bytes_batch_dev(N, Q, P_MOD, W, ptr(d_f), ptr(d_fp), ptr(d_e), B, ptr(d_out), ptr(d_flags))),
        "decrypt_batch value only": ("b", B * (2 * N + N), lambda: eng.decrypt_batch_dev(N, Q, P_MOD, ptr(d_f), ptr(d_fp), ptr(d_e), B, ptr(d_value))),
    }
    for _, _, fn in dev_calls.values():
        for _ in range(3):
            fn()
    torch.cuda.synchronize()
    ms = {name: [] for name in dev_calls}
    for _ in range(reps):
        for name, (_, _, fn) in dev_calls.items():
            t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            t0.record()
            for _ in range(a.iters):
                fn()
            t1.record()
            torch.cuda.synchronize()
            ms[name].append(t0.elapsed_time(t1) / a.iters)
    results = []
    for name, (group, algo, _) in dev_calls.items():
        med = statistics.median(ms[name])
        results.append(dict(report, group=group, call=name, N=N, q=Q, nbytes=W, items=B, timer="device events", ms=round(med, 4),
                            ms_spread=[round(min(ms[name]), 4), round(max(ms[name]), 4)], M_items_per_s=round(B / med / 1e3, 2),
                            algo_bytes=algo, algo_TB_per_s=round(algo / (med * 1e-3) / 1e12, 3)))
        print("(%s) %-26s %8.3f ms [%7.3f .. %7.3f]  %8.1f M items/s  %6.3f TB/s algorithmic" % (
            group, name, med, min(ms[name]), max(ms[name]), B / med / 1e3, algo / (med * 1e-3) / 1e12), flush=True)
    del d_rows, d_r, d_e, d_e2, d_e3, d_value, d_out, d_flags
    torch.cuda.empty_cache()

    # (c) host arrays in and out
    msg = d_msg.cpu().numpy()
    del d_msg
    rows = np.unpackbits(msg, axis=1, bitorder="big")
    rows = np.ascontiguousarray(np.pad(rows, ((0, 0), (0, N - 8 * W))))
    for kind in ("pinned", "pageable"):
        alloc = eng.pinned_empty if kind == "pinned" else (lambda shape, dt: np.empty(shape, dt))
        h_msg, h_rows = alloc((B, W), np.uint8), alloc((B, N), np.uint8)
        h_msg[:], h_rows[:] = msg, rows
        o_msg, o_flags, o_value = alloc((B, W), np.uint8), alloc((B,), np.uint8), alloc((B, N), np.uint8)
        lib, H = eng._lib, eng._h
        vp = lambda x: x.ctypes.data_as(ctypes.c_void_p)

        def bytes_call():
            eng._chk(lib.ntru_pipeline_bytes_batch(H, N, Q, P_MOD, vp(h), vp(f), vp(fp), vp(key), 0, dr, dr, None, W, vp(h_msg), B, None, None,
                                                   vp(o_msg), vp(o_flags)))

        def rows_call():
            eng._chk(lib.ntru_pipeline_batch(H, N, Q, P_MOD, vp(h), vp(f), vp(fp), vp(key), 0, dr, dr, None, vp(h_rows), B, None, None,
                                             vp(o_value), None))
        host_calls = {"pipeline_bytes_batch": (2 * W + 1, bytes_call), "pipeline_batch": (2 * N, rows_call)}
        for _, fn in host_calls.values():
            fn()
        sec = {name: [] for name in host_calls}
        for _ in range(reps):
            for name, (_, fn) in host_calls.items():
                t0 = time.perf_counter()
                fn()
                sec[name].append(time.perf_counter() - t0)
        for name, (bus, _) in host_calls.items():
            med = statistics.median(sec[name])
            results.append(dict(report, group="c", call=name, host_arrays=kind, N=N, q=Q, nbytes=W, items=B, timer="host clock, synchronised call",
                                ms=round(med * 1e3, 3), ms_spread=[round(min(sec[name]) * 1e3, 3), round(max(sec[name]) * 1e3, 3)],
                                M_items_per_s=round(B / med / 1e6, 2), bus_bytes_per_item=bus, bus_GB_per_s=round(bus * B / med / 1e9, 2)))
            print("(c) %-22s %-8s %9.2f ms [%8.2f .. %8.2f]  %8.2f M items/s  %6.2f GB/s over the bus" % (
                name, kind, med * 1e3, min(sec[name]) * 1e3, max(sec[name]) * 1e3, B / med / 1e6, bus * B / med / 1e9), flush=True)
        del h_msg, h_rows, o_msg, o_flags, o_value
    if a.jsonl:
        with open(a.jsonl, "w") as fh:
            for r in results:
                fh.write(json.dumps(r) + "\n")
    signal.alarm(0)


if __name__ == "__main__":
    main()
