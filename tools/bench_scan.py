#!/usr/bin/env python3
"""Scanning for decryptable rows, measured at N = 821, q = 4096, nbytes = 102, the centred lift, a 4-byte tag and 2^20 rows on one
device, for hit rates of 0, 1 % and 100 %, K = 1 and 4 keys (the rows are addressed to key 0), dense and packed input:
  (gate) host arrays in and out: ntru_scan_bytes_batch against what it replaces, ntru_decrypt_bytes_batch plus the numpy filter, in the
      same process and alternating; the scan passes when the composition's median exceeds the scan's by more than the composition's
      own min-to-max spread (K = 1, 1 % hits, dense).  The other host cases are recorded beside it.
  (dev) ntru_scan_bytes[_packed]_batch_dev against ntru_decrypt_bytes_batch_dev per key on the same rows: the difference is what the three
      select kernels and their launches cost; ntru_rows_to_bytes_dev alone on the same rows stands beside it (it reads about eight times
      the bytes the select kernels read).
The host calls are timed with the host clock around calls that return synchronised, the device calls with device events; every call is
warmed up first; min, median and max over the repeats are reported.  Nothing is checked here (tests/test_scan_gpu.py does that) and
nothing is retried: any failure ends the run, and so does the time limit.
    python tools/bench_scan.py [--reps 7] [--log-b 20] [--timeout 540] [--jsonl out.jsonl]"""
import argparse
import ctypes
import json
import os
import signal
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np  # noqa: E402
import torch  # noqa: E402

import __graft_entry__ as ge  # noqa: E402

N, Q, P_MOD = 821, 4096, 3
W = N // 8
TAG = b"NTRU"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=7, help="alternating repeats (>= 5)")
    ap.add_argument("--log-b", type=int, default=20)
    ap.add_argument("--timeout", type=int, default=540, help="seconds after which the run gives up")
    ap.add_argument("--jsonl", default=None)
    a = ap.parse_args()
    signal.signal(signal.SIGALRM, lambda *_: sys.exit("bench_scan: time limit of %d s reached" % a.timeout))
    signal.alarm(a.timeout)
    reps = max(5, a.reps)
    pkg = ge.load_package()
    eng = pkg.Engine(0)
    dev = torch.device("cuda:0")
    eng.set_stream(torch.cuda.current_stream().cuda_stream)
    pkg.lift.set_lift(eng, "centred")
    props = torch.cuda.get_device_properties(0)
    report = {"device": props.name, "cus": props.multi_processor_count}
    B = 1 << a.log_b
    with open(os.path.join(ge.ROOT, "tests", "golden", "scheme_n821_q4096.json")) as fh:
        gold = json.load(fh)
    k0, dr = gold["keys"][0], gold["options"]["dr"]
    pad = lambda v, dt: np.array(list(v) + [0] * (N - len(v)), dtype=dt)
    h = pad(k0["h"], np.uint16)
    more = eng.keygen_batch(N, Q, P_MOD, gold["options"]["df"], gold["options"]["dg"], np.arange(8, dtype=np.uint32), 3, want=("f", "fp"))
    f = np.concatenate([pad(k0["f"], np.int8)[None], more["f"]])
    fp = np.concatenate([pad(k0["fp"], np.uint8)[None], more["fp"]])
    key = np.arange(1, 9, dtype=np.uint32) * 0x9E3779B1
    ptr = lambda t: t.data_ptr()
    gen = torch.Generator(device=dev).manual_seed(1)
    d_h = torch.from_numpy(h.view(np.uint8)).to(dev)
    d_f, d_fp = torch.from_numpy(f).to(dev), torch.from_numpy(fp).to(dev)
    d_msg = torch.randint(0, 256, (B, W), generator=gen, device=dev, dtype=torch.int32).to(torch.uint8)
    d_msg[:, :4] = torch.tensor(list(b"none"), dtype=torch.uint8, device=dev)
    d_r = torch.empty((B, N), dtype=torch.uint8, device=dev)
    eng.sample_ternary_dev(N, dr, dr, P_MOD - 1, key, 0, B, ptr(d_r))
    osz = eng.pack_params(Q - 1, N)["outputSize"]
    d_e = {}                                                  # hit rate in percent -> dense rows
    d_e[0] = torch.empty((B, N), dtype=torch.int16, device=dev)
    eng.encrypt_bytes_batch_dev(N, Q, W, ptr(d_h), ptr(d_r), ptr(d_msg), B, ptr(d_e[0]))
    d_msg[:, :4] = torch.tensor(list(TAG), dtype=torch.uint8, device=dev)
    d_e[100] = torch.empty((B, N), dtype=torch.int16, device=dev)
    eng.encrypt_bytes_batch_dev(N, Q, W, ptr(d_h), ptr(d_r), ptr(d_msg), B, ptr(d_e[100]))
    torch.cuda.synchronize()
    pick = (torch.rand(B, generator=gen, device=dev) < 0.01)
    d_e[1] = torch.where(pick[:, None], d_e[100], d_e[0]).contiguous()
    del d_msg, d_r
    d_packed = torch.empty((B, osz, 4), dtype=torch.int64, device=dev)
    d_bytes = torch.empty((B, W), dtype=torch.uint8, device=dev)
    d_flags = torch.empty((B,), dtype=torch.uint8, device=dev)
    d_value = torch.empty((B, N), dtype=torch.uint8, device=dev)
    d_count = torch.zeros(4, dtype=torch.int64, device=dev)
    d_hit_row = torch.empty((4, B), dtype=torch.int64, device=dev)
    d_hit_bytes = torch.empty((4, B, W), dtype=torch.uint8, device=dev)
    eng.decrypt_batch_dev(N, Q, P_MOD, ptr(d_f), ptr(d_fp), ptr(d_e[1]), B, ptr(d_value))
    torch.cuda.synchronize()
    results = []

    def emit(rec, line):
        results.append(dict(report, N=N, q=Q, nbytes=W, items=B, lift="centred", tag_len=len(TAG), **rec))
        print(line, flush=True)

    # ---- (dev) --------------------------------------------------------------------------------------------------------------------
    def timed(fn):
        for _ in range(2):
            fn()
        torch.cuda.synchronize()
        ms = []
        for _ in range(reps):
            t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            t0.record()
            fn()
            t1.record()
            torch.cuda.synchronize()
            ms.append(t0.elapsed_time(t1))
        return ms

    r2b = timed(lambda: eng.rows_to_bytes_dev(N, W, ptr(d_value), B, ptr(d_bytes), ptr(d_flags)))
    emit({"group": "dev", "call": "rows_to_bytes", "ms": round(statistics.median(r2b), 4), "ms_spread": [round(min(r2b), 4), round(max(r2b), 4)]},
         "(dev) rows_to_bytes alone                         %8.3f ms [%7.3f .. %7.3f]" % (statistics.median(r2b), min(r2b), max(r2b)))
    for rate in (0, 1, 100):
        eng._chk(eng._lib.ntru_pack_batch_dev(eng._h, Q - 1, N, eng._dp(ptr(d_e[rate])), B, eng._dp(ptr(d_packed))))
        torch.cuda.synchronize()
        for K in (1, 4):
            def decrypt_only():
                for k in range(K):
                    eng.decrypt_bytes_batch_dev(N, Q, P_MOD, W, ptr(d_f) + k * N, ptr(d_fp) + k * N, ptr(d_e[rate]), B, ptr(d_bytes), ptr(d_flags))
            base = timed(decrypt_only)
            for packed in (False, True):
                fn = pkg.scan_bytes_packed_batch_dev if packed else pkg.scan_bytes_batch_dev
                rows = ptr(d_packed) if packed else ptr(d_e[rate])
                ms = timed(lambda: fn(eng, N, Q, P_MOD, W, K, ptr(d_f), ptr(d_fp), rows, B, ptr(d_count), tag=TAG, tag_off=0, max_hits=B,
                                      d_hit_row=ptr(d_hit_row), d_hit_bytes=ptr(d_hit_bytes)))
                med, bmed = statistics.median(ms), statistics.median(base)
                emit({"group": "dev", "call": "scan_bytes_%sbatch_dev" % ("packed_" if packed else ""), "hit_percent": rate, "K": K,
                      "count": d_count[:K].tolist(), "ms": round(med, 4), "ms_spread": [round(min(ms), 4), round(max(ms), 4)],
                      "decrypt_bytes_ms": round(bmed, 4), "decrypt_bytes_ms_spread": [round(min(base), 4), round(max(base), 4)],
                      "select_ms": round(med - bmed, 4), "M_rows_per_s": round(B * K / med / 1e3, 1)},
                     "(dev) %-6s %3d %% hits K=%d  scan %8.3f ms [%7.3f .. %7.3f]  decrypt_bytes_dev x K %8.3f ms [%7.3f .. %7.3f]  "
                     "difference %7.3f ms  %7.1f M row-keys/s" % ("packed" if packed else "dense", rate, K, med, min(ms), max(ms), bmed,
                                                                   min(base), max(base), med - bmed, B * K / med / 1e3))
    del d_packed, d_bytes, d_flags, d_value, d_hit_row, d_hit_bytes

    # ---- (gate) and the other host cases ------------------------------------------------------------------------------------------
    lib, H = eng._lib, eng._h
    vp = lambda x: x.ctypes.data_as(ctypes.c_void_p)
    tag = np.frombuffer(TAG, np.uint8)
    tag_word = tag.view(np.uint32)[0]
    for rate, K, packed in ((1, 1, False), (0, 1, False), (100, 1, False), (1, 4, False), (1, 1, True)):
        e = d_e[rate].cpu().numpy().view(np.uint16)
        rows = pkg.pack_rows(eng, N, Q, e) if packed else e
        out_bytes, out_flags = np.empty((B, W), np.uint8), np.empty(B, np.uint8)
        value = np.empty((B, N), np.uint8) if packed else None
        hit_row, hit_bytes, count = np.empty((K, B), np.int64), np.empty((K, B, W), np.uint8), np.zeros(K, np.int64)
        sym = lib.ntru_scan_bytes_packed_batch if packed else lib.ntru_scan_bytes_batch
        got = {}

        def scan_call():
            eng._chk(sym(H, N, Q, P_MOD, W, K, vp(f), vp(fp), vp(rows), B, 0, 4, vp(tag), B, vp(hit_row), vp(hit_bytes), vp(count)))
            got["scan"] = [(hit_row[k, :count[k]], hit_bytes[k, :count[k]]) for k in range(K)]

        def composition():
            res = []
            for k in range(K):
                if packed:                                   # what exists for packed rows: decrypt to values, then the codec on the device
                    eng._chk(lib.ntru_decrypt_packed_batch(H, N, Q, P_MOD, vp(f[k]), vp(fp[k]), vp(rows), B, vp(value), None, None, None))
                    eng._chk(lib.ntru_rows_to_bytes(H, N, W, vp(value), B, vp(out_bytes), vp(out_flags)))
                else:
                    eng._chk(lib.ntru_decrypt_bytes_batch(H, N, Q, P_MOD, W, vp(f[k]), vp(fp[k]), vp(rows), B, vp(out_bytes), vp(out_flags)))
                hit = (out_flags == 0) & (np.ascontiguousarray(out_bytes[:, :4]).view(np.uint32)[:, 0] == tag_word)
                idx = np.flatnonzero(hit)
                res.append((idx, out_bytes[idx]))
            got["composition"] = res
        calls = {"scan": scan_call, "composition": composition}
        for fn in calls.values():
            fn()
        sec = {name: [] for name in calls}
        for _ in range(reps):
            for name, fn in calls.items():
                t0 = time.perf_counter()
                fn()
                sec[name].append(time.perf_counter() - t0)
        agree = all(np.array_equal(x[0], y[0]) and np.array_equal(x[1], y[1]) for x, y in zip(got["scan"], got["composition"]))
        s, c = [x * 1e3 for x in sec["scan"]], [x * 1e3 for x in sec["composition"]]
        margin, spread = statistics.median(c) - statistics.median(s), max(c) - min(c)
        gate = rate == 1 and K == 1 and not packed
        emit({"group": "gate" if gate else "host", "hit_percent": rate, "K": K, "packed": packed, "count": count.tolist(), "same_result": agree,
              "scan_ms": round(statistics.median(s), 3), "scan_ms_spread": [round(min(s), 3), round(max(s), 3)],
              "composition_ms": round(statistics.median(c), 3), "composition_ms_spread": [round(min(c), 3), round(max(c), 3)],
              "margin_ms": round(margin, 3), "composition_spread_ms": round(spread, 3), "scan_wins": bool(margin > spread),
              "scan_M_rows_per_s": round(B * K / statistics.median(s) / 1e3, 1),
              "composition_M_rows_per_s": round(B * K / statistics.median(c) / 1e3, 1)},
             "(%s) %-6s %3d %% hits K=%d  scan %8.2f ms [%7.2f .. %7.2f]  decrypt_bytes + numpy filter %8.2f ms [%7.2f .. %7.2f]  "
             "margin %7.2f ms against a spread of %6.2f ms: %s; same result: %s" % (
                 "gate" if gate else "host", "packed" if packed else "dense", rate, K, statistics.median(s), min(s), max(s),
                 statistics.median(c), min(c), max(c), margin, spread, "scan wins" if margin > spread else "NO WIN", agree))
    if a.jsonl:
        with open(a.jsonl, "w") as fh:
            for r in results:
                fh.write(json.dumps(r) + "\n")
    signal.alarm(0)


if __name__ == "__main__":
    main()
