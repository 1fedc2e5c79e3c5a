#!/usr/bin/env python3
"""Removing duplicates from a batch, measured with everything resident on one device: 2^20 rows at (N, mod) = (821, 4096), (509, 2048)
and (701, 8192), dense and packed, with no duplicates, 1 % duplicates and all rows identical.  Arms, interleaved in the same run:
  dedup        ntru_dedup_rows_dev, first and unique, 64-bit fingerprints, a fresh salt per call
  packed       ntru_dedup_packed_dev on the same rows in the wire format
  torch_unique (a) torch.unique(rows % mod, dim=0, return_inverse=True) on the same device (what a caller had on the device)
  numpy_unique (b) the download plus numpy.unique(axis=0, return_index=True, return_inverse=True), at 2^--numpy-log-b rows and reported
               as such (2^20 rows take too long to repeat), on the batch without duplicates only
Device events around each device arm, wall clock around (b); every arm warmed up first; median and min .. max over the repeats.  The
traffic floor beside it: one read of the rows for the fingerprint, the eight sort passes over 12 bytes per key, one more row read per
fingerprint-equal neighbour (every duplicate), at --hbm-tbps (6.3 TB/s: the measured streaming rate of the device).  Nothing is checked
here (tests/test_dedup_gpu.py does that) and nothing is retried: any failure ends the run, and so does the time limit.
    python tools/bench_dedup.py [--reps 5] [--log-b 20] [--arms dedup,packed,torch_unique,numpy_unique] [--slow-reps 2]
                                [--numpy-log-b 16] [--label text] [--timeout 900] [--jsonl out.jsonl]"""
import argparse
import json
import os
import secrets
import signal
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np  # noqa: E402
import torch  # noqa: E402

import __graft_entry__ as ge  # noqa: E402

SETS = ((821, 4096), (509, 2048), (701, 8192))
KINDS = ("distinct", "one_percent", "identical")
ARMS = ("dedup", "packed", "torch_unique", "numpy_unique")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5, help="interleaved repeats of the engine's arms (>= 3)")
    ap.add_argument("--slow-reps", type=int, default=2, help="repeats of torch.unique and numpy.unique")
    ap.add_argument("--log-b", type=int, default=20)
    ap.add_argument("--numpy-log-b", type=int, default=16)
    ap.add_argument("--arms", default=",".join(ARMS))
    ap.add_argument("--hbm-tbps", type=float, default=6.3)
    ap.add_argument("--timeout", type=int, default=900, help="seconds after which the run gives up")
    ap.add_argument("--label", default="working tree", help="what the records call the build that was measured")
    ap.add_argument("--jsonl", default=None)
    a = ap.parse_args()
    signal.signal(signal.SIGALRM, lambda *_: sys.exit("bench_dedup: time limit of %d s reached" % a.timeout))
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
    print("%s, %d CUs, library %s, B = 2^%d" % (props.name, report["cus"], pkg.library_path(), a.log_b), flush=True)
    gen = torch.Generator(device=dev).manual_seed(1)
    ptr = lambda t: t.data_ptr()
    d_work = torch.empty((pkg.dedup_workspace_bytes(eng, 821, B),), dtype=torch.uint8, device=dev)
    d_first = torch.empty((B,), dtype=torch.int64, device=dev)
    d_unique = torch.empty((B,), dtype=torch.int64, device=dev)
    d_count = torch.zeros((1,), dtype=torch.int64, device=dev)
    out = open(a.jsonl, "w") if a.jsonl else None                             # a record per line as it is measured

    def timed(fn):
        t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        t0.record()
        fn()
        t1.record()
        torch.cuda.synchronize()
        return t0.elapsed_time(t1)

    for N, mod in SETS:
        os_ = eng.pack_params(mod - 1, N)["outputSize"]
        base = torch.randint(0, mod, (B, N), generator=gen, device=dev, dtype=torch.int32).to(torch.int16)
        for kind in KINDS:
            d_rows = base.clone()
            if kind == "one_percent":
                at = torch.randperm(B, generator=gen, device=dev)[:B // 100]
                d_rows[at] = d_rows[torch.randint(0, B, (B // 100,), generator=gen, device=dev)]
            elif kind == "identical":
                d_rows[:] = d_rows[0]
            d_packed = None
            if "packed" in names:
                d_packed = torch.empty((B, os_, 4), dtype=torch.int64, device=dev)
                eng._chk(eng._lib.ntru_pack_batch_dev(eng._h, mod - 1, N, eng._dp(ptr(d_rows)), B, eng._dp(ptr(d_packed))))
            torch.cuda.synchronize()

            def dedup():
                pkg.dedup_rows_dev(eng, N, mod, None, 0, ptr(d_rows), B, secrets.randbits(64), 64, ptr(d_work), ptr(d_first), ptr(d_unique),
                                   ptr(d_count))

            def packed():
                pkg.dedup_packed_dev(eng, N, mod, None, 0, ptr(d_packed), B, secrets.randbits(64), 64, ptr(d_work), ptr(d_first),
                                     ptr(d_unique), ptr(d_count))

            def torch_unique():
                torch.unique(d_rows % mod, dim=0, return_inverse=True)
            fast = {n: fn for n, fn in (("dedup", dedup), ("packed", packed)) if n in names}
            for fn in fast.values():
                fn()
                fn()
            torch.cuda.synchronize()
            ms = {n: [] for n in fast}
            for _ in range(reps):
                for n, fn in fast.items():
                    ms[n].append(timed(fn))
            firsts = int(d_count.item())
            if "torch_unique" in names:
                torch_unique()
                torch.cuda.synchronize()
                ms["torch_unique"] = [timed(torch_unique) for _ in range(max(1, a.slow_reps))]
            rec = dict(report, N=N, mod=mod, kind=kind, first_occurrences=firsts)
            line = "N = %4d mod = %4d %-11s" % (N, mod, kind)
            for n, v in ms.items():
                med = statistics.median(v)
                rec[n] = {"ms": round(med, 4), "ms_spread": [round(min(v), 4), round(max(v), 4)], "reps": len(v)}
                line += " %-12s %9.3f ms [%9.3f .. %9.3f]" % (n, med, min(v), max(v))
            for n, row_bytes in (("dedup", 2 * N), ("packed", 32 * os_)):
                if n in ms:
                    floor = B * row_bytes + 8 * 12 * B + (B - firsts) * row_bytes
                    rec[n]["floor_bytes"] = floor
                    rec[n]["floor_ms"] = round(floor / (a.hbm_tbps * 1e9), 4)
                    rec[n]["over_floor"] = round(rec[n]["ms"] / rec[n]["floor_ms"], 2)
                    line += " %s / floor = %.2f" % (n, rec[n]["over_floor"])
            if "dedup" in ms and "torch_unique" in ms:
                gain = rec["torch_unique"]["ms"] - rec["dedup"]["ms"]
                spread = max(rec[n]["ms_spread"][1] - rec[n]["ms_spread"][0] for n in ("dedup", "torch_unique"))
                rec["torch_unique_over_dedup"] = round(rec["torch_unique"]["ms"] / rec["dedup"]["ms"], 2)
                rec["dedup_beats_torch_unique"] = bool(gain > spread)          # the gain against the larger max - min of the two
                line += " torch / dedup = %.1f (%s)" % (rec["torch_unique_over_dedup"], "holds" if rec["dedup_beats_torch_unique"] else "does NOT hold")
            if "numpy_unique" in names and kind == "distinct":
                Bn = min(B, 1 << a.numpy_log_b)
                wall = []
                for _ in range(1 + max(1, a.slow_reps)):                      # the first one is the warm-up
                    t = time.perf_counter()
                    host = d_rows[:Bn].cpu().numpy().view(np.uint16)
                    np.unique(host % mod, axis=0, return_index=True, return_inverse=True)
                    wall.append((time.perf_counter() - t) * 1e3)
                wall = wall[1:]
                rec["numpy_unique"] = {"rows": Bn, "ms": round(statistics.median(wall), 2), "ms_spread": [round(min(wall), 2), round(max(wall), 2)],
                                       "reps": len(wall)}
                line += " numpy_unique at 2^%d rows %9.1f ms" % (a.numpy_log_b, rec["numpy_unique"]["ms"])
            if out:
                out.write(json.dumps(rec) + "\n")
                out.flush()
            print(line, flush=True)
            del d_rows, d_packed
        del base
    if out:
        out.close()
    signal.alarm(0)


if __name__ == "__main__":
    main()
