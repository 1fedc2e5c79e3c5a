#!/usr/bin/env python3
"""Drawing the order of a mix step on the device (ntru_draw_permutation_dev, ntru_mix_batch_dev: csrc/permutation.hip), B = 2^20.
  1. the draw: draw_permutation_dev beside what a caller did before -- numpy.random.default_rng().permutation(B) as int64 plus
     dev_upload of its 8 B per row -- a host clock around calls that end synchronised.  Gate: the device draw is faster by more than
     the two min-to-max spreads added; "met" or "NOT met" is printed with the numbers, and the exit status is 1 when it is not met.
  2. the mix: mix_batch_dev beside sample_ternary_dev + reencrypt_batch_dev with src already resident, N = 821, q = 4096, with the
     quotient, device events; the difference is what drawing the order costs.  No gate.
  3. sort traffic: the bytes the eight radix passes, the key kernel and the finish move, computed from the shapes below, over the
     time of argsort_keys_dev (device events), beside the HBM peak.
The method of tools/bench_mix.py: one process, every shape warmed up, the sides alternating within every repeat, the median and the
fastest .. slowest repeat.  No result is checked here: tests/test_shuffle_gpu.py does that.
    python tools/bench_shuffle.py [--reps 7] [--iters 5] [--log-rows 20] [--jsonl out.jsonl] [--only draw|mix|sort]"""
import argparse
import json
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np  # noqa: E402
import torch  # noqa: E402

import __graft_entry__ as ge  # noqa: E402

N, Q, P_MOD, DR = 821, 4096, 3, 30
KEY = [(i + 1) * 0x01010101 for i in range(8)]
HBM_PEAK_TB_S, HBM_ACHIEVABLE_TB_S = 8.0, 6.3          # MI355X: the specified peak and what streaming kernels reach
TILE, DIGITS, PASSES = 1024, 256, 8                    # PT_TILE, PT_DIGITS, PT_PASSES of permutation.hip


def sort_bytes(B, drawn):
    """Bytes the kernels of one argsort (drawn: one draw) read and write, from the shapes: per pass k_perm_hist reads the keys and writes
    the table, k_perm_offsets reads and writes the table and writes 256 totals, k_perm_scatter reads keys, indices (not in pass 0),
    the table row and the totals and writes keys (not in the last pass) and indices; k_perm_finish reads the indices and writes src;
    k_perm_keys writes the keys."""
    tiles = -(-B // TILE)
    table = tiles * DIGITS * 4
    per_pass = []
    for p in range(PASSES):
        hist = 8 * B + table
        offsets = 2 * table + DIGITS * 4
        scatter = 8 * B + (4 * B if p else 0) + table + tiles * DIGITS * 4 + (8 * B if p < PASSES - 1 else 0) + 4 * B
        per_pass.append(hist + offsets + scatter)
    return {"per_pass": per_pass, "finish": 4 * B + 8 * B, "keys": 8 * B if drawn else 0,
            "total": sum(per_pass) + 12 * B + (8 * B if drawn else 0)}


def spread(v):
    return round(statistics.median(v), 4), [round(min(v), 4), round(max(v), 4)]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=7, help="alternating repeats (>= 3)")
    ap.add_argument("--iters", type=int, default=5, help="calls per timed window")
    ap.add_argument("--log-rows", type=int, default=20)
    ap.add_argument("--jsonl", default=None)
    ap.add_argument("--only", choices=("draw", "mix", "sort"), default=None)
    a = ap.parse_args()
    pkg = ge.load_package()
    eng = pkg.Engine(0)
    dev = torch.device("cuda:0")
    eng.set_stream(torch.cuda.current_stream().cuda_stream)
    B = 1 << a.log_rows
    reps = max(3, a.reps)
    gen = torch.Generator(device=dev).manual_seed(1)
    P = lambda t: t.data_ptr()
    src = torch.empty(B, dtype=torch.int64, device=dev)
    results = []
    ok = True

    def device_ms(calls):
        """{name: [ms per call of every repeat]}, device events, the calls alternating within a repeat."""
        for fn in calls.values():
            for _ in range(3):
                fn()
        torch.cuda.synchronize()
        ms = {name: [] for name in calls}
        for _ in range(reps):
            for name, fn in calls.items():
                t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                t0.record()
                for _ in range(a.iters):
                    fn()
                t1.record()
                torch.cuda.synchronize()
                ms[name].append(t0.elapsed_time(t1) / a.iters)
        return ms

    if a.only in (None, "draw"):
        rng = np.random.default_rng()
        state = {"id": 0}

        def device_draw():
            state["id"] += 1
            pkg.draw_permutation_dev(eng, KEY, state["id"], B, P(src))
            eng.synchronize()

        def host_draw():
            perm = rng.permutation(B).astype(np.int64, copy=False)
            eng.dev_upload(P(src), perm)
            eng.synchronize()

        sides = {"draw_permutation_dev": device_draw, "numpy permutation + dev_upload": host_draw}
        for fn in sides.values():
            for _ in range(3):
                fn()
        ms = {name: [] for name in sides}
        for _ in range(reps):
            for name, fn in sides.items():
                t0 = time.perf_counter()
                for _ in range(a.iters):
                    fn()
                ms[name].append((time.perf_counter() - t0) * 1e3 / a.iters)
        (new, new_sp), (old, old_sp) = spread(ms["draw_permutation_dev"]), spread(ms["numpy permutation + dev_upload"])
        for name, (med, sp) in (("draw_permutation_dev", (new, new_sp)), ("numpy permutation + dev_upload", (old, old_sp))):
            print("draw  %-32s %8.3f ms [%7.3f .. %7.3f]  %7.1f M items/s" % (name, med, sp[0], sp[1], B / med / 1e3), flush=True)
            results.append({"measurement": "draw", "rows": B, "call": name, "ms": med, "ms_spread": sp, "clock": "host, synchronised"})
        spreads = (new_sp[1] - new_sp[0]) + (old_sp[1] - old_sp[0])
        met = old - new > spreads
        ok = ok and met
        print("draw  gate %s: the device draw is %.3f ms faster (%.2fx); the two spreads added are %.3f ms"
              % ("met" if met else "NOT met", old - new, old / new, spreads), flush=True)
        results.append({"measurement": "draw gate", "met": bool(met), "margin_ms": round(old - new, 4), "spreads_ms": round(spreads, 4)})

    if a.only in (None, "mix"):
        rnd = lambda hi, shape, dt: torch.randint(0, hi, shape, generator=gen, device=dev, dtype=torch.int32).to(dt)
        h, e_in = rnd(Q, (N,), torch.int16), rnd(Q, (B, N), torch.int16)
        r = torch.empty((B, N), dtype=torch.uint8, device=dev)
        out, quot = torch.empty_like(e_in), torch.empty_like(e_in)
        resident = torch.randperm(B, generator=gen, device=dev)

        def one_call():
            pkg.mix_batch_dev(eng, N, Q, P_MOD, P(h), KEY, 0, DR, DR, 1, P(e_in), B, P(r), P(src), P(out), d_quotE=P(quot))

        def two_calls():
            eng.sample_ternary_dev(N, DR, DR, P_MOD - 1, KEY, 0, B, P(r))
            pkg.reencrypt_batch_dev(eng, N, Q, P(h), P(r), P(e_in), B, P(out), B, d_src=P(resident), d_quotE=P(quot))

        ms = device_ms({"mix_batch_dev": one_call, "sample_ternary_dev + reencrypt_batch_dev, src resident": two_calls})
        meds = {}
        for name, v in ms.items():
            med, sp = spread(v)
            meds[name] = med
            print("mix   %-52s %8.3f ms [%7.3f .. %7.3f]  %6.3f G rows/s" % (name, med, sp[0], sp[1], B / med / 1e6), flush=True)
            results.append({"measurement": "mix", "N": N, "q": Q, "rows": B, "call": name, "ms": med, "ms_spread": sp, "clock": "device events"})
        a_ms, b_ms = meds["mix_batch_dev"], meds["sample_ternary_dev + reencrypt_batch_dev, src resident"]
        print("mix   drawing the order costs %.3f ms of %.3f ms (%.1f %%)" % (a_ms - b_ms, a_ms, 100.0 * (a_ms - b_ms) / a_ms), flush=True)
        del h, e_in, r, out, quot, resident

    if a.only in (None, "sort"):
        keys = torch.randint(-2**63, 2**63 - 1, (B,), generator=gen, device=dev, dtype=torch.int64)
        ms = device_ms({"argsort_keys_dev": lambda: pkg.argsort_keys_dev(eng, P(keys), B, P(src)),
                        "draw_permutation_dev": lambda: pkg.draw_permutation_dev(eng, KEY, 1, B, P(src))})
        for name, v in ms.items():
            med, sp = spread(v)
            nbytes = sort_bytes(B, name.startswith("draw"))
            rate = nbytes["total"] / (med * 1e-3) / 1e12
            print("sort  %-22s %8.3f ms [%7.3f .. %7.3f]  %6.1f M keys/s  %.1f MB moved (%.1f MB per middle pass)  %.3f TB/s = %.1f %% of the "
                  "%.1f TB/s HBM peak (%.1f TB/s achievable)" % (name, med, sp[0], sp[1], B / med / 1e3, nbytes["total"] / 1e6,
                                                                 nbytes["per_pass"][1] / 1e6, rate, 100.0 * rate / HBM_PEAK_TB_S,
                                                                 HBM_PEAK_TB_S, HBM_ACHIEVABLE_TB_S), flush=True)
            results.append({"measurement": "sort", "rows": B, "call": name, "ms": med, "ms_spread": sp, "bytes": nbytes["total"],
                            "bytes_per_pass": nbytes["per_pass"], "TB_per_s": round(rate, 4), "clock": "device events"})

    if a.jsonl:
        with open(a.jsonl, "w") as fh:
            for r_ in results:
                fh.write(json.dumps(r_) + "\n")
    sys.exit(0 if ok else 1)


if __name__ == "__main__":
    main()
