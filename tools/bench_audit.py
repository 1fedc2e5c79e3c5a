#!/usr/bin/env python3
"""Checking revealed re-encryption links (ntru_check_links_batch_dev: one flag byte per link), device-resident, beside the composition a
user had before: ntru_reencrypt_batch_dev without the quotient into a scratch array, (tmp != e_out).any(dim=1) in torch, then the range
and count test of r in torch -- and a second composed arm without the r test, for what the product-and-compare part alone buys.
(N, q) = (821, 4096), (509, 2048), (701, 8192); 2^20 links that all hold, a random permutation as in_idx, out_idx None; r from the
engine's sampler with dr ones and dr entries 2.  The method of tools/bench_mix.py: one process, HIP events after a warm-up, the arms
alternating within every repeat, the median and max - min reported as ms, links/s and achieved bytes/s over the 5 N bytes per link the
fused call has to move.  The fused arm's n_bad is read back once, before the timing, and must be 0; no other result is checked here:
tests/test_audit_gpu.py does that.
    python tools/bench_audit.py [--reps 7] [--iters 5] [--log-links 20] [--sets 821:4096:30,...] [--arms fused,...] [--jsonl out.jsonl]"""
import argparse
import json
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402

import __graft_entry__ as ge  # noqa: E402

ARMS = ("fused", "composed", "composed without r test")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=7, help="alternating repeats (>= 3)")
    ap.add_argument("--iters", type=int, default=5, help="launches per timed call")
    ap.add_argument("--log-links", type=int, default=20)
    ap.add_argument("--sets", default="821:4096:30,509:2048:20,701:8192:30", help="N:q:dr, comma separated")
    ap.add_argument("--arms", default=",".join(ARMS))
    ap.add_argument("--jsonl", default=None)
    a = ap.parse_args()
    pkg = ge.load_package()
    eng = pkg.Engine(0)
    dev = torch.device("cuda:0")
    eng.set_stream(torch.cuda.current_stream().cuda_stream)
    L = 1 << a.log_links
    arms = [x.strip() for x in a.arms.split(",")]
    P = lambda t: t.data_ptr()
    lines = []
    for spec in a.sets.split(","):
        N, Q, dr = (int(x) for x in spec.split(":"))
        gen = torch.Generator(device=dev).manual_seed(N)
        rnd = lambda hi, shape, dt: torch.randint(0, hi, shape, generator=gen, device=dev, dtype=torch.int32).to(dt)
        h, e_in = rnd(Q, (N,), torch.int16), rnd(Q, (L, N), torch.int16)
        r = torch.empty((L, N), dtype=torch.uint8, device=dev)
        eng.sample_ternary_dev(N, dr, dr, 2, list(range(1, 9)), 0, L, P(r))
        perm = torch.randperm(L, generator=gen, device=dev)
        e_out, tmp = torch.empty_like(e_in), torch.empty_like(e_in)
        pkg.reencrypt_batch_dev(eng, N, Q, P(h), P(r), P(e_in), L, P(e_out), L, d_src=P(perm))          # links that hold
        flags = torch.empty(L, dtype=torch.uint8, device=dev)
        n_bad = torch.full((1,), -1, dtype=torch.int64, device=dev)

        def fused():
            pkg.check_links_dev(eng, N, Q, P(h), P(r), P(e_in), L, P(e_out), L, L, P(flags), d_n_bad=P(n_bad), d_in_idx=P(perm), other=2,
                                n1=dr, n2=dr)

        def composed(r_test):
            pkg.reencrypt_batch_dev(eng, N, Q, P(h), P(r), P(e_in), L, P(tmp), L, d_src=P(perm))
            bad = (tmp != e_out).any(dim=1).to(torch.uint8) * 4
            if r_test:
                bad_r = (r > 2).any(dim=1) | ((r == 1).sum(dim=1) != dr) | ((r == 2).sum(dim=1) != dr)
                bad = torch.where(bad_r, torch.full_like(bad, 2), bad)
            flags.copy_(bad)
            n_bad.copy_(torch.count_nonzero(bad))

        calls = {"fused": fused, "composed": lambda: composed(True), "composed without r test": lambda: composed(False)}
        calls = {k: v for k, v in calls.items() if k in arms}
        kernels = {}
        for name, fn in calls.items():
            for _ in range(3):
                fn()
            kernels[name] = eng.last_kernel() + ("" if name == "fused" else " + torch")
            torch.cuda.synchronize()
            if int(n_bad.item()) != 0:
                sys.exit("%s at N = %d: n_bad = %d on links that hold" % (name, N, int(n_bad.item())))
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
        res = {}
        for name in calls:
            med, spread = statistics.median(ms[name]), max(ms[name]) - min(ms[name])
            res[name] = {"N": N, "q": Q, "dr": dr, "links": L, "arm": name, "kernel": kernels[name], "ms": round(med, 4),
                         "ms_max_minus_min": round(spread, 4), "G_links_per_s": round(L / med / 1e6, 3), "bytes_per_link": 5 * N,
                         "TB_per_s": round(5 * N * L / (med * 1e-3) / 1e12, 3), "library": os.path.basename(pkg.engine.library_path())}
            lines.append(res[name])
            print("N %4d q %5d  %-20s %-44s %8.3f ms (max - min %6.3f)  %6.3f G links/s  %6.3f TB/s over %d bytes per link"
                  % (N, Q, name, kernels[name], med, spread, L / med / 1e6, res[name]["TB_per_s"], 5 * N), flush=True)
        if "fused" in res:
            for other in ("composed", "composed without r test"):
                if other in res:
                    gap, noise = res[other]["ms"] - res["fused"]["ms"], res[other]["ms_max_minus_min"] + res["fused"]["ms_max_minus_min"]
                    print("N %4d q %5d  %s %.3f ms / fused %.3f ms = %.2fx; the gap of %.3f ms is %s both arms' spread (%.3f ms)"
                          % (N, Q, other, res[other]["ms"], res["fused"]["ms"], res[other]["ms"] / res["fused"]["ms"], gap,
                             "above" if gap > noise else "NOT above", noise), flush=True)
        del h, e_in, r, perm, e_out, tmp, flags, n_bad
        torch.cuda.empty_cache()
    if a.jsonl:
        with open(a.jsonl, "w") as fh:
            for line in lines:
                fh.write(json.dumps(line) + "\n")


if __name__ == "__main__":
    main()
