#!/usr/bin/env python3
"""One mix step (ntru_reencrypt_batch_dev: re-randomise under h and permute), device-resident, beside the composition that was the only
way to do it on the device before: torch index_select of the rows, ntru_encrypt_batch_dev on an all-zero m, ntru_add_batch_dev.
N = 821, q = 4096, 2^20 rows, a random permutation, with and without the quotient; then the same call at identity src beside
k_encrypt_md on a byte m, for the cost of the wider addend.  The method of tools/bench_packed.py: one process, HIP events after a warm-up,
the calls alternating within every repeat, the median and the spread reported as ms, rows/s and achieved bytes/s over the 7 N bytes per row
the fused call has to move (5 N without the quotient).  No result is checked here: tests/test_mix_gpu.py does that.  Exit status 1 when the
slowest fused repeat is not below the fastest composed repeat.
    python tools/bench_mix.py [--reps 7] [--iters 5] [--log-rows 20] [--jsonl out.jsonl]"""
import argparse
import json
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402

import __graft_entry__ as ge  # noqa: E402

N, Q = 821, 4096


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=7, help="alternating repeats (>= 3)")
    ap.add_argument("--iters", type=int, default=5, help="launches per timed call")
    ap.add_argument("--log-rows", type=int, default=20)
    ap.add_argument("--jsonl", default=None)
    a = ap.parse_args()
    pkg = ge.load_package()
    eng = pkg.Engine(0)
    dev = torch.device("cuda:0")
    eng.set_stream(torch.cuda.current_stream().cuda_stream)
    B = 1 << a.log_rows
    gen = torch.Generator(device=dev).manual_seed(1)
    rnd = lambda hi, shape, dt: torch.randint(0, hi, shape, generator=gen, device=dev, dtype=torch.int32).to(dt)
    h, r = rnd(Q, (N,), torch.int16), rnd(3, (B, N), torch.uint8)
    e_in, m_bytes = rnd(Q, (B, N), torch.int16), rnd(2, (B, N), torch.uint8)
    perm = torch.randperm(B, generator=gen, device=dev)
    zero_m = torch.zeros((B, N), dtype=torch.uint8, device=dev)
    gathered, e0 = torch.empty_like(e_in), torch.empty_like(e_in)
    out, quot = torch.empty_like(e_in), torch.empty_like(e_in)
    P = lambda t: t.data_ptr()

    def fused(src, want_quot):
        pkg.reencrypt_batch_dev(eng, N, Q, P(h), P(r), P(e_in), B, P(out), B, d_src=None if src is None else P(src),
                                d_quotE=P(quot) if want_quot else None)

    def composed(want_quot):
        torch.index_select(e_in, 0, perm, out=gathered)
        eng.encrypt_batch_dev(N, Q, P(h), P(r), P(zero_m), B, P(e0), P(quot) if want_quot else None)
        eng.add_batch_dev(N, Q, P(e0), P(gathered), B, P(out))

    def encrypt_bytes(want_quot):
        eng.encrypt_batch_dev(N, Q, P(h), P(r), P(m_bytes), B, P(out), P(quot) if want_quot else None)

    calls = {}
    for wq in (True, False):
        tag = "e + quotE" if wq else "e only"
        calls["fused, permutation, " + tag] = (lambda wq=wq: fused(perm, wq), wq)
        calls["composed, permutation, " + tag] = (lambda wq=wq: composed(wq), wq)
        calls["fused, identity src, " + tag] = (lambda wq=wq: fused(None, wq), wq)
        calls["encrypt of byte m, " + tag] = (lambda wq=wq: encrypt_bytes(wq), wq)
    kernels = {}
    for name, (fn, _) in calls.items():
        for _ in range(3):
            fn()
        kernels[name] = ("index_select + k_encrypt_md + k_add_mod_vec" if name.startswith("composed") else eng.last_kernel())
    torch.cuda.synchronize()
    ms = {name: [] for name in calls}
    for _ in range(max(3, a.reps)):
        for name, (fn, _) in calls.items():
            t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            t0.record()
            for _ in range(a.iters):
                fn()
            t1.record()
            torch.cuda.synchronize()
            ms[name].append(t0.elapsed_time(t1) / a.iters)
    results = {}
    for name, (_, wq) in calls.items():
        med = statistics.median(ms[name])
        row_bytes = (7 if wq else 5) * N
        results[name] = {"N": N, "q": Q, "rows": B, "call": name, "kernel": kernels[name], "ms": round(med, 4),
                         "ms_spread": [round(min(ms[name]), 4), round(max(ms[name]), 4)], "G_rows_per_s": round(B / med / 1e6, 3),
                         "bytes_per_row": row_bytes, "TB_per_s": round(row_bytes * B / (med * 1e-3) / 1e12, 3)}
        print("%-36s %-44s %8.3f ms [%7.3f .. %7.3f]  %6.3f G rows/s  %6.3f TB/s over %d bytes per row"
              % (name, kernels[name], med, min(ms[name]), max(ms[name]), B / med / 1e6, results[name]["TB_per_s"], row_bytes), flush=True)
    ok = True
    for tag in ("e + quotE", "e only"):
        new, old = results["fused, permutation, " + tag], results["composed, permutation, " + tag]
        wins = new["ms_spread"][1] < old["ms_spread"][0]
        ok = ok and wins
        print("%s: composed %.3f ms / fused %.3f ms = %.2fx; slowest fused repeat %.3f ms %s fastest composed repeat %.3f ms"
              % (tag, old["ms"], new["ms"], old["ms"] / new["ms"], new["ms_spread"][1], "<" if wins else ">=", old["ms_spread"][0]))
        ident, enc = results["fused, identity src, " + tag], results["encrypt of byte m, " + tag]
        print("%s: identity src %.3f ms against the encrypt of a byte m %.3f ms: %+.1f %%"
              % (tag, ident["ms"], enc["ms"], 100.0 * (ident["ms"] / enc["ms"] - 1.0)))
    if a.jsonl:
        with open(a.jsonl, "w") as fh:
            for r_ in results.values():
                fh.write(json.dumps(r_) + "\n")
    sys.exit(0 if ok else 1)


if __name__ == "__main__":
    main()
