#!/usr/bin/env python3
"""Counting decrypted messages by choice and group, measured at N = 821, q = 4096, nbytes = 102, the centred lift, a 4-byte tag at byte 0,
a 2-byte choice field at byte 4 with 8 choices, and 2^20 rows on one device of which about 90 % are honest ballots (5 % carry a wrong
tag, 5 % are arbitrary values).  Every comparison runs both arms in the same process, alternating, after a warm-up of each; the median
and max - min of each arm are reported and a difference counts only where it exceeds BOTH spreads, else the verdict is "level":
  (dev)   ntru_count_bytes_batch_dev against ntru_decrypt_bytes_batch_dev alone: the difference is what classification adds;
          the same call against the composition on the device: ntru_decrypt_bytes_batch_dev, then torch ops (compare the tag, assemble
          the field, torch.bincount); the same two with G = 4096 groups (the table no longer fits the LDS histogram);
  (packed) ntru_count_bytes_packed_batch_dev against the dense call (the difference is the unpack) and against what exists for packed
          rows: ntru_decrypt_packed_batch_dev, ntru_rows_to_bytes_dev, then the torch ops;
  (host)  ntru_count_bytes_batch against ntru_decrypt_bytes_batch plus a numpy bincount, from pageable and from pinned arrays.
The host calls are timed with the host clock around calls that return synchronised, the device calls with device events.  Every
comparison also records whether both arms gave the same table.  Nothing is retried: any failure ends the run, and so does the time limit.
    python tools/bench_count.py [--reps 7] [--log-b 20] [--timeout 540] [--jsonl out.jsonl]"""
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
FIRST, CHOICES, FIELD_OFF, FIELD_LEN = 1, 8, 4, 2
BINS = CHOICES + 3
G_LARGE = 4096


def verdict(a, b, name_a, name_b):
    """Which arm's median is lower by more than both arms' max - min, or "level"."""
    gap = statistics.median(b) - statistics.median(a)
    spread = max(max(a) - min(a), max(b) - min(b))
    return "level" if abs(gap) <= spread else (name_a if gap > 0 else name_b) + " faster"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=7, help="alternating repeats (>= 5)")
    ap.add_argument("--log-b", type=int, default=20)
    ap.add_argument("--timeout", type=int, default=540, help="seconds after which the run gives up")
    ap.add_argument("--jsonl", default=None)
    a = ap.parse_args()
    signal.signal(signal.SIGALRM, lambda *_: sys.exit("bench_count: time limit of %d s reached" % a.timeout))
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
    h, f, fp = pad(k0["h"], np.uint16), pad(k0["f"], np.int8), pad(k0["fp"], np.uint8)
    key = np.arange(1, 9, dtype=np.uint32) * 0x9E3779B1
    ptr = lambda t: t.data_ptr()
    gen = torch.Generator(device=dev).manual_seed(1)
    d_h = torch.from_numpy(h.view(np.uint8)).to(dev)
    d_f, d_fp = torch.from_numpy(f).to(dev), torch.from_numpy(fp).to(dev)
    # the ballots: random bytes, the tag, the field = FIRST + a choice; 5 % get a wrong tag, 5 % are replaced by arbitrary rows
    tag_t = torch.tensor(list(TAG), dtype=torch.uint8, device=dev)
    d_msg = torch.randint(0, 256, (B, W), generator=gen, device=dev, dtype=torch.int32).to(torch.uint8)
    d_msg[:, :4] = tag_t
    choice = torch.randint(0, CHOICES, (B,), generator=gen, device=dev, dtype=torch.int32) + FIRST
    d_msg[:, FIELD_OFF] = (choice >> 8).to(torch.uint8)
    d_msg[:, FIELD_OFF + 1] = (choice & 255).to(torch.uint8)
    lot = torch.rand(B, generator=gen, device=dev)
    d_msg[:, 1] = torch.where(lot < 0.05, d_msg[:, 1] ^ 0x20, d_msg[:, 1])
    d_r = torch.empty((B, N), dtype=torch.uint8, device=dev)
    eng.sample_ternary_dev(N, dr, dr, P_MOD - 1, key, 0, B, ptr(d_r))
    d_e = torch.empty((B, N), dtype=torch.int16, device=dev)
    eng.encrypt_bytes_batch_dev(N, Q, W, ptr(d_h), ptr(d_r), ptr(d_msg), B, ptr(d_e))
    torch.cuda.synchronize()
    noise = torch.randint(0, Q, (B, N), generator=gen, device=dev, dtype=torch.int32).to(torch.int16)
    d_e = torch.where((lot >= 0.95)[:, None], noise, d_e).contiguous()
    del d_msg, d_r, noise, choice
    osz = eng.pack_params(Q - 1, N)["outputSize"]
    d_packed = torch.empty((B, osz, 4), dtype=torch.int64, device=dev)
    eng._chk(eng._lib.ntru_pack_batch_dev(eng._h, Q - 1, N, eng._dp(ptr(d_e)), B, eng._dp(ptr(d_packed))))
    d_bytes = torch.empty((B, W), dtype=torch.uint8, device=dev)
    d_flags = torch.empty((B,), dtype=torch.uint8, device=dev)
    d_value = torch.empty((B, N), dtype=torch.uint8, device=dev)
    d_group = torch.randint(0, G_LARGE, (B,), generator=gen, device=dev, dtype=torch.int32)
    d_count = torch.zeros(G_LARGE * BINS, dtype=torch.int64, device=dev)
    torch.cuda.synchronize()
    lay = dict(first_choice=FIRST, n_choices=CHOICES, field_off=FIELD_OFF, field_len=FIELD_LEN, tag=TAG, tag_off=0)
    results = []

    def emit(rec, line):
        results.append(dict(report, N=N, q=Q, nbytes=W, items=B, lift="centred", choices=CHOICES, **rec))
        print(line, flush=True)

    def compare(group, what, name_a, fn_a, name_b, fn_b, clock, same):
        """Both arms warmed up, then alternating; clock(fn) -> milliseconds of one call."""
        for fn in (fn_a, fn_b, fn_a, fn_b):
            fn()
        torch.cuda.synchronize()
        ms_a, ms_b = [], []
        for _ in range(reps):
            ms_a.append(clock(fn_a))
            ms_b.append(clock(fn_b))
        v = verdict(ms_a, ms_b, name_a, name_b)
        med_a, med_b = statistics.median(ms_a), statistics.median(ms_b)
        emit({"group": group, "case": what, "a": name_a, "b": name_b, "a_ms": round(med_a, 4), "a_spread_ms": round(max(ms_a) - min(ms_a), 4),
              "b_ms": round(med_b, 4), "b_spread_ms": round(max(ms_b) - min(ms_b), 4), "b_minus_a_ms": round(med_b - med_a, 4), "verdict": v,
              "same_result": same() if same else None, "a_M_rows_per_s": round(B / med_a / 1e3, 1)},
             "(%s) %-28s %s %9.3f ms (max - min %7.3f)   %s %9.3f ms (max - min %7.3f)   b - a %8.3f ms: %s%s" % (
                 group, what, name_a, med_a, max(ms_a) - min(ms_a), name_b, med_b, max(ms_b) - min(ms_b), med_b - med_a, v,
                 "" if same is None else "; same table: %s" % same()))

    def event_clock(fn):
        t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        t0.record()
        fn()
        t1.record()
        torch.cuda.synchronize()
        return t0.elapsed_time(t1)

    def host_clock(fn):
        t0 = time.perf_counter()
        fn()
        return (time.perf_counter() - t0) * 1e3

    # ---- (dev) and (packed) ---------------------------------------------------------------------------------------------------------
    got = {}

    def torch_table(groups, G):
        v = (d_bytes[:, FIELD_OFF].to(torch.int64) << 8) | d_bytes[:, FIELD_OFF + 1].to(torch.int64)
        cls = torch.where((v < FIRST) | (v - FIRST >= CHOICES), CHOICES, v - FIRST)
        cls = torch.where((d_bytes[:, :4] == tag_t).all(dim=1), cls, CHOICES + 1)
        cls = torch.where(d_flags == 0, cls, CHOICES + 2)
        got["torch"] = torch.bincount(cls if groups is None else groups.to(torch.int64) * BINS + cls, minlength=G * BINS)

    def decrypt_bytes():
        eng.decrypt_bytes_batch_dev(N, Q, P_MOD, W, ptr(d_f), ptr(d_fp), ptr(d_e), B, ptr(d_bytes), ptr(d_flags))

    def count_dev(groups=None, G=1, packed=False):
        fn = pkg.count_bytes_packed_batch_dev if packed else pkg.count_bytes_batch_dev
        fn(eng, N, Q, P_MOD, W, ptr(d_f), ptr(d_fp), ptr(d_packed) if packed else ptr(d_e), B, ptr(d_count),
           d_group=None if groups is None else ptr(groups), G=G, **lay)

    def composition(groups=None, G=1):
        decrypt_bytes()
        torch_table(groups, G)

    def composition_packed():
        pkg.decrypt_packed_batch_dev(eng, N, Q, P_MOD, ptr(d_f), ptr(d_fp), ptr(d_packed), B, ptr(d_value))
        eng.rows_to_bytes_dev(N, W, ptr(d_value), B, ptr(d_bytes), ptr(d_flags))
        torch_table(None, 1)

    same_dev = lambda G: (lambda: bool(torch.equal(d_count[:G * BINS], got["torch"])))
    compare("dev", "G = 1: what classifying adds", "count_dev", count_dev, "decrypt_bytes_dev", decrypt_bytes, event_clock, None)
    compare("dev", "G = 1: against torch", "count_dev", count_dev, "decrypt_bytes_dev + torch", composition, event_clock, same_dev(1))
    big = lambda: count_dev(d_group, G_LARGE)
    compare("dev", "G = 4096: what classifying adds", "count_dev", big, "decrypt_bytes_dev", decrypt_bytes, event_clock, None)
    compare("dev", "G = 4096: against torch", "count_dev", big, "decrypt_bytes_dev + torch", lambda: composition(d_group, G_LARGE), event_clock,
            same_dev(G_LARGE))
    compare("packed", "G = 1: the unpack", "count_dev", count_dev, "count_packed_dev", lambda: count_dev(packed=True), event_clock, None)
    compare("packed", "G = 1: against torch", "count_packed_dev", lambda: count_dev(packed=True), "decrypt_packed_dev + rows_to_bytes + torch",
            composition_packed, event_clock, same_dev(1))
    table = d_count[:BINS].cpu().numpy().copy()
    emit({"group": "table", "count": table.tolist()}, "table (G = 1): %s" % table.tolist())
    e_host = d_e.cpu().numpy().view(np.uint16)
    del d_packed, d_bytes, d_flags, d_value, d_group, d_count, d_e
    torch.cuda.empty_cache()

    # ---- (host) ---------------------------------------------------------------------------------------------------------------------
    lib, H = eng._lib, eng._h
    vp = lambda x: x.ctypes.data_as(ctypes.c_void_p)
    tag = np.frombuffer(TAG, np.uint8)
    tag_word = tag.view(np.uint32)[0]
    for memory in ("pageable", "pinned"):
        if memory == "pinned":
            e, out_bytes, out_flags = eng.pinned_empty((B, N), np.uint16), eng.pinned_empty((B, W), np.uint8), eng.pinned_empty((B,), np.uint8)
            e[:] = e_host
        else:
            e, out_bytes, out_flags = e_host, np.empty((B, W), np.uint8), np.empty(B, np.uint8)
        count = np.zeros((1, BINS), np.int64)
        res = {}

        def count_call():
            eng._chk(lib.ntru_count_bytes_batch(H, N, Q, P_MOD, W, vp(f), vp(fp), vp(e), B, 0, 4, vp(tag), FIELD_OFF, FIELD_LEN, FIRST, CHOICES, 1,
                                                None, vp(count), None))

        def composition_host():
            eng._chk(lib.ntru_decrypt_bytes_batch(H, N, Q, P_MOD, W, vp(f), vp(fp), vp(e), B, vp(out_bytes), vp(out_flags)))
            v = (out_bytes[:, FIELD_OFF].astype(np.int64) << 8) | out_bytes[:, FIELD_OFF + 1]
            cls = np.where((v < FIRST) | (v - FIRST >= CHOICES), CHOICES, v - FIRST)
            cls = np.where(np.ascontiguousarray(out_bytes[:, :4]).view(np.uint32)[:, 0] == tag_word, cls, CHOICES + 1)
            res["table"] = np.bincount(np.where(out_flags == 0, cls, CHOICES + 2), minlength=BINS)
        compare("host", "%s arrays, G = 1" % memory, "count_bytes_batch", count_call, "decrypt_bytes_batch + numpy", composition_host,
                host_clock, lambda: bool(np.array_equal(count[0], res["table"]) and np.array_equal(count[0], table)))
    if a.jsonl:
        with open(a.jsonl, "w") as fh:
            for r in results:
                fh.write(json.dumps(r) + "\n")
    signal.alarm(0)


if __name__ == "__main__":
    main()
