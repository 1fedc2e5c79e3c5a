#!/usr/bin/env python3
"""Launch times of the vector-ALU families (valu_families.hip), one kernel shape class per line, on seeded synthetic operands with the
witness arrays on (no result check: for same-device A/B of library builds).  HIP events around one call, 3 warm-up calls, 15 timed;
a line's figure is its fastest call.  A fresh process per library and round:
    NTRU_ENGINE_LIB=... python tools/time_valu_families.py [logB]"""
import os, sys
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch
import __graft_entry__ as ge
pkg = ge.load_package()
eng = pkg.Engine(0)
dev = torch.device("cuda:0")
eng.set_stream(torch.cuda.current_stream().cuda_stream)
logB = int(sys.argv[1]) if len(sys.argv) > 1 else 18
lib = os.path.basename(os.environ.get("NTRU_ENGINE_LIB", "default"))

def fastest(fn, warm=3, reps=15):
    for _ in range(warm): fn()
    best = float("inf")
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record(); fn(); b.record(); torch.cuda.synchronize()
        best = min(best, a.elapsed_time(b))
    return best

def run(N, q, B, cases):
    """cases: (call, kernel path, expected kernel)"""
    torch.manual_seed(N * 65536 + q)
    u16 = lambda hi: torch.randint(0, hi, (B, N), dtype=torch.int32, device=dev).to(torch.int16)
    tern = lambda: torch.randint(-1, 2, (B, N), dtype=torch.int8, device=dev)
    f, g = tern(), tern()
    fq, h, e = u16(q), u16(q), u16(q)
    fp, r = (torch.randint(0, 3, (B, N), dtype=torch.uint8, device=dev) for _ in range(2))
    m = torch.randint(0, 2, (B, N), dtype=torch.uint8, device=dev)
    o16 = [torch.empty((B, N), dtype=torch.int16, device=dev) for _ in range(4)]
    o8 = [torch.empty((B, N), dtype=torch.uint8, device=dev) for _ in range(2)]
    fl = torch.empty(B, dtype=torch.uint8, device=dev)
    p = lambda t: t.data_ptr()
    calls = {
        "encrypt": lambda: eng.encrypt_batch_dev(N, q, p(h[0]), p(r), p(m), B, p(o16[0]), p(o16[1])),
        "decrypt": lambda: eng.decrypt_batch_dev(N, q, 3, p(f[0]), p(fp[0]), p(e), B, p(o8[0]), p(o16[0]), p(o16[1]), p(o8[1])),
        "verify_keys": lambda: eng.verify_keys_batch_dev(N, q, 3, p(f), p(g), p(fq), p(fp), p(h), B, p(o16[0]), p(o16[1]), p(o8[0]), p(o8[1]),
                                                         p(o16[2]), p(o16[3]), p(fl)),
        "polymul_split": lambda: eng.polymul_split_dev(N, q, p(fq), p(h), B, p(o16[0]), p(o16[1])),
        "public_key": lambda: eng.public_key_batch_dev(N, q, 3, p(fq), p(g), B, p(o16[0])),
    }
    for call, path, kernel in cases:
        eng.set_kernel_path(path)
        ms = fastest(calls[call])
        assert eng.last_kernel() == kernel, (call, path, eng.last_kernel(), kernel)
        print("lib %s  N=%d q=%d B=2^%d path %d  %-24s %.4f ms" % (lib, N, q, B.bit_length() - 1, path, kernel, ms), flush=True)
    eng.set_kernel_path(0)

B = 1 << logB
run(821, 4096, B, [("encrypt", 2, "k_encrypt_t<7,14>"), ("decrypt", 2, "k_decrypt_s+dot8<13,13>"), ("decrypt", 3, "k_decrypt_s<13,13>"),
                   ("verify_keys", 2, "k_verify_keys_t<7,14>"), ("encrypt", 1, "k_encrypt<7>"), ("decrypt", 1, "k_decrypt<7>"),
                   ("verify_keys", 1, "k_verify_keys<7>"), ("polymul_split", 1, "k_polymul_split<7>"), ("public_key", 1, "k_public_key<7>")])
run(701, 8192, B, [("encrypt", 2, "k_encrypt_t<7,7>"), ("decrypt", 2, "k_decrypt_s+dot8<11,7>")])
run(820, 4096, B, [("decrypt", 2, "k_decrypt_t<7,14>")])
run(17, 32, 4 * B, [("encrypt", 1, "k_encrypt<1>"), ("decrypt", 1, "k_decrypt<1>")])
