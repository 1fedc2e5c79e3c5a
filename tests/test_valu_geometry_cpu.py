"""tests/valu_geometry.py without a GPU: its restatement of the vector-ALU launchers against the variant table and the launchers'
own dispatch lists, and what the sweep of tests/test_valu_geometry_gpu.py covers and how many cases it runs."""
import os
import re

import kernel_variants as kv
import valu_geometry as vg

VALU_FAMILIES = ("k_encrypt<", "k_encrypt_t<", "k_decrypt<", "k_decrypt_t<", "k_decrypt_s<", "k_verify_keys<", "k_verify_keys_t<",
                 "k_polymul_split<")
VALU_ROWS = [r for r in kv.ROWS if r["entry"] in vg.ENTRIES and r["kernel"].startswith(VALU_FAMILIES)]
SOURCE = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "ntru-circom_amd", "csrc", "valu_families.hip")

# The distinct (entry, N, kernel path, q, p) the GPU module runs, each at three batch sizes.  A floor, so that the sweep cannot
# quietly shrink: 219 N (75 with several items per wave, 144 with one) give 7958 cases in 24964 calls.
CASE_FLOOR = 7900
ALL_CALLS = {(entry, K): vg.calls(entry, K) for entry in vg.ENTRIES for K in kv.K_RANGES}


def test_table_has_the_rows_this_module_speaks_of():
    assert len(VALU_ROWS) == 7 * 8 + 16, len(VALU_ROWS)           # seven families of eight, k_polymul_split<K, *>
    assert {r["last"] for r in VALU_ROWS} <= kv.LAST_KERNELS


def test_geometry_is_the_launchers():
    for N in range(2, vg.MAXN + 1):
        K, nl, G = vg.geom(N)
        lo, hi = kv.K_RANGES[K]
        assert lo <= N <= hi and K % 2 == 1, (N, K)
        assert nl == -(-N // (2 * K)) <= 64 and (K == 1 or -(-N // (2 * (K - 2))) > 64), (N, K, nl)
        assert G == 64 // nl >= 1 and G * nl <= 64, (N, nl, G)
        assert 1 <= vg.last_lane_fill(N) <= 2 * K and 2 * K * (nl - 1) + vg.last_lane_fill(N) == N, N


def dispatch_tuples(macro):
    """The VARIANT(K, ME, D8 tuples of one DISPATCH_* switch in valu_families.hip."""
    text = open(SOURCE).read()
    body = text[text.index("#define " + macro + "("):]
    body = body[:body.index("default:")]
    return sorted({tuple(int(x) for x in m) for m in re.findall(r"VARIANT\((\d+), (\d+), (\d+),", body)})


def test_expected_last_equals_the_table_on_every_vector_alu_shape():
    """Pins the restatement to the table (which tests/test_build_quality.py pins to the compiled library)."""
    checked = 0
    for r in VALU_ROWS:
        for s in r["shapes"]:
            got = vg.expected_last(r["entry"], s["N"], s["q"], s["p"], s["path"])
            if got is None:
                assert vg.matrix_may_apply(r["entry"], s["N"], s["q"], s["p"], s["path"]) and s["path"] == 0, (r["kernel"], s)
                continue
            assert got == r["last"], (r["kernel"], s, got)
            assert vg.accepted(r["entry"], s["N"], s["q"], s["p"]), (r["kernel"], s)
            checked += 1
    assert checked >= 2 * sum(1 for r in VALU_ROWS if r["shapes"]), checked
    # and the matrix-core rows of the same entries at kernel path 0 are where no name is predicted
    for r in kv.ROWS:
        if r["entry"] in vg.ENTRIES and r not in VALU_ROWS:
            for s in r["shapes"]:
                if s["path"] == 0:
                    assert vg.expected_last(r["entry"], s["N"], s["q"], s["p"], 0) is None, (r["kernel"], s)


def test_every_call_at_paths_1_to_3_is_predicted_and_names_a_table_kernel():
    for entry in vg.ENTRIES:
        p = 3 if entry in ("decrypt", "verify_keys", "public_key") else 0
        for N in range(2, vg.MAXN + 1):
            for q in (2048, 4096, 8192, 16384, 32768, 65536):
                for path in vg.PATHS:
                    name = vg.expected_last(entry, N, q, p, path)
                    assert (name is None) == vg.matrix_may_apply(entry, N, q, p, path) and (name is not None or path == 0)
                    if name is not None and not (entry == "verify_keys" and q == 32768):    # k_verify_keys_t<1,1>: the ABI refuses that q
                        assert name in kv.LAST_KERNELS, (entry, N, q, path, name)


def test_names_follow_the_dispatch_lists():
    """Every (K, ME[, dot8]) the restatement can name is one the launchers' switches hold, and the other way round."""
    add, shared = dispatch_tuples("DISPATCH_K_ADD"), dispatch_tuples("DISPATCH_K_SHARED")
    assert len(add) == 8 and len(shared) == 8, (add, shared)
    named_add, named_shared = set(), set()
    for N in range(2, vg.MAXN + 1):
        for q in (2048, 4096, 8192, 16384, 32768, 65536):
            me = vg.add_path_me(N, q, 2)
            if me:
                named_add.add((vg.pick_K(N), me, 0))
            for path in (2, 3):
                s = vg.shared_path(N, q, 3, path)
                if s:
                    named_shared.add((s[0], s[1], int(s[2])))
    assert sorted(named_add) == add and sorted(named_shared) == shared, (sorted(named_add), sorted(named_shared))


def test_sweep_ns_cover_the_geometries():
    every = [N for K in kv.K_RANGES for N in vg.sweep_ns(K)]
    assert len(every) == len(set(every)) and all(vg.pick_K(N) == K for K in kv.K_RANGES for N in vg.sweep_ns(K))
    assert len(every) >= 170, len(every)
    # several items per wave: every nl of K = 1, idle lanes among them, and K = 3 with two items per wave
    assert {vg.geom(N)[1] for N in vg.sweep_ns(1) if vg.geom(N)[2] > 1} == set(range(1, 33))
    assert set(range(2, 65)) <= set(vg.sweep_ns(1))
    assert {(vg.geom(N)[1], vg.geom(N)[2]) for N in vg.sweep_ns(3) if vg.geom(N)[2] > 1} == {(22, 2), (23, 2), (32, 2)}
    for K, (lo, hi) in kv.K_RANGES.items():
        ns = vg.sweep_ns(K)
        assert {lo, lo + 1, hi - 1, hi} <= set(ns), K
        one = [N for N in ns if vg.geom(N)[2] == 1]
        for nl in (63, 64):
            assert {vg.last_lane_fill(N) for N in one if vg.geom(N)[1] == nl} == {1, 2, 2 * K - 1, 2 * K}, (K, nl)
        nl_min = min(vg.geom(N)[1] for N in range(lo, hi + 1) if vg.geom(N)[2] == 1)
        assert any(vg.geom(N)[1] == nl_min for N in one) and any(nl_min < vg.geom(N)[1] < 63 for N in one), K
    # the shared stepping: both sides of each end of its 32-lane stretches
    for K in vg.SHARED_KS:
        for N in (62 * K - 1, 62 * K + 1, 64 * K - 1, 64 * K + 1):
            assert N in every, (K, N)


def test_sweep_reaches_every_add_path_and_shared_kernel_beyond_its_table_shapes():
    """Every reachable k_*_t<K,ME> and k_decrypt_s<K,ME,D8> row is launched at two N or more that are not shapes of its row, and every
    multiply-accumulate row as well."""
    n_of = {}
    for (entry, K), calls in ALL_CALLS.items():
        for c in calls:
            n_of.setdefault((entry, c["last"]), set()).add(c["N"])
    for r in VALU_ROWS:
        if r["unreachable"]:
            continue
        fresh = n_of.get((r["entry"], r["last"]), set()) - {s["N"] for s in r["shapes"]}
        assert len(fresh) >= 2, (r["kernel"], sorted(fresh))
    add, shared = dispatch_tuples("DISPATCH_K_ADD"), dispatch_tuples("DISPATCH_K_SHARED")
    launched = {vg.kernel_tuple(last) for _, last in n_of}
    for K, me, d8 in shared:
        assert ("k_decrypt_s+dot8" if d8 else "k_decrypt_s", K, me) in launched, (K, me, d8)
    for K, me, _ in add:
        for family in ("k_encrypt_t", "k_decrypt_t") + (("k_verify_keys_t",) if (K, me) != (1, 1) else ()):
            assert (family, K, me) in launched, (family, K, me)


def test_calls_of_the_sweep():
    cases = set()
    zero = set()                                 # (kernel, nl) that met variant 0: all q - 1 / all -1 operands
    every = set()
    for (entry, K), calls in ALL_CALLS.items():
        by_case = {}
        for c in calls:
            N, q, p, path = c["N"], c["q"], c["p"], c["path"]
            assert vg.accepted(entry, N, q, p) and c["last"] == vg.expected_last(entry, N, q, p, path), (entry, c)
            assert not (entry == "verify_keys" and p * (q - 1) > 65535), c          # the one documented refusal is never asked for
            Kk, nl, G = vg.kernel_geom(c["last"], N)
            every.add((c["last"], nl))
            if c["variant"] == 0:
                zero.add((c["last"], nl))
            if c["witness"]:
                by_case.setdefault((N, q, p, path), []).append(c["B"])
            else:
                assert entry == "decrypt" and p == 3, c
            if entry == "verify_keys" and G > 1:
                assert c["B"] == 1 or c["B"] >= 7, c
        for (N, q, p, path), Bs in by_case.items():
            G = vg.kernel_geom(vg.expected_last(entry, N, q, p, path), N)[2]
            assert Bs == vg.batch_sizes(entry, G) and Bs[0] == 1 and Bs[1] >= G + 1 and Bs[2] == 4 * G + 1, (entry, N, q, path, Bs)
            cases.add((entry, N, path, q, p))
        if entry == "decrypt":
            assert sum(not c["witness"] for c in calls) == len({k for k in by_case if k[2] == 3}), K
            assert {c["path"] for c in calls if c["p"] == 5} == {1}, K
        # every kernel name the ABI-accepted q of QS reach at an (N, path) is launched there
        for N in vg.sweep_ns(K):
            for p, paths in vg.ENTRY_P[entry]:
                for path in paths:
                    reach = {vg.expected_last(entry, N, q, p, path) for q in vg.QS
                             if vg.accepted(entry, N, q, p) and not (entry == "verify_keys" and p == 5 and q > 8192)} - {None}
                    assert reach == {c["last"] for c in calls if (c["N"], c["p"], c["path"]) == (N, p, path)}, (entry, N, p, path)
    assert zero == every, sorted(every - zero)[:8]
    assert len(cases) >= CASE_FLOOR, len(cases)
    assert {c[3] for c in cases} == set(vg.QS) | {3}
    assert {(c[0], c[4]) for c in cases} == {("encrypt", 0), ("decrypt", 3), ("decrypt", 5), ("verify_keys", 3), ("verify_keys", 5),
                                             ("polymul_split", 0), ("public_key", 3), ("public_key", 8)}
    assert all(sum(len(ALL_CALLS[entry, K]) for entry in vg.ENTRIES) for K in kv.K_RANGES)
