"""Sums of ciphertexts in groups, the parts that need no GPU: the build of ciphertext_sum.hip (no spills, the documented kernels, no
scalar memory writes), the tally fixture against its generator and against the numpy restatement the GPU tests check with, and the
argument checks of the new entry points."""
import filecmp
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

import __graft_entry__ as ge
import ciphertext_sum_ref as ref

pkg = ge.load_package()
NEW_SYMBOLS = ["ntru_sum_groups", "ntru_sum_groups_dev", "ntru_tally_decrypt_batch", "ntru_tally_decrypt_batch_dev"]
# scalar stores, scalar atomics and the scalar data cache write-back: not allowed on the shared machines
FORBIDDEN = [a + b for a, b in (("s_st", "ore"), ("s_buffer_st", "ore"), ("s_scratch_st", "ore"), ("s_ato", "mic"), ("s_buffer_ato", "mic"),
                                ("s_dcache_", "wb"), ("s_dcache_", "discard"))]


@pytest.fixture(scope="module")
def lib():
    ge.build()
    return pkg.load_library()


def test_new_symbols_are_exported(lib):
    for name in NEW_SYMBOLS:
        assert hasattr(lib, name), name
    assert callable(pkg.sumCiphertexts) and callable(pkg.NTRU.tallyBatch)
    assert callable(pkg.Engine.sum_groups_dev) and callable(pkg.Engine.tally_decrypt_batch_dev)


def test_new_translation_unit(tmp_path):
    """`make asm` of ciphertext_sum.hip: the documented kernel set, ScratchSize 0 everywhere, none of the forbidden mnemonics."""
    src = os.path.join(ge.PKG_DIR, "csrc")
    out = subprocess.run(["make", "-C", src, "ASMDIR=%s" % tmp_path, "%s/ciphertext_sum.s" % tmp_path], capture_output=True, text=True,
                         timeout=900)
    assert out.returncode == 0, out.stderr[-2000:]
    text = open(os.path.join(str(tmp_path), "ciphertext_sum.usage")).read()
    names = re.findall(r"Function Name: (\S+)", text)
    scratch = [int(x) for x in re.findall(r"ScratchSize \[bytes/lane\]: (\d+)", text)]
    # k_sum_groups<power of two?, weighted?> and k_sum_groups_finish<power of two?>
    assert len(names) == 6 and len(scratch) == 6, text[-2000:]
    assert sum("k_sum_groups_finish" in n for n in names) == 2 and sum("12k_sum_groupsILb" in n for n in names) == 4, names
    assert scratch == [0] * 6, list(zip(names, scratch))
    isa = open(os.path.join(str(tmp_path), "ciphertext_sum.s")).read().lower()
    source = open(os.path.join(src, "ciphertext_sum.hip")).read().lower()
    for word in FORBIDDEN:
        assert word not in isa and word not in source, word
    assert "global_load_dwordx4" in isa                    # 16 bytes per lane on the row loads


def test_fixture_regenerates_byte_identically(tmp_path):
    refdir = os.environ.get("NTRU_REFERENCE_DIR", "/root/reference")
    if not os.path.exists(os.path.join(refdir, "index.js")) or not shutil.which("node"):
        pytest.skip("the reference tree or node is not present")
    gen = os.path.join(ge.ROOT, "tests", "golden", "gen_tally_cases.mjs")
    subprocess.run(["node", gen, refdir, str(tmp_path)], check=True, capture_output=True, timeout=600)
    assert filecmp.cmp(os.path.join(str(tmp_path), "tally_cases.json"), ref.GOLDEN, shallow=False)
    assert os.path.getsize(ref.GOLDEN) < (1 << 20)


def test_fixture_shape_and_recovery_share():
    cases = ref.load_cases()
    main = [c for c in cases if c["set"] in ("n167_q128_low_noise", "n509_q2048")]
    assert sorted({(c["set"], c["K"]) for c in main if c["weights"] is None}) == [
        ("n167_q128_low_noise", 2), ("n167_q128_low_noise", 4), ("n167_q128_low_noise", 8),
        ("n509_q2048", 2), ("n509_q2048", 4), ("n509_q2048", 8), ("n509_q2048", 16), ("n509_q2048", 32)]
    assert any(c["weights"] for c in main)
    assert 4 * sum(c["recovered"] for c in main) >= 3 * len(main)
    assert {c["set"] for c in cases} >= {"n167_q128_default", "n167_q4096_default"}
    for c in cases:
        N, p = c["options"]["N"], c["options"]["p"]
        want = np.zeros(N, np.int64)
        for k, m in enumerate(c["m"]):
            want += (c["weights"][k] if c["weights"] else 1) * np.array(m)
        assert (want % p).tolist() == c["expected"]
        value = c["decrypt"]["value"] + [0] * (N - len(c["decrypt"]["value"]))
        assert (value == c["expected"]) == c["recovered"]
        assert c["decrypt"]["inputs"]["e"] == c["sum"]


def test_numpy_restatement_equals_the_reference_sums():
    for c in ref.load_cases():
        N, q, p, f, fp, rows, w, total = ref.case_arrays(c)
        K = rows.shape[0]
        assert np.array_equal(ref.np_sum(rows, q, K=K, weights=w)[0], total), (c["set"], c["K"])
        assert np.array_equal(ref.np_sum(rows, q, offsets=[0, K], weights=w, chunk=3)[0], total)


def test_numpy_restatement_on_ragged_groups():
    g = np.random.default_rng(1)
    rows = g.integers(0, 65521, (40, 5)).astype(np.uint16)
    w = g.integers(0, 65521, 40).astype(np.uint16)
    offsets = [2, 2, 9, 10, 10, 10, 33, 40, 40]
    for chunk in (1, 4, 7, 64):
        got = ref.np_sum(rows, 65521, offsets=offsets, weights=w, chunk=chunk)
        for i in range(len(offsets) - 1):
            want = sum(int(w[r]) * rows[r].astype(object) for r in range(offsets[i], offsets[i + 1])) if offsets[i + 1] > offsets[i] else 0
            assert np.array_equal(got[i].astype(object), (want % 65521) + np.zeros(5, dtype=object)), (chunk, i)


def test_argument_errors_without_a_gpu(lib):
    """Domain checks run on the host before the engine is looked at: NTRU_ERR_ARG with a message."""
    s, sd, t, td = lib.ntru_sum_groups, lib.ntru_sum_groups_dev, lib.ntru_tally_decrypt_batch, lib.ntru_tally_decrypt_batch_dev
    tail = [None] * 5
    cases = [
        (s, [None, 1, 32, None, None, None, 1, 1, None], "N"),
        (sd, [None, 1921, 32, None, None, None, 1, 1, None], "N"),
        (s, [None, 17, 1, None, None, None, 1, 1, None], "mod"),
        (sd, [None, 17, 65537, None, None, None, 1, 1, None], "mod"),
        (s, [None, 17, 32, None, None, None, 0, 1, None], "K >= 1"),
        (sd, [None, 17, 32, None, None, None, 1, -1, None], "negative"),
        (s, [None, 17, 32, None, None, None, 1 << 40, 1 << 40, None], "out of range"),
        (t, [None, 17, 32, 3, None, None, None, None, None, 0, 1] + tail, "K >= 1"),
        (td, [None, 0, 32, 3, None, None, None, None, None, 1, 1] + tail, "N"),
        (s, [None, 17, 32, None, None, None, 1, 1, None], "engine is NULL"),
        (td, [None, 17, 32, 3, None, None, None, None, None, 1, 1] + tail, "engine is NULL"),
    ]
    for fn, args, word in cases:
        assert fn(*args) == 2, (fn.__name__, args)
        assert word in lib.ntru_last_error().decode(), (fn.__name__, args, lib.ntru_last_error())


def test_python_shim_refuses_malformed_groups():
    rows = np.zeros((6, 17), np.uint16)
    for kw, word in (({"K": 4}, "whole groups"), ({"offsets": [0, 7]}, "offsets"), ({"K": 3, "weights": [1, 2]}, "one weight")):
        with pytest.raises(ValueError, match=word):
            pkg.Engine._groups(rows, kw.get("offsets"), kw.get("K"), kw.get("weights"))
