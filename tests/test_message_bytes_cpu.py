"""Byte messages as packed bits, the parts that need no GPU: the build of message_bytes.hip (no spills), the bytes fixture against its
generator and against the numpy restatement the GPU tests check with, the exported symbols and the host-side argument checks."""
import filecmp
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

import __graft_entry__ as ge
import message_bytes_ref as ref

pkg = ge.load_package()
NEW_SYMBOLS = [n + s for n in ("ntru_bytes_to_rows", "ntru_rows_to_bytes", "ntru_encrypt_bytes_batch", "ntru_decrypt_bytes_batch")
               for s in ("", "_dev")] + ["ntru_pipeline_bytes_batch"]


@pytest.fixture(scope="module")
def lib():
    ge.build()
    return pkg.load_library()


@pytest.fixture(scope="module")
def sets():
    return ref.load_sets()


def test_new_symbols_are_exported(lib):
    for name in NEW_SYMBOLS:
        assert hasattr(lib, name), name
    for name in ("bytes_to_rows", "rows_to_bytes", "encrypt_bytes_batch", "decrypt_bytes_batch"):
        assert callable(getattr(pkg.Engine, name)) and callable(getattr(pkg.Engine, name + "_dev")), name
    assert callable(pkg.Engine.pipeline_bytes_batch)
    assert callable(pkg.NTRU.encryptBytes) and callable(pkg.NTRU.decryptBytes)
    assert pkg.NTRU({"N": 821}).bytesPerBlock == 102 and pkg.NTRU({"N": 17}).bytesPerBlock == 2
    assert (pkg.FLAG_NOT_BITS, pkg.FLAG_PAD_NONZERO) == (ref.FLAG_NOT_BITS, ref.FLAG_PAD_NONZERO) == (32, 64)


def test_new_translation_unit(tmp_path):
    """`make asm` of message_bytes.hip: the two codec kernels, ScratchSize 0 for both, 16 bytes per lane on the wide side of each."""
    src = os.path.join(ge.PKG_DIR, "csrc")
    out = subprocess.run(["make", "-C", src, "ASMDIR=%s" % tmp_path, "%s/message_bytes.s" % tmp_path], capture_output=True, text=True,
                         timeout=900)
    assert out.returncode == 0, out.stderr[-2000:]
    text = open(os.path.join(str(tmp_path), "message_bytes.usage")).read()
    names = re.findall(r"Function Name: (\S+)", text)
    scratch = [int(x) for x in re.findall(r"ScratchSize \[bytes/lane\]: (\d+)", text)]
    assert len(names) == 2 and len(scratch) == 2, text[-2000:]
    assert sum("k_bytes_to_rows" in n for n in names) == 1 and sum("k_rows_to_bytes" in n for n in names) == 1, names
    assert scratch == [0, 0], list(zip(names, scratch))
    isa = open(os.path.join(str(tmp_path), "message_bytes.s")).read()
    assert "global_load_dwordx4" in isa and "global_store_dwordx4" in isa
    assert "global_atomic" not in isa and "flat_atomic" not in isa          # the flags are gathered in the LDS


def test_fixture_regenerates_byte_identically(tmp_path):
    refdir = os.environ.get("NTRU_REFERENCE_DIR", "/root/reference")
    if not os.path.exists(os.path.join(refdir, "index.js")) or not shutil.which("node"):
        pytest.skip("the reference tree or node is not present")
    gen = os.path.join(ge.ROOT, "tests", "golden", "gen_bytes_cases.mjs")
    subprocess.run(["node", gen, refdir, str(tmp_path)], check=True, capture_output=True, timeout=600)
    assert filecmp.cmp(os.path.join(str(tmp_path), "bytes_cases.json"), ref.GOLDEN, shallow=False)
    assert os.path.getsize(ref.GOLDEN) < (1 << 20)


def test_fixture_shape(sets):
    assert [(s["options"]["N"], s["options"]["q"], s["options"]["df"]) for s in sets] == [(17, 32, 3), (167, 128, 20), (167, 128, 61),
                                                                                         (509, 2048, 40)]
    for s in sets:
        W = s["W"]
        assert W == s["options"]["N"] // 8
        lengths = [m["length"] for m in s["messages"]]
        assert set(lengths) >= {1, W, W + 1, 2 * W, 3 * W + 1} | ({W - 1} if W > 1 else set())
        data = b"".join(m["data"] for m in s["messages"])
        if W > 2:
            assert 0x00 in data and 0xff in data
        for m in s["messages"]:
            assert len(m["data"]) == m["length"] and len(m["blocks"]) == -(-m["length"] // W)
            assert all(b["chunk"][-1] != 0 for b in m["blocks"])               # decryptStr trims trailing zeros
            assert all(len(b["chunk"]) == W for b in m["blocks"][:-1])


def test_restatement_reproduces_every_fixture_block(sets):
    """Expansion = the recorded stringToBits padded to N; collection of the recorded decrypted row, trailing zeros stripped, = the
    recorded decryptStr = the chunk, with flags 0."""
    for s in sets:
        N, W = s["options"]["N"], s["W"]
        for m in s["messages"]:
            for b in m["blocks"]:
                n = len(b["chunk"])
                chunk = np.array([b["chunk"]], np.uint8)
                assert ref.np_bytes_to_rows(chunk, N)[0].tolist() == b["bits"] + [0] * (N - 8 * n)
                padded = np.array([b["chunk"] + [0] * (W - n)], np.uint8)
                assert ref.np_bytes_to_rows(padded, N)[0].tolist() == b["bits"] + [0] * (N - 8 * n)
                out, flags = ref.np_rows_to_bytes(np.array([b["decrypted"]], np.uint8), W)
                assert int(flags[0]) == 0
                assert out[0].tobytes().rstrip(b"\x00") == bytes(b["str"]) == bytes(b["chunk"])
                assert len(b["r"]) == N and len(b["value"]) == N and set(b["r"]) <= {0, 1, 2}


def test_restatement_flags_and_round_trip():
    g = np.random.default_rng(5)
    for N, nbytes in ((8, 1), (17, 1), (17, 2), (167, 19), (821, 102)):
        data = g.integers(0, 256, (9, nbytes), dtype=np.uint8)
        rows = ref.np_bytes_to_rows(data, N)
        assert rows.shape == (9, N) and rows.max() <= 1 and not rows[:, 8 * nbytes:].any()
        assert rows[0, 0] == data[0, 0] >> 7 and rows[0, 7] == data[0, 0] & 1
        out, flags = ref.np_rows_to_bytes(rows, nbytes)
        assert np.array_equal(out, data) and not flags.any()
        rows[1, 0] = 2
        rows[2, 8 * nbytes - 1] = 3
        if 8 * nbytes < N:
            rows[3, 8 * nbytes] = 1
            rows[4, N - 1] = 2
        want = [0, 32, 32] + ([64, 64] if 8 * nbytes < N else [0, 0]) + [0] * 4
        out, flags = ref.np_rows_to_bytes(rows, nbytes)
        assert flags.tolist() == want
        assert out[2, -1] == (data[2, -1] | 1) and out[1, 0] == data[1, 0] & 0x7f          # bit = value & 1


def test_argument_errors_without_a_gpu(lib):
    """Domain checks run on the host before the engine is looked at: NTRU_ERR_ARG with a message."""
    b2r, r2b, enc, dec = lib.ntru_bytes_to_rows, lib.ntru_rows_to_bytes_dev, lib.ntru_encrypt_bytes_batch, lib.ntru_decrypt_bytes_batch_dev
    pipe = lib.ntru_pipeline_bytes_batch
    cases = [
        (b2r, [None, 7, 1, None, 1, None], "N"),
        (b2r, [None, 1921, 1, None, 1, None], "N"),
        (b2r, [None, 17, 0, None, 1, None], "nbytes"),
        (r2b, [None, 17, 3, None, 1, None, None], "nbytes"),
        (r2b, [None, 17, 2, None, -1, None, None], "negative"),
        (enc, [None, 821, 4096, 103, None, None, None, 1, None, None], "nbytes"),
        (dec, [None, 7, 4096, 3, 1, None, None, None, 1, None, None], "N"),
        (pipe, [None, 821, 4096, 3, None, None, None, None, 0, 0, 0, None, 0, None, 1, None, None, None, None], "nbytes"),
        (b2r, [None, 17, 2, None, 1, None], "engine is NULL"),
        (dec, [None, 17, 32, 3, 2, None, None, None, 1, None, None], "engine is NULL"),
    ]
    for fn, args, word in cases:
        assert fn(*args) == 2, (fn.__name__, args)
        assert word in lib.ntru_last_error().decode(), (fn.__name__, args, lib.ntru_last_error())


def test_python_shim_refuses_wide_strings_without_a_gpu():
    ntru = pkg.NTRU({"N": 167, "q": 128, "h": [1, 2, 3]})
    with pytest.raises(ValueError, match="latin-1"):
        ntru.encryptBytes("snow ☃")
    with pytest.raises(ValueError, match="rows of r"):
        ntru.encryptBytes(b"x" * 21, r=[[0] * 167])
