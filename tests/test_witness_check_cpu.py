"""Witness checks on the CPU: the two evaluators of tests/witness_circuit.py against each other and against the reference-captured
witnesses, the argument checks of ntru_check_*_batch without a GPU, and the build of the new kernel translation unit."""
import os
import re
import subprocess

import numpy as np
import pytest

import __graft_entry__ as ge
import witness_circuit as wc
from conftest import PROFILES, load_golden

pkg = ge.load_package()
NEW_SYMBOLS = ["ntru_check_%s_batch%s" % (t, s) for t in ("encrypt", "decrypt", "inverse") for s in ("", "_dev")]


@pytest.fixture(scope="module")
def golden():
    return wc.golden_witnesses(load_golden, PROFILES)


@pytest.fixture(scope="module")
def lib():
    ge.build()
    return pkg.load_library()


def test_literal_evaluator_accepts_every_golden_witness(golden):
    assert {t: len(v) for t, v in golden.items()} == {"VerifyEncrypt": 53, "VerifyDecrypt": 101, "VerifyInverse": 24}
    for template, ws in golden.items():
        flags = [wc.literal(template, w) for w in ws]
        assert flags == [0] * len(ws), template


def test_closed_form_equals_literal_modulus_and_less_than():
    for M in range(2, 41):
        for n in range(1, 8):
            xs = np.arange(1 << (n + 2))
            y, ok = wc.modulus_closed(M, n, xs)
            for x in xs.tolist():
                ly, lok = wc.modulus(M, n, x)
                assert (ly, lok) == (y[x], ok[x]), (M, n, x)
    for n in range(1, 8):
        for a in range(0, 1 << (n + 1)):
            xs = np.arange(1 << (n + 2))
            out, ok = wc.less_than_closed(n, a, xs)
            for x in xs.tolist():
                lout, lok = wc.less_than(n, a, x)
                assert lok == ok[x], (n, a, x)
                if lok:
                    assert lout == out[x], (n, a, x)


@pytest.mark.parametrize("template", wc.TEMPLATES)
def test_numpy_evaluator_equals_literal(golden, template):
    rng = np.random.default_rng(11)
    seen = set()
    for params, ws in wc.by_params(golden[template]).items():
        small = params[-1] <= 167
        batch = list(ws)
        for w in ws[:2]:
            batch += wc.mutations(template, w, rng, 200 if small else 12)
        p, arrays = wc.stack(template, batch)
        got = wc.numpy_check(template, p, arrays)
        want = [wc.literal(template, w) for w in batch]
        assert got.tolist() == want, params
        seen |= set(want)
    assert 0 in seen and len(seen) >= 3, seen                 # mutations do reach the flags


def test_tight_np_rejects_honest_decrypt_at_q8192():
    """calculateNp() at N = 167, p = 3 is 11: Modulus(3, 11) gets remainder1[i] + gt past T(3, 11) = 3071 when q = 8192."""
    assert wc.T_bound(3, 11) == 3071
    rng = np.random.default_rng(5)
    N, p = 167, 3
    for q, want in ((8192, 32), (2048, 0)):
        f = rng.choice([0, 1, q - 1], (4, N))
        arrays = wc.honest_decrypt(q, p, N, f, rng.integers(0, p, (4, N)), rng.integers(0, q, (4, N)))
        params = (q, wc.calc_nbits(q, N), p, wc.calc_nbits(p, N), N)
        assert params[3] == 11
        assert wc.numpy_check("VerifyDecrypt", params, arrays).tolist() == [want] * 4
        assert [wc.literal("VerifyDecrypt", wc.witness("VerifyDecrypt", params, arrays, i)) for i in range(4)] == [want] * 4


def test_new_symbols_are_exported(lib):
    for name in NEW_SYMBOLS:
        assert hasattr(lib, name), name


def test_argument_errors_without_a_gpu(lib):
    """Domain checks run on the host before the engine is looked at: NTRU_ERR_ARG with a message."""
    enc, dec, inv = lib.ntru_check_encrypt_batch, lib.ntru_check_decrypt_batch, lib.ntru_check_inverse_batch
    encd, decd, invd = lib.ntru_check_encrypt_batch_dev, lib.ntru_check_decrypt_batch_dev, lib.ntru_check_inverse_batch_dev
    nul5, nul7, nul4 = [None] * 5, [None] * 7, [None] * 4
    cases = [
        (enc, [None, 1, 32, 15] + nul5 + [1, None], "N"),
        (enc, [None, 1921, 32, 15] + nul5 + [1, None], "N"),
        (encd, [None, 17, 1, 15] + nul5 + [1, None], "q"),
        (encd, [None, 17, 65537, 15] + nul5 + [1, None], "q"),
        (enc, [None, 17, 32, 0] + nul5 + [1, None], "bit count"),
        (enc, [None, 17, 32, 253] + nul5 + [1, None], "bit count"),
        (dec, [None, 17, 33, 15, 3, 8] + nul7 + [1, None], "even"),
        (decd, [None, 17, 32, 15, 1, 8] + nul7 + [1, None], "p"),
        (dec, [None, 17, 32, 15, 3, 300] + nul7 + [1, None], "bit count"),
        (inv, [None, 17, 70000, 15] + nul4 + [1, None], "M"),
        (invd, [None, 0, 3, 8] + nul4 + [1, None], "N"),
        (inv, [None, 17, 3, 8] + nul4 + [-1, None], "negative"),
        (enc, [None, 17, 32, 15] + nul5 + [1, None], "engine is NULL"),
        (decd, [None, 17, 32, 15, 3, 8] + nul7 + [0, None], "engine is NULL"),
    ]
    for fn, args, word in cases:
        assert fn(*args) == 2, (fn.__name__, args)
        assert word in lib.ntru_last_error().decode(), (fn.__name__, args, lib.ntru_last_error())


def test_new_translation_unit_does_not_spill(tmp_path):
    """`make asm` of witness_check.hip: every kernel reports ScratchSize 0."""
    src = os.path.join(ge.PKG_DIR, "csrc")
    out = subprocess.run(["make", "-C", src, "ASMDIR=%s" % tmp_path, "%s/witness_check.s" % tmp_path], capture_output=True, text=True,
                         timeout=900)
    assert out.returncode == 0, out.stderr[-2000:]
    text = open(os.path.join(str(tmp_path), "witness_check.usage")).read()
    names = re.findall(r"Function Name: (\S+)", text)
    scratch = [int(x) for x in re.findall(r"ScratchSize \[bytes/lane\]: (\d+)", text)]
    assert len(names) == 3 and len(scratch) == 3, text[-2000:]
    for kern in ("k_check_encrypt", "k_check_decrypt", "k_check_inverse"):
        assert any(kern in n for n in names), kern
    assert scratch == [0, 0, 0], list(zip(names, scratch))


def test_python_mirror_refuses_malformed_witnesses(golden):
    """checkWitnesses validates on the host, before any engine is needed."""
    enc = golden["VerifyEncrypt"][0]
    other = next(w for w in golden["VerifyEncrypt"] if w["params"] != enc["params"])

    def changed(name, idx, value):
        w = {"params": enc["params"], "inputs": dict(enc["inputs"])}
        w["inputs"][name] = list(enc["inputs"][name])
        if idx is None:
            w["inputs"][name].pop()
        else:
            w["inputs"][name][idx] = value
        return w
    for args, word in ((("VerifyEncrypt", [enc, other]), "params"), (("VerifyEncrypt", [changed("r", None, 0)]), "length"),
                       (("VerifyEncrypt", [changed("m", 1, 65536)]), "65535"), (("VerifyEncrypt", [changed("h", 0, -1)]), "65535"),
                       (("VerifyEncrypt", [changed("h", 0, 1.5)]), "65535"), (("VerifyInverse", [enc]), "missing signal"),
                       (("VerifyCombine", [enc]), "unknown template")):
        with pytest.raises(ValueError, match=word):
            pkg.checkWitnesses(*args)
    assert pkg.checkWitnesses("VerifyDecrypt", []) == []
