"""ntru_keygen_batch[_dev] on the GPU: every item against a CPU replay of its documented stream positions (include/ntru_engine.h),
full-size batches against the sampler, verify_keys and the oracle, and agreement with the chain it replaces."""
import os

import numpy as np
import pytest

import __graft_entry__ as ge
from oracle import ntru_keygen as kg
from oracle import ntru_oracle as orc
from keygen_ref import key_pairs, replay

pytestmark = pytest.mark.gpu
pkg = ge.load_package()

KEY = np.array([0x9E3779B9 * (i + 1) & 0xFFFFFFFF for i in range(8)], np.uint32)
NOT_UNIT = pkg.engine.FLAG_NOT_UNIT_MOD2 | pkg.engine.FLAG_NOT_UNIT_MODP
SMALL = {  # name: (N, q, df, dg) -- parameter sets with many non-units among the draws
    "n17_q32": (17, 32, 3, 2),
    "n7": (7, 32, 2, 2),
    "n31": (31, 64, 8, 5),
}


@pytest.fixture(scope="module")
def eng():
    return pkg.Engine(0)


@pytest.fixture(scope="module")
def torch_dev():
    import torch
    return torch, torch.device("cuda:0")


def options(name):
    return ge_golden(name)["options"]


def ge_golden(name):
    import json
    with open(os.path.join(ge.ROOT, "tests", "golden", "scheme_%s.json" % name)) as fh:
        return json.load(fh)


def check_against_replay(N, q, out, want):
    f, g, tries, flags = want
    assert np.array_equal(out["tries"], tries)
    assert np.array_equal(out["flags"], flags)
    assert np.array_equal(out["f"], f)
    assert np.array_equal(out["g"], g)
    ok = flags == 0
    if ok.any():
        v = orc.verify_keys_batch(N, q, 3, out["f"][ok], out["g"][ok], out["fq"][ok], out["fp"][ok], out["h"][ok])
        assert not v["flags"].any()
        assert np.array_equal(orc.public_key_batch(N, q, 3, out["fq"][ok], out["g"][ok]), out["h"][ok])
    for name in ("fq", "fp", "h"):
        assert not out[name][~ok].any(), name


@pytest.mark.parametrize("name,B", [("n17_q32", 4096), ("n7", 3000), ("n31", 2000)])
def test_natural_non_units_replay(eng, name, B):
    N, q, df, dg = SMALL[name]
    out = eng.keygen_batch(N, q, 3, df, dg, KEY, B, first_item=123, max_tries=100)
    want = replay(N, df, dg, KEY, 123, B, 100)
    assert (want[2] > 1).any()                     # the set does redraw
    check_against_replay(N, q, out, want)


@pytest.mark.parametrize("max_tries", [1, 2])
def test_exhaustion(eng, max_tries):
    N, q, df, dg = SMALL["n7"]
    B = 1000
    out = eng.keygen_batch(N, q, 3, df, dg, KEY, B, first_item=5, max_tries=max_tries)
    want = replay(N, df, dg, KEY, 5, B, max_tries)
    failed = want[3] != 0
    assert failed.any() and (want[2][failed] == max_tries).all()
    assert not (out["flags"] & 1).any()
    check_against_replay(N, q, out, want)


def test_more_non_units_than_one_pass(eng):
    """N = 7 at B = 2^15: about 13000 first draws are non-units, more than one redraw pass holds."""
    N, q, df, dg = SMALL["n7"]
    B = 1 << 15
    out = eng.keygen_batch(N, q, 3, df, dg, KEY, B, first_item=0, max_tries=40)
    assert (out["tries"] > 1).sum() > 4096
    want = replay(N, df, dg, KEY, 0, B, 40)
    check_against_replay(N, q, out, want)


def test_listed_draw_fills_whole_blocks_of_compact_rows(eng):
    """N = 16, B = 256: 135 items wait after the first attempt and 65 after the second, so the listed draw writes two full blocks of 64
    compact rows plus seven, then one full block plus one: full blocks with N >= 16 leave through the sampler's aligned output stage,
    the rest row by row.  Every field against the CPU replay."""
    N, q, df, dg, B, tries = 16, 32, 3, 2, 256, 6
    key = np.arange(1, 9, dtype=np.uint32)
    want = key_pairs(N, q, df, dg, key, 0, B, tries)
    assert int((want["tries"] >= 2).sum()) == 135 and int((want["tries"] >= 3).sum()) == 65    # the oracle still exercises the path
    out = eng.keygen_batch(N, q, 3, df, dg, key, B, first_item=0, max_tries=tries)
    for name in ("tries", "flags", "f", "g", "fq", "fp", "h"):
        assert np.array_equal(out[name], want[name]), name


@pytest.mark.parametrize("name", ["n821_q4096", "n701_q8192", "n509_q2048"])
def test_full_size(eng, torch_dev, name):
    torch, dev = torch_dev
    o = options(name)
    N, q, df, dg = o["N"], o["q"], o["df"], o["dg"]
    B = 1 << 16
    d = lambda dt, shape=(B, N): torch.empty(shape, dtype=dt, device=dev)
    f, g, fq, fp, h = d(torch.int8), d(torch.int8), d(torch.int16), d(torch.uint8), d(torch.int16)
    tries, flags = d(torch.uint8, (B,)), d(torch.uint8, (B,))
    work = d(torch.uint8, (eng.keygen_workspace_bytes(N, B),))
    eng.keygen_batch_dev(N, q, 3, df, dg, KEY, 0, 100, B, work.data_ptr(), f.data_ptr(), g.data_ptr(), fq.data_ptr(), fp.data_ptr(),
                         h.data_ptr(), tries.data_ptr(), flags.data_ptr())
    torch.cuda.synchronize()
    assert not flags.any().item()
    fs, gs = d(torch.uint8), d(torch.uint8)
    eng.sample_ternary_dev(N, df, df - 1, 255, KEY, 0, B, fs.data_ptr())
    eng.sample_ternary_dev(N, dg, dg, 255, KEY, 1 << 40, B, gs.data_ptr())
    first = tries == 1
    assert torch.equal(gs.view(torch.int8), g)
    assert torch.equal(fs.view(torch.int8)[first], f[first])
    o16, o8 = lambda: d(torch.int16), lambda: d(torch.uint8)
    ws = [o16(), o16(), o8(), o8(), o16(), o16()]
    vfl = d(torch.uint8, (B,))
    eng.verify_keys_batch_dev(N, q, 3, f.data_ptr(), g.data_ptr(), fq.data_ptr(), fp.data_ptr(), h.data_ptr(), B,
                              *[w.data_ptr() for w in ws], vfl.data_ptr())
    torch.cuda.synchronize()
    assert not vfl.any().item()
    assert torch.equal(ws[5], h)
    rows = torch.arange(0, B, B // 1024, device=dev)
    host = lambda t: t.index_select(0, rows).cpu().numpy()
    fh, gh, fqh, fph, hh = host(f), host(g), host(fq).view(np.uint16), host(fp), host(h).view(np.uint16)
    assert not orc.verify_keys_batch(N, q, 3, fh, gh, fqh, fph, hh)["flags"].any()
    assert np.array_equal(orc.public_key_batch(N, q, 3, fqh, gh), hh)
    for t in (f, g):
        assert bool(((t == 1).sum(1) == (df if t is f else dg)).all())


def test_agrees_with_the_composed_chain(eng, torch_dev):
    """Without non-units the call is sample -> invert_key_batch_dev -> public_key_batch_dev, and bench.generate_key_pairs."""
    import bench
    torch, dev = torch_dev
    o = options("n821_q4096")
    N, q, df, dg = o["N"], o["q"], o["df"], o["dg"]
    B, first = 3000, 77
    key = (np.arange(8, dtype=np.uint32) * 0x85EBCA6B + 7).astype(np.uint32)     # bench.generate_key_pairs's key
    out = eng.keygen_batch(N, q, 3, df, dg, key, B, first_item=first)
    assert (out["tries"] == 1).all() and not out["flags"].any()
    fs = torch.empty((B, N), dtype=torch.uint8, device=dev)
    gs = torch.empty((B, N), dtype=torch.uint8, device=dev)
    eng.sample_ternary_dev(N, df, df - 1, 255, key, first, B, fs.data_ptr())
    eng.sample_ternary_dev(N, dg, dg, 255, key, (1 << 40) + first, B, gs.data_ptr())
    fq = torch.empty((B, N), dtype=torch.int16, device=dev); fp = torch.empty((B, N), dtype=torch.uint8, device=dev)
    fl = torch.empty(B, dtype=torch.uint8, device=dev); h = torch.empty((B, N), dtype=torch.int16, device=dev)
    eng.invert_key_batch_dev(N, q, 3, fs.data_ptr(), B, fq.data_ptr(), fp.data_ptr(), fl.data_ptr())
    eng.public_key_batch_dev(N, q, 3, fq.data_ptr(), gs.data_ptr(), B, h.data_ptr())
    torch.cuda.synchronize()
    assert np.array_equal(out["f"], fs.cpu().numpy().view(np.int8))
    assert np.array_equal(out["g"], gs.cpu().numpy().view(np.int8))
    assert np.array_equal(out["fq"], fq.cpu().numpy().view(np.uint16))
    assert np.array_equal(out["fp"], fp.cpu().numpy())
    assert np.array_equal(out["h"], h.cpu().numpy().view(np.uint16))
    bf, bg, bfq, bfp, bh, info = bench.generate_key_pairs(torch, eng, dev, o, B, first)
    assert info["non_units_redrawn"] == 0
    assert np.array_equal(out["f"], bf.cpu().numpy())
    assert np.array_equal(out["fq"], bfq.cpu().numpy().view(np.uint16))
    assert np.array_equal(out["h"], bh.cpu().numpy().view(np.uint16))


@pytest.mark.parametrize("B", [0, 1, 77, 1000])
def test_independent_of_batch_and_form(eng, torch_dev, B):
    torch, dev = torch_dev
    N, q, df, dg = SMALL["n7"]
    X, k = 1000, min(B, 13)
    a = eng.keygen_batch(N, q, 3, df, dg, KEY, B, first_item=X)
    b = eng.keygen_batch(N, q, 3, df, dg, KEY, B - k, first_item=X + k)
    for name in a:
        assert np.array_equal(a[name][k:], b[name]), name
    # pinned outputs
    shapes = {n: (a[n].shape, a[n].dtype) for n in a}
    pinned = {n: eng.pinned_empty(s, dt) for n, (s, dt) in shapes.items()}
    c = eng.keygen_batch(N, q, 3, df, dg, KEY, B, first_item=X, out=pinned)
    for name in a:
        assert np.array_equal(a[name], c[name]), name
    if B == 0:
        return
    # the _dev form
    dd = {n: torch.empty(s, dtype={np.dtype(np.int8): torch.int8, np.dtype(np.uint8): torch.uint8,
                                   np.dtype(np.uint16): torch.int16}[np.dtype(dt)], device=dev) for n, (s, dt) in shapes.items()}
    work = torch.empty(eng.keygen_workspace_bytes(N, B), dtype=torch.uint8, device=dev)
    eng.keygen_batch_dev(N, q, 3, df, dg, KEY, X, 100, B, work.data_ptr(), *[dd[n].data_ptr() for n in ("f", "g", "fq", "fp", "h", "tries", "flags")])
    torch.cuda.synchronize()
    for name in a:
        got = dd[name].cpu().numpy()
        assert np.array_equal(a[name], got.view(a[name].dtype)), name


def test_optional_outputs_and_packed_h(eng):
    N, q, df, dg = SMALL["n17_q32"]
    B = 500
    a = eng.keygen_batch(N, q, 3, df, dg, KEY, B, first_item=9, packed_h=True)
    assert np.array_equal(a["packed_h"], orc.pack_batch(q - 1, N, a["h"]))
    b = eng.keygen_batch(N, q, 3, df, dg, KEY, B, first_item=9, want=("h",))
    assert set(b) == {"h", "flags"}
    assert np.array_equal(a["h"], b["h"]) and np.array_equal(a["flags"], b["flags"])


def test_sampler_rounds_do_not_apply(eng):
    N, q, df, dg = SMALL["n31"]
    a = eng.keygen_batch(N, q, 3, df, dg, KEY, 300, first_item=3)
    eng.set_sampler_rounds(8)
    try:
        b = eng.keygen_batch(N, q, 3, df, dg, KEY, 300, first_item=3)
        assert eng.sampler_rounds() == 8
    finally:
        eng.set_sampler_rounds(20)
    for name in a:
        assert np.array_equal(a[name], b[name]), name


@pytest.mark.parametrize("name", ["n17_q32", "n509_q2048"])
def test_python_shim(eng, name):
    ntru = pkg.ntru
    o = options(name)
    obj = ntru.NTRU(dict(o), engine=eng)
    keys = obj.generateKeysBatch(6, KEY, firstItem=40)
    for i in range(3):
        obj.loadKeyFromBatch(keys, i)
        orc_obj = orc.OracleNTRU(N=o["N"], p=o["p"], q=o["q"], df=o["df"], dg=o["dg"], dr=o["dr"], f=list(obj.f), fp=list(obj.fp),
                                 fq=list(obj.fq), g=list(obj.g), h=list(obj.h))
        assert obj.verifyKeysInputs() == orc_obj.verify_keys_inputs()
    rng = np.random.default_rng(1)
    m = [int(x) for x in rng.integers(0, 2, o["N"])]
    m[-1] = 1
    e = obj.encryptBits(m)["value"]
    assert obj.decryptBits(e)["value"] == m
    bad = dict(keys)
    bad["flags"] = keys["flags"].copy()
    bad["flags"][0] = 8
    with pytest.raises(ValueError, match="Could not find invertible f"):
        obj.loadKeyFromBatch(bad, 0)
