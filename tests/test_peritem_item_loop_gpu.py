"""The seam that the six per-item matrix kernels share (k_verify_keys_m, k_polymul_m, k_product_tern_m, k_newton_round_m,
k_encrypt_pi_m, k_decrypt_pi_m): the persistent item loop, the operand rows requested one item ahead and their shift by the row
pointer's low four bits.  Every entry point runs on one item and on 3 * 65536 + 7 items (every wave walks at least three items, the
last trip is ragged), with every device array starting one element into its allocation, so that no row pointer is 16-byte aligned at
item 0.  Item b is item b % 61 of a pool of 61 items; the oracle runs on the pool only and every output bit of every item is compared
on the device against the pool's row."""
import numpy as np
import pytest

import __graft_entry__ as ge
from oracle import ntru_oracle as orc
from peritem_ref import oracle_decrypt, oracle_encrypt

pytestmark = pytest.mark.gpu
pkg = ge.load_package()

POOL = 61
BATCHES = [1, 3 * 65536 + 7]
SHAPES = [(64, 256, 4), (509, 8192, 0), (1024, 8192, 0)]       # (N, q, kernel path): one digit plane at two tiles; odd N; the largest
CALLS = ["verify_keys", "polymul_split", "public_key", "invert_key", "encrypt_peritem", "decrypt_peritem"]
FILL = 0x5A


@pytest.fixture(scope="module")
def eng():
    e = pkg.Engine(0)
    yield e
    e.set_kernel_path(0)


@pytest.fixture(scope="module")
def torch_dev():
    import torch
    return torch, torch.device("cuda:0")


_pools = {}


def pool(eng, N, q):
    """{call: (inputs, expected outputs)} for the 61 items of (N, q), made once.  The keys are true key material from the device's key
    generation, accepted only after the CPU oracle has confirmed f fq = 1 (mod q), f fp = 1 (mod 3) and h = p fq g: the inverses are
    unique, so these rows ARE the oracle's answer for invert_key and public_key."""
    if (N, q) in _pools:
        return _pools[(N, q)]
    rng = np.random.default_rng(N * 17 + q)
    eng.set_kernel_path(0)
    k = eng.keygen_batch(N, q, 3, N // 3, N // 3, np.array([0x9E3779B1 * (i + 11) & 0xFFFFFFFF for i in range(8)], np.uint32), POOL)
    good = np.nonzero(k["flags"] == 0)[0]
    assert good.size >= POOL // 2, (N, q, good.size)
    rows = good[np.arange(POOL) % good.size]
    f, g, fq, fp, h = (np.ascontiguousarray(k[n][rows]) for n in ("f", "g", "fq", "fp", "h"))
    one = np.zeros((POOL, N), np.int64); one[:, 0] = 1
    assert np.array_equal(orc.polymul_split_batch(N, q, (f.astype(np.int64) % q).astype(np.uint16), fq)[1], one)
    assert np.array_equal(orc.polymul_split_batch(N, 3, (f.astype(np.int64) % 3).astype(np.uint16), fp.astype(np.uint16))[1], one)
    assert np.array_equal(orc.public_key_batch(N, q, 3, fq, g), h)
    # verify_keys: the true keys, three of them spoilt (fq, fp, h) so that the flags differ between items
    vfq, vfp, vh = fq.copy(), fp.copy(), h.copy()
    vfq[1, 0] ^= 1; vfq[1, 1] ^= 1; vfp[2, 0] = (vfp[2, 0] + 1) % 3; vfp[2, 2] = (vfp[2, 2] + 1) % 3; vh[3, 0] ^= 1
    v = orc.verify_keys_batch(N, q, 3, f, g, vfq, vfp, vh)
    assert v["flags"][0] == 0 and v["flags"][3] & 4
    a, b = rng.integers(0, q, (POOL, N), dtype=np.uint16), rng.integers(0, q, (POOL, N), dtype=np.uint16)
    r, m = rng.integers(0, 3, (POOL, N), dtype=np.uint8), rng.integers(0, 256, (POOL, N), dtype=np.uint8)
    e = rng.integers(0, q, (POOL, N), dtype=np.uint16)
    p = {
        "verify_keys": ((f, g, vfq, vfp, vh), tuple(v[n] for n in ("quot_fq", "rem_fq", "quot_fp", "rem_fp", "quot_h", "rem_h", "flags"))),
        "polymul_split": ((a, b), tuple(x.astype(np.uint16) for x in orc.polymul_split_batch(N, q, a, b))),
        "public_key": ((fq, g), (h,)),
        "invert_key": ((f,), (fq, fp, np.zeros(POOL, np.uint8))),
        "encrypt_peritem": ((h, r, m), oracle_encrypt(N, q, h, r, m)),
        "decrypt_peritem": ((f, fp, e), oracle_decrypt(N, q, 3, f, fp, e)),
    }
    _pools[(N, q)] = p
    return p


def launch(eng, call, N, q, B, ins, outs):
    if call == "verify_keys":
        eng.verify_keys_batch_dev(N, q, 3, *ins, B, *outs)
        return "k_verify_keys_m"
    if call == "polymul_split":
        eng.polymul_split_dev(N, q, *ins, B, *outs)
        return "k_polymul_m"
    if call == "public_key":
        eng.public_key_batch_dev(N, q, 3, *ins, B, *outs)
        return "k_public_key_m"
    if call == "invert_key":
        eng.invert_key_batch_dev(N, q, 3, *ins, B, *outs)
        return "k_invert_key"
    if call == "encrypt_peritem":
        eng.encrypt_peritem_batch_dev(N, q, *ins, B, *outs)
        return "k_encrypt_pi_m"
    eng.decrypt_peritem_batch_dev(N, q, 3, *ins, B, *outs)
    return "k_decrypt_pi_m"


@pytest.mark.parametrize("B", BATCHES)
@pytest.mark.parametrize("N,q,path", SHAPES)
@pytest.mark.parametrize("call", CALLS)
def test_item_loop_on_misaligned_rows(eng, torch_dev, call, N, q, path, B):
    torch, dev = torch_dev
    ins_np, want_np = pool(eng, N, q)[call]
    idx = torch.arange(B, device=dev) % POOL
    signed = lambda a: a.view(np.int16) if a.dtype == np.uint16 else a
    on_dev = lambda a: torch.from_numpy(np.ascontiguousarray(signed(a))).to(dev)
    keep, ins, outs = [], [], []
    for a in ins_np:                                           # rows of the pool, starting one element into the allocation
        t = on_dev(a)
        buf = torch.full((1 + B * N,), FILL, dtype=t.dtype, device=dev)
        buf[1:].view(B, N).copy_(t[idx])
        keep.append(buf); ins.append(buf.data_ptr() + buf.element_size())
    for w in want_np:                                          # outputs likewise, one guard element on either side
        t = on_dev(w)
        n = B * (N if w.ndim == 2 else 1)
        buf = torch.full((n + 2,), FILL, dtype=t.dtype, device=dev)
        outs.append((buf, t, n)); keep.append(buf)
    eng.set_kernel_path(path)
    try:
        kernel = launch(eng, call, N, q, B, ins, [buf.data_ptr() + buf.element_size() for buf, _, _ in outs])
        assert eng.last_kernel() == kernel, eng.last_kernel()
        if call == "invert_key":       # (names no inner kernel: its Newton rounds take k_newton_round_m by the rule this product follows)
            z = torch.zeros((3, N), dtype=torch.int16, device=dev)
            eng.polymul_split_dev(N, q, z[0].data_ptr(), z[0].data_ptr(), 1, z[1].data_ptr(), z[2].data_ptr())
            assert eng.last_kernel() == "k_polymul_m", eng.last_kernel()
        torch.cuda.synchronize()
    finally:
        eng.set_kernel_path(0)
    for i, (buf, t, n) in enumerate(outs):
        assert buf[0].item() == FILL and buf[n + 1].item() == FILL, (call, i, "wrote outside its rows")
        got = buf[1:n + 1].view(B, N) if t.ndim == 2 else buf[1:n + 1]
        same = got == t[idx]
        if not bool(same.all()):
            bad = torch.nonzero(~(same.all(dim=1) if t.ndim == 2 else same)).flatten()
            raise AssertionError((call, N, q, B, "output %d" % i, "items", bad[:8].tolist(), "of", int(bad.numel())))
