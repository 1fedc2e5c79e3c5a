"""The hand-offs of the lock-step decrypt kernel (k_decrypt_m8, kernel path 5): product 2 reads its batch operand from the 2-bit
packed image that product 1's epilogues write (no expansion phase, one barrier between the image's last write and its first read),
and the e stages are rewritten for the group's next row block while the partner group is anywhere in its own.  Every case compares
value, quotient1, remainder1 and quotient2 bit for bit with the CPU oracle on every row and with k_decrypt_m (kernel path 4).
Inputs are uniform e mod q."""
import threading

import numpy as np
import pytest

import __graft_entry__ as ge
import bench
from oracle import ntru_keygen as kg
from oracle import ntru_oracle as orc

pytestmark = pytest.mark.gpu
pkg = ge.load_package()
NAMES = ("value", "quotient1", "remainder1", "quotient2")


@pytest.fixture(scope="module")
def ctx():
    import torch
    eng = pkg.Engine(0)
    eng.set_stream(torch.cuda.current_stream().cuda_stream)
    yield torch, eng, torch.device("cuda:0")
    eng.set_kernel_path(0)


def _ternary(rng, N, n1, n2):
    out = np.zeros(N, np.int8)
    perm = rng.permutation(N)
    out[perm[:n1]] = 1
    out[perm[n1:n1 + n2]] = -1
    return out


_KEYS = {}


def _key(N, q):
    """(f, fp): the golden key of a shipped profile; N = 521 (17 column tiles: the smallest count that takes two rounds of strips;
    the golden set has nothing between 509 and 701): random ternary f with fp from the oracle's inversion; the LDS limits (no
    profile, x^N - 1 with N even): random ternary f and uniform fp, as tests/test_decrypt_lockstep_fit_gpu.py does."""
    if (N, q) not in _KEYS:
        rng = np.random.default_rng(N * 11 + q)
        if (N, q) in ((821, 4096), (701, 8192)):
            _, _, f, fp = bench.load_key("n%d_q%d" % (N, q))
        elif N == 521:
            while True:
                f = _ternary(rng, N, N // 3 + 1, N // 3)
                if kg.is_unit(f, N, 3):
                    break
            fp = np.asarray(kg.poly_inv(f.astype(np.int64), N, 3), np.int64) % 3
            fp = np.concatenate([fp, np.zeros(N - len(fp), np.int64)]).astype(np.uint8)
        else:
            f, fp = _ternary(rng, N, N // 3 + 1, N // 3), rng.integers(0, 3, N).astype(np.uint8)
        _KEYS[(N, q)] = (np.ascontiguousarray(f, np.int8), np.ascontiguousarray(fp, np.uint8))
    return _KEYS[(N, q)]


def _oracle(N, q, f, fp, e):
    """orc.decrypt_batch on every row, split over the host's cores (the C oracle releases the interpreter lock)."""
    B = e.shape[0]
    threads = max(1, min(16, len(__import__("os").sched_getaffinity(0)), (B + 255) // 256))
    cuts = np.linspace(0, B, threads + 1).astype(int)
    parts, errs = [None] * threads, []

    def work(i):
        try:
            parts[i] = orc.decrypt_batch(N, q, 3, f, fp, e[cuts[i]:cuts[i + 1]])
        except BaseException as exc:                         # a worker that dies must not read as a result
            errs.append(exc)

    ths = [threading.Thread(target=work, args=(i,)) for i in range(threads)]
    [t.start() for t in ths]; [t.join() for t in ths]
    assert not errs, errs[:1]
    return tuple(np.concatenate([p[k] for p in parts]) for k in range(4))


def _run(ctx, path, kernel, N, q, f, fp, e_np, ld=None):
    """One launch on device arrays at a row pitch of ld elements; returns the four outputs as dense host arrays.  The output arrays
    are filled with a pattern first, and with a pitch the pad elements must keep it."""
    torch, eng, dev = ctx
    B, ld = e_np.shape[0], ld or N
    e = torch.zeros((B, ld), dtype=torch.int16, device=dev)
    e[:, :N] = torch.from_numpy(e_np.view(np.int16)).to(dev)
    d_f, d_fp = torch.from_numpy(f).to(dev), torch.from_numpy(fp).to(dev)
    outs = [torch.full((B, ld), 0x5A, dtype=dt, device=dev) for dt in (torch.uint8, torch.int16, torch.int16, torch.uint8)]
    eng.set_kernel_path(path)
    eng.decrypt_batch_dev(N, q, 3, d_f.data_ptr(), d_fp.data_ptr(), e.data_ptr(), B, *[t.data_ptr() for t in outs],
                          **({"ld": ld} if ld != N else {}))
    torch.cuda.synchronize()
    assert eng.last_kernel() == kernel, (eng.last_kernel(), kernel, N, q, path)
    host = [t.cpu().numpy() for t in outs]
    for h_, name in zip(host, NAMES):
        assert (h_[:, N:] == 0x5A).all(), ("pad elements written", name)
    return tuple(np.ascontiguousarray(h_[:, :N]).view(np.uint16 if h_.dtype == np.int16 else np.uint8) for h_ in host)


def _check(ctx, N, q, B, ld=None, seed=0):
    f, fp = _key(N, q)
    rng = np.random.default_rng(N * 7 + q + B + seed)
    e = rng.integers(0, q, (B, N)).astype(np.uint16)
    e[0, :4] = (q - 1, 0, q // 2, q // 2 + 1)
    want = _oracle(N, q, f, fp, e)
    got8 = _run(ctx, 5, "k_decrypt_m8", N, q, f, fp, e, ld)
    got4 = _run(ctx, 4, "k_decrypt_m", N, q, f, fp, e, ld)
    for g8, g4, w, name in zip(got8, got4, want, NAMES):
        assert np.array_equal(g8, w), (N, q, B, ld, name, "k_decrypt_m8 against the oracle", np.argwhere(g8 != w)[:3].tolist())
        assert np.array_equal(g4, w), (N, q, B, ld, name, "k_decrypt_m against the oracle")
        assert np.array_equal(g8, g4), (N, q, B, ld, name, "k_decrypt_m8 against k_decrypt_m")
    return f, fp, e, got8


# B = 1: one group has a row block of one row, its partner none; 33: both groups, the second row block of one row; 32 * 5 + 7: an
# odd row-block count on a grid of three workgroups' worth -- one group walks empty phases while its partner works on real rows.
# N: 521 = two rounds of strips at their smallest (17 tiles); the shipped profiles; the LDS limits of the lock-step kernel
# (tests/test_decrypt_lockstep_fit_gpu.py: 864 at q = 4096 / 8192, 896 at q <= 2048).
@pytest.mark.parametrize("B", [1, 33, 32 * 5 + 7])
@pytest.mark.parametrize("N,q", [(521, 2048), (821, 4096), (701, 8192), (864, 8192), (896, 2048)])
def test_small_batches_every_row(ctx, N, q, B):
    _check(ctx, N, q, B)


def test_pitched_rows(ctx):
    """Row pitch = N rounded up to 64 elements: rows start at other alignments than the dense layout's, pads stay untouched."""
    _check(ctx, 821, 4096, 32 * 5 + 7, ld=832)
    _check(ctx, 521, 2048, 33, ld=576)


@pytest.mark.parametrize("N,q", [(821, 4096), (521, 2048)])
def test_many_trips_per_workgroup(ctx, N, q):
    """B = 32 (4 CUs + 1) + 5: every workgroup makes at least three trips (the grid is one workgroup of two row blocks per CU): the
    stages and the image of trip `it` are overwritten in trip `it + 1`, the last trip is partial and ends in a ragged row block.
    The launch is repeated and the two runs compared: a stage or image write racing a late operand read would differ between runs."""
    torch, eng, dev = ctx
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    B = 32 * (4 * cus + 1) + 5
    f, fp, e, first = _check(ctx, N, q, B)
    again = _run(ctx, 5, "k_decrypt_m8", N, q, f, fp, e)
    for a, b, name in zip(first, again, NAMES):
        assert np.array_equal(a, b), (N, q, B, name, "two runs of k_decrypt_m8 differ")
