"""The regular host-pointer forms and the ntru_multi_* forms of the C ABI, all through one description each (tests/host_forms.py).

Error parity: the return code and the ntru_last_error() text of every bad-argument case equal tests/golden/host_form_errors.json,
recorded by tests/golden/record_host_form_errors.py from the commit before the forms were derived from one description each.
Data parity: a host form's outputs equal, byte for byte, what its own _dev form writes for the same inputs held in device buffers:
B = 1 and B = 8197 (four chunks of 2050, the last one ragged), pageable and pinned arrays, optional outputs asked for and not.

The host forms that keep results on the device for a whole call (sum_groups, combine_batch, draw_permutation: the engine's resident
buffer, one holder at a time) one after the other on one engine, each against numpy."""
import ctypes as C

import numpy as np
import pytest

import __graft_entry__ as ge
import host_forms as hf
from conftest import load_golden

pkg = ge.load_package()
pytestmark = pytest.mark.gpu
BATCHES = (1, 8197)
FILL = 0xA5


@pytest.fixture(scope="module")
def eng():
    return pkg.Engine(0)


@pytest.fixture(scope="module")
def multi():
    return pkg.MultiEngine([0, 0, 0])        # three engines whatever the number of devices: unequal shards, B = 1 leaves two empty


@pytest.fixture(scope="module")
def recorded():
    return load_golden("host_form_errors.json")


@pytest.mark.parametrize("f", hf.FORMS + hf.MULTI_FORMS, ids=lambda f: f.name)
def test_error_parity(eng, multi, recorded, f):
    h = multi if f.name.startswith("ntru_multi_") else eng
    got = hf.run_error_cases(h._lib, f, h._h)
    want = recorded[f.name]
    assert sorted(got) == sorted(want), "the case list and the recorded table differ"
    assert got == want, {k: (got[k], want[k]) for k in got if got[k] != want[k]}
    assert got["B_0_all_NULL"][0] == 0


class HostArrays:
    """Host arrays of one call, pageable (numpy's own) or pinned (ntru_host_alloc), released together."""

    def __init__(self, lib, pinned):
        self.lib, self.pinned, self.held = lib, pinned, []

    def empty(self, count, dt):
        nbytes = max(1, count * np.dtype(dt).itemsize)
        if not self.pinned:
            return np.empty(nbytes, np.uint8).view(dt)[:count]
        p = self.lib.ntru_host_alloc(nbytes)
        assert p, "ntru_host_alloc failed"
        self.held.append(p)
        return np.ctypeslib.as_array((C.c_uint8 * nbytes).from_address(p)).view(dt)[:count]

    def copy(self, a):
        b = self.empty(a.size, a.dtype)
        b[:] = a
        return b

    def filled(self, count, dt):
        b = self.empty(count, dt)
        b.view(np.uint8)[:] = FILL
        return b

    def close(self):
        for p in self.held:
            self.lib.ntru_host_free(p)
        self.held = []


def make_inputs(f, count):
    rng = np.random.default_rng(len(f.name) * 1000 + count)
    once = ("key", "hostkey")                # one row per call, not per item
    return {a.name: rng.integers(a.lo, a.hi, hf.row_len(f, a) * (1 if a.role in once else count),
                                 dtype=np.int64 if a.lo < 0 else np.uint64).astype(a.dt)
            for a in hf.arrays(f) if a.role in once + ("in",)}


def outputs_of(f, wanted):
    return [a for a in hf.arrays(f) if a.role == "out" or (a.role == "opt" and a.name in wanted)]


def run_host(lib, symbol, handle, f, inputs, count, wanted, pinned):
    """The host form `symbol` on copies of the inputs; returns {output: bytes}."""
    mem = HostArrays(lib, pinned)
    try:
        bufs = {name: mem.copy(a) for name, a in inputs.items()}
        bufs.update({a.name: mem.filled(hf.row_len(f, a) * count, a.dt) for a in outputs_of(f, wanted)})
        rc = hf.invoke(lib, symbol, handle, f, f.vals, {name: b.ctypes.data for name, b in bufs.items()}, count)
        assert rc == 0, (symbol, count, wanted, pinned, lib.ntru_last_error().decode())
        return {a.name: bufs[a.name].tobytes() for a in outputs_of(f, wanted)}
    finally:
        mem.close()


def run_dev(eng, f, inputs, count, wanted):
    """The _dev form of f on device buffers holding the same inputs; returns {output: bytes}."""
    lib, h, dev = eng._lib, eng._h, {}

    def alloc(name, host):
        p = C.c_void_p()
        assert lib.ntru_dev_alloc(h, host.nbytes, C.byref(p)) == 0
        dev[name] = p.value
        assert lib.ntru_dev_upload(h, C.c_void_p(p.value), C.c_void_p(host.ctypes.data), host.nbytes) == 0

    try:
        ptrs, outs = {}, {}
        for a in hf.arrays(f):
            if a.role == "hostkey":
                ptrs[a.name] = inputs[a.name].ctypes.data
            elif a.name in inputs:
                alloc(a.name, inputs[a.name])
        for a in outputs_of(f, wanted):
            outs[a.name] = np.full(hf.row_len(f, a) * count * np.dtype(a.dt).itemsize, FILL, np.uint8)
            alloc(a.name, outs[a.name])
        ptrs.update(dev)
        rc = hf.invoke(lib, f.name + "_dev", h, f, f.vals, ptrs, count)
        assert rc == 0, (f.name, count, wanted, lib.ntru_last_error().decode())
        for name, o in outs.items():
            assert lib.ntru_dev_download(h, C.c_void_p(o.ctypes.data), C.c_void_p(dev[name]), o.nbytes) == 0
        return {name: o.tobytes() for name, o in outs.items()}
    finally:
        for p in dev.values():
            lib.ntru_dev_free(h, C.c_void_p(p))


@pytest.mark.parametrize("f", hf.FORMS, ids=lambda f: f.name)
def test_host_form_equals_dev_form(eng, f):
    for count in BATCHES:
        inputs = make_inputs(f, count)
        for wanted in f.opt_sets:
            want = run_dev(eng, f, inputs, count, wanted)
            assert want and all(len(v) for v in want.values())
            if count > 1:                    # (a single byte may equal the fill by right)
                assert all(v.strip(bytes([FILL])) for v in want.values()), "an output the _dev form did not write"
            for pinned in (False, True):
                got = run_host(eng._lib, f.name, eng._h, f, inputs, count, wanted, pinned)
                diff = [k for k in want if got[k] != want[k]]
                assert not diff, (f.name, count, wanted, pinned, diff)


@pytest.mark.parametrize("f", hf.MULTI_FORMS, ids=lambda f: f.name)
def test_multi_form_equals_host_form(eng, multi, f):
    single = f.name.replace("ntru_multi_", "ntru_")
    for count in BATCHES:
        inputs = make_inputs(f, count)
        for wanted in f.opt_sets:
            want = run_host(eng._lib, single, eng._h, f, inputs, count, wanted, False)
            got = run_host(multi._lib, f.name, multi._h, f, inputs, count, wanted, False)
            diff = [k for k in want if got[k] != want[k]]
            assert not diff, (f.name, count, wanted, diff)


def test_resident_buffer_passes_from_one_host_form_to_the_next():
    """sum_groups (offsets with an empty group), combine_batch, draw_permutation, then sums of four times the groups and the
    combination again, on ONE engine: every holder of the resident buffer takes it after every other kind and computes what numpy
    does.  The buffer grows in steps of 1 MiB, which none of these sizes crosses, so a draw of 200000 items (3.2 MB) follows and the sums
    and the combination run once more behind that regrow."""
    N, mod, rows_n = 17, 4096, 40
    rng = np.random.default_rng(20)
    rows = rng.integers(0, mod, (rows_n, N), dtype=np.uint16)
    w = rng.integers(0, mod, (rows_n, 3), dtype=np.uint16)
    key = np.arange(1, 9, dtype=np.uint32)
    wide = rows.astype(np.int64)
    want_combo = ((w.T.astype(np.int64) @ wide) % mod).astype(np.uint16)

    def sums(offsets):
        return np.stack([wide[a:b].sum(axis=0) % mod for a, b in zip(offsets[:-1], offsets[1:])]).astype(np.uint16)

    def check_draw(B):
        src = pkg.draw_permutation(eng, key, 7, B)
        assert np.array_equal(np.sort(src), np.arange(B)), "not a permutation of range(B)"
        assert np.array_equal(pkg.draw_permutation(eng, key, 7, B), src), "a second draw under the same key and id differs"

    few = np.array([0, 7, 7, 19, 40], np.int64)                                  # group 1 is empty
    many = np.array([0, 2, 5, 5, 7, 10, 12, 15, 19, 20, 24, 27, 30, 33, 36, 38, 40], np.int64)   # 16 groups, group 2 is empty
    eng = pkg.Engine(0)
    assert np.array_equal(eng.sum_groups(N, mod, rows, offsets=few), sums(few))
    assert np.array_equal(pkg.combine_batch(eng, N, mod, rows, w), want_combo)
    check_draw(1000)
    assert np.array_equal(eng.sum_groups(N, mod, rows, offsets=many), sums(many))
    assert np.array_equal(pkg.combine_batch(eng, N, mod, rows, w), want_combo)
    check_draw(200000)
    assert np.array_equal(eng.sum_groups(N, mod, rows, offsets=few), sums(few))
    assert np.array_equal(pkg.combine_batch(eng, N, mod, rows, w), want_combo)
