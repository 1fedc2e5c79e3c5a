"""The ctypes binding (ntru-circom_amd/engine.py) against the header it binds, without a GPU and without the library:
(a) every prototype of include/ntru_engine.h has its _SIGS entry with the same arity and argument classes, and _SIGS has nothing else;
(b) the public methods of Engine and MultiEngine keep their signatures;
(c) every regular batch call, in its host, _dev and MultiEngine forms, hands the library what the header asks for: driven against a
    stub that records its arguments and reads the memory behind the host pointers while the call is in flight."""
import ctypes as C
import inspect
import json
import os
import re

import numpy as np
import pytest

import __graft_entry__ as ge

pkg = ge.load_package()
engine = pkg.engine
ROOT = ge.ROOT


# ---- (a) the header -------------------------------------------------------------------------------------------------------------
def prototypes():
    """{name: (return type, [(type, name) per parameter])} of every function the header declares; a pointer type is spelled '*'."""
    text = open(os.path.join(ROOT, "include", "ntru_engine.h")).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    text = re.sub(r"^\s*#.*$", "", text, flags=re.M).replace('extern "C" {', "")

    def kind(decl):
        decl = decl.strip()
        if "*" in decl:
            return "*", decl.rsplit("*", 1)[1].strip()
        words = [w for w in decl.split() if w != "const"]
        return " ".join(words[:-1]), words[-1]
    protos = {}
    for chunk in text.split(";"):
        m = re.match(r"^\s*([\w\s\*]+?)\s*\b(ntru_\w+)\s*\((.*)\)\s*$", chunk, flags=re.S)
        if m:
            ret, name, args = m.group(1).strip(), m.group(2), m.group(3).strip()
            protos[name] = ("*" if "*" in ret else ret, [] if args == "void" else [kind(a) for a in args.split(",")])
    return protos


PROTOS = prototypes()
CLASSES = {"int": C.c_int, "int64_t": C.c_int64, "uint64_t": C.c_uint64, "size_t": C.c_size_t, "void": None}


def class_matches(header_type, ctype):
    if header_type == "*":
        return ctype in (C.c_void_p, C.c_char_p) or (isinstance(ctype, type) and issubclass(ctype, C._Pointer))
    return ctype is CLASSES[header_type]


def test_header_parse_finds_the_prototypes():
    assert len(PROTOS) >= 86
    assert PROTOS["ntru_engine_device_count"] == ("int", [])
    assert PROTOS["ntru_host_alloc"] == ("*", [("size_t", "bytes")])
    assert PROTOS["ntru_sample_ternary"][1][6] == ("uint64_t", "first_item")


def test_sigs_match_the_header():
    assert sorted(engine._SIGS) == sorted(PROTOS)
    for name, (ret, params) in PROTOS.items():
        res, args = engine._SIGS[name]
        assert class_matches(ret, res), (name, "return", ret, res)
        assert len(args) == len(params), (name, len(args), len(params))
        for k, ((htype, pname), ctype) in enumerate(zip(params, args)):
            assert class_matches(htype, ctype), (name, k, pname, htype, ctype)


# ---- (b) the public surface, as recorded before the batch calls were derived from a table ------------------------------------------
def public_surface(cls):
    return {n: str(inspect.signature(f)) for n, f in inspect.getmembers(cls, inspect.isfunction) if not n.startswith("_")}


ENGINE_SURFACE = json.loads(r"""
{
 "add_batch": "(self, N, mod, a, b)",
 "add_batch_dev": "(self, N, mod, d_a, d_b, B, d_out)",
 "bytes_to_rows": "(self, N, nbytes, data)",
 "bytes_to_rows_dev": "(self, N, nbytes, d_bytes, B, d_m)",
 "check_decrypt_batch": "(self, N, q, nq, p, np_, f, fp, e, quot1, rem1, quot2, rem2)",
 "check_decrypt_batch_dev": "(self, N, q, nq, p, np_, d_f, d_fp, d_e, d_quot1, d_rem1, d_quot2, d_rem2, B, d_flags)",
 "check_encrypt_batch": "(self, N, q, nq, r, m, h, quotE, remE)",
 "check_encrypt_batch_dev": "(self, N, q, nq, d_r, d_m, d_h, d_quotE, d_remE, B, d_flags)",
 "check_inverse_batch": "(self, N, M, n, f, fq, quotI, remI)",
 "check_inverse_batch_dev": "(self, N, M, n, d_f, d_fq, d_quotI, d_remI, B, d_flags)",
 "close": "(self)",
 "decrypt_batch": "(self, N, q, p, f, fp, e, want_witness=True)",
 "decrypt_batch_dev": "(self, N, q, p, d_f, d_fp, d_e, B, d_value, d_quot1=None, d_rem1=None, d_quot2=None, ld=None)",
 "decrypt_bytes_batch": "(self, N, q, p, nbytes, f, fp, e, want_flags=True)",
 "decrypt_bytes_batch_dev": "(self, N, q, p, nbytes, d_f, d_fp, d_e, B, d_bytes, d_flags=None)",
 "decrypt_pack_batch_dev": "(self, N, q, p, d_f, d_fp, d_e, B, d_value, d_packed)",
 "decrypt_peritem_batch": "(self, N, q, p, f, fp, e, want_witness=True)",
 "decrypt_peritem_batch_dev": "(self, N, q, p, d_f, d_fp, d_e, B, d_value, d_quot1=None, d_rem1=None, d_quot2=None)",
 "dev_alloc": "(self, nbytes)",
 "dev_download": "(self, d_ptr, shape, dtype)",
 "dev_free": "(self, d_ptr)",
 "dev_upload": "(self, d_ptr, host)",
 "encrypt_batch": "(self, N, q, h, r, m, want_quot=True)",
 "encrypt_batch_dev": "(self, N, q, d_h, d_r, d_m, B, d_e, d_quotE=None, ld=None)",
 "encrypt_bytes_batch": "(self, N, q, nbytes, h, r, data, want_quot=True)",
 "encrypt_bytes_batch_dev": "(self, N, q, nbytes, d_h, d_r, d_bytes, B, d_e, d_quotE=None)",
 "encrypt_pack_batch_dev": "(self, N, q, d_h, d_r, d_m, B, d_e, d_packed)",
 "encrypt_peritem_batch": "(self, N, q, h, r, m, want_quot=True)",
 "encrypt_peritem_batch_dev": "(self, N, q, d_h, d_r, d_m, B, d_e, d_quotE=None)",
 "generic_divide": "(self, a, b, mod)",
 "generic_eea": "(self, a, b, mod)",
 "generic_multiply": "(self, a, b, mod)",
 "generic_poly_inv": "(self, a, poly_i, mod)",
 "invert_key_batch": "(self, N, q, p, f, want_fq=True, want_fp=True)",
 "invert_key_batch_dev": "(self, N, q, p, d_f, B, d_fq, d_fp, d_flags)",
 "keygen_batch": "(self, N, q, p, df, dg, key, B, first_item=0, max_tries=100, want=('f', 'g', 'fq', 'fp', 'h', 'tries'), packed_h=False, out=None)",
 "keygen_batch_dev": "(self, N, q, p, df, dg, key, first_item, max_tries, B, d_work, d_f, d_g, d_fq, d_fp, d_h, d_tries, d_flags)",
 "keygen_workspace_bytes": "(self, N, B)",
 "last_kernel": "(self)",
 "pack_batch": "(self, max_val, data_len, data)",
 "pack_bytes_batch_dev": "(self, max_val, data_len, d_data, B, d_out)",
 "pack_params": "(self, max_val, data_len)",
 "pinned_empty": "(self, shape, dtype)",
 "pipeline_batch": "(self, N, q, p, h, m, f=None, fp=None, key=None, first_item=0, n1=0, n2=0, r=None, want_r=False, want_e=False, want_value=False, want_packed=False)",
 "pipeline_bytes_batch": "(self, N, q, p, nbytes, h, msg, f=None, fp=None, key=None, first_item=0, n1=0, n2=0, r=None, want_r=False, want_e=False, want_msg=False, want_flags=False, out=None)",
 "polymul_split": "(self, N, mod, a, b)",
 "polymul_split_dev": "(self, N, mod, d_a, d_b, B, d_quot, d_rem)",
 "public_key_batch": "(self, N, q, p, fq, g)",
 "public_key_batch_dev": "(self, N, q, p, d_fq, d_g, B, d_h)",
 "rows_to_bytes": "(self, N, nbytes, value, want_flags=True)",
 "rows_to_bytes_dev": "(self, N, nbytes, d_value, B, d_bytes, d_flags=None)",
 "sample_ternary": "(self, N, n1, n2, other, key, first_item, B)",
 "sample_ternary_dev": "(self, N, n1, n2, other, key, first_item, B, d_out)",
 "sampler_rounds": "(self)",
 "set_kernel_path": "(self, path)",
 "set_sampler_rounds": "(self, rounds)",
 "set_stream": "(self, hip_stream)",
 "split_by_I": "(self, N, mod, a)",
 "split_by_I_dev": "(self, N, mod, d_a, B, d_quot, d_rem)",
 "sum_groups": "(self, N, mod, rows, offsets=None, K=None, weights=None)",
 "sum_groups_dev": "(self, N, mod, d_rows, d_out, G, d_offsets=None, K=None, d_weights=None)",
 "supports": "(self, N, mod)",
 "synchronize": "(self)",
 "tally_decrypt_batch": "(self, N, q, p, f, fp, rows, offsets=None, K=None, weights=None, want_witness=True)",
 "tally_decrypt_batch_dev": "(self, N, q, p, d_f, d_fp, d_rows, d_sum, d_value, G, d_offsets=None, K=None, d_weights=None, d_quot1=None, d_rem1=None, d_quot2=None)",
 "unpack_batch": "(self, max_val, packed_bits, limbs)",
 "verify_keys_batch": "(self, N, q, p, f, g, fq, fp, h)",
 "verify_keys_batch_dev": "(self, N, q, p, d_f, d_g, d_fq, d_fp, d_h, B, d_quot_fq, d_rem_fq, d_quot_fp, d_rem_fp, d_quot_h, d_rem_h, d_flags)"
}
""")
MULTI_SURFACE = json.loads(r"""
{
 "close": "(self)",
 "decrypt_batch": "(self, N, q, p, f, fp, e, want_witness=True)",
 "encrypt_batch": "(self, N, q, h, r, m, want_quot=True)",
 "engines": "(self)",
 "invert_key_batch": "(self, N, q, p, f)",
 "polymul_split": "(self, N, mod, a, b)",
 "public_key_batch": "(self, N, q, p, fq, g)",
 "verify_keys_batch": "(self, N, q, p, f, g, fq, fp, h)"
}
""")


def test_public_surface_is_frozen():
    assert public_surface(pkg.Engine) == ENGINE_SURFACE
    assert public_surface(pkg.MultiEngine) == MULTI_SURFACE


# ---- (c) the regular batch calls against a recording stub ---------------------------------------------------------------------------
class StubLibrary:
    """Stands in for the loaded library: every symbol records (name, arguments) and returns 0.  A host pointer is recorded as
    (address, the `peek[k]` bytes behind it at the time of the call) where the test has said how many bytes argument k must hold."""

    def __init__(self):
        self.calls, self.peek = [], {}

    def __getattr__(self, name):
        def fn(*args):
            seen = []
            for k, a in enumerate(args):
                if isinstance(a, C.c_void_p):
                    size = self.peek.get(k)
                    a = (a.value, C.string_at(a.value, size) if size is not None and a.value else None)
                seen.append(a)
            self.calls.append((name, seen))
            if name == "ntru_engine_last_kernel":
                return b"k_stub"
            if name in ("ntru_engine_create", "ntru_multi_create"):
                args[-1]._obj.value = 0x5150
            if name == "ntru_pack_params":
                for ref, v in zip(args[2:], (2, 126, 378, 3)):
                    ref._obj.value = v
            return 0
        return fn


@pytest.fixture()
def stub(monkeypatch):
    lib = StubLibrary()
    monkeypatch.setattr(engine, "_LIB", lib)
    return lib


B = 3
SCALARS = {"N": 5, "q": 64, "p": 3, "mod": 8, "nq": 7, "np": 2, "M": 16, "n": 4, "nbytes": 0, "ld": 7}
N = SCALARS["N"]
KEY = "key"          # a shared input of shape (N,)
# per call: the row length of every array parameter of the header's prototype, by the header's name without d_ (None: [B]);
# the dtypes come from the header.  `forms`: which of the host / _dev / MultiEngine methods exist.
NB = "nbytes"
CASES = {
    "polymul_split": (dict(a=N, b=N, quot=N, rem=N), "host dev multi"),
    "split_by_I": (dict(a=2 * N, quot=N, rem=N), "host dev"),
    "add_batch": (dict(a=N, b=N, out=N), "host dev"),
    "encrypt_batch": (dict(h=KEY, r=N, m=N, e=N, quotE=N), "host dev multi"),
    "decrypt_batch": (dict(f=KEY, fp=KEY, e=N, value=N, quot1=N, rem1=N, quot2=N), "host dev multi"),
    "bytes_to_rows": (dict(bytes=NB, m=N), "host dev"),
    "rows_to_bytes": (dict(value=N, bytes=NB, flags=None), "host dev"),
    "encrypt_bytes_batch": (dict(h=KEY, r=N, bytes=NB, e=N, quotE=N), "host dev"),
    "decrypt_bytes_batch": (dict(f=KEY, fp=KEY, e=N, bytes=NB, flags=None), "host dev"),
    "encrypt_peritem_batch": (dict(h=N, r=N, m=N, e=N, quotE=N), "host dev"),
    "decrypt_peritem_batch": (dict(f=N, fp=N, e=N, value=N, quot1=N, rem1=N, quot2=N), "host dev"),
    "verify_keys_batch": (dict(f=N, g=N, fq=N, fp=N, h=N, quot_fq=N, rem_fq=N, quot_fp=N, rem_fp=N, quot_h=N, rem_h=N, flags=None),
                          "host dev multi"),
    "public_key_batch": (dict(fq=N, g=N, h=N), "host dev multi"),
    "invert_key_batch": (dict(f=N, fq=N, fp=N, flags=None), "host dev multi"),
    "check_encrypt_batch": (dict(r=N, m=N, h=N, quotE=N + 1, remE=N + 1, flags=None), "host dev"),
    "check_decrypt_batch": (dict(f=N, fp=N, e=N, quot1=N + 1, rem1=N + 1, quot2=N + 1, rem2=N + 1, flags=None), "host dev"),
    "check_inverse_batch": (dict(f=N, fq=N, quotI=N + 1, remI=N + 1, flags=None), "host dev"),
    "decrypt_pack_batch": (dict(f=KEY, fp=KEY, e=N, value=N, packed=12), "dev"),
    "encrypt_pack_batch": (dict(h=KEY, r=N, m=N, e=N, packed=12), "dev"),
}
# the keyword of the host method that gates an optional output, and the outputs it gates
WANTS = {"want_quot": ["quotE"], "want_witness": ["quot1", "rem1", "quot2"], "want_flags": ["flags"], "want_fq": ["fq"], "want_fp": ["fp"]}
DTYPES = {"uint8_t": np.uint8, "int8_t": np.int8, "uint16_t": np.uint16, "uint64_t": np.uint64}


def header_arrays(symbol):
    """[(position, name without d_ and with the header's mm as m, dtype, is an input)] of the prototype's typed pointers after the
    engine."""
    text = open(os.path.join(ROOT, "include", "ntru_engine.h")).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    args = re.search(r"\b%s\s*\((.*?)\)\s*;" % symbol, text, flags=re.S).group(1).split(",")
    out = []
    for k, a in enumerate(args[1:], 1):
        m = re.match(r"\s*(const\s+)?(\w+)\s*\*\s*(?:d_)?(\w+)\s*$", a)
        if m:
            out.append((k, "m" if m.group(3) == "mm" else m.group(3), DTYPES[m.group(2)], bool(m.group(1))))
    return out


def row_length(rows, name, nbytes):
    n = rows[name]
    return nbytes if n == NB else N if n == KEY else n


def check_scalars(symbol, seen, scalars):
    """Arity, the engine handle, every int parameter and the batch count sit where the header puts them."""
    params = PROTOS[symbol][1]
    assert len(seen) == len(params), (symbol, len(seen), len(params))
    assert seen[0] == (0x5150, None)
    for k, (htype, pname) in enumerate(params):
        if htype == "int":
            assert seen[k] == scalars[pname], (symbol, pname, k, seen[k])
        elif htype == "int64_t":
            assert pname == "B" and seen[k] == B, (symbol, pname, k, seen[k])


def make_input(kind, dtype, shape):
    """An input with distinct values: 0 as the binding wants it, 1 of the wrong dtype, 2 a strided view of a wider array."""
    size = int(np.prod(shape))
    vals = (np.arange(size) % 3).reshape(shape)
    if kind == 0:
        return vals.astype(dtype)
    if kind == 1:
        return vals.astype(np.int64)
    wide = np.zeros(shape[:-1] + (2 * shape[-1],), dtype)
    wide[..., ::2] = vals
    return wide[..., ::2]


def drive_host(stub, obj, name, prefix, nbytes, wants):
    """Call the host method `name` of obj and check what reached <prefix><name>; returns what the method returned."""
    rows, _ = CASES[name]
    symbol = prefix + name
    arrays = header_arrays(symbol)
    method = getattr(obj, name)
    scalars = dict(SCALARS, nbytes=nbytes)
    kwargs, inputs = {}, {}
    for kind, pname in enumerate(p for p in inspect.signature(method).parameters):
        cname = {"np_": "np", "data": "bytes"}.get(pname, pname)
        if cname in scalars:
            kwargs[pname] = scalars[cname]
        elif pname.startswith("want_"):
            kwargs[pname] = wants
        else:
            shape = (N,) if rows[cname] == KEY else (B, row_length(rows, cname, nbytes))
            dtype = [dt for _, n, dt, is_in in arrays if n == cname and is_in][0]
            inputs[cname] = kwargs[pname] = make_input(kind % 3, dtype, shape)
    stub.peek = {k: (N if rows[n] == KEY else B if rows[n] is None else B * row_length(rows, n, nbytes)) * np.dtype(dt).itemsize
                 for k, n, dt, _ in arrays}
    del stub.calls[:]
    result = method(**kwargs)
    (called, seen), = stub.calls
    assert called == symbol
    check_scalars(symbol, seen, scalars)
    gated = [] if wants else [o for w in inspect.signature(method).parameters if w in WANTS for o in WANTS[w]]
    returned = list(result.values()) if isinstance(result, dict) else list(result) if isinstance(result, tuple) else [result]
    outputs = [(k, n, dt) for k, n, dt, is_in in arrays if not is_in]
    assert len(returned) == len(outputs), (symbol, len(returned))
    if isinstance(result, dict):
        assert list(result) == [n for _, n, _ in outputs]
    for k, n, dt, is_in in arrays:
        if is_in:
            want = np.ascontiguousarray(np.asarray(inputs[n], dtype=dt))
            assert seen[k][1] == want.tobytes(), (symbol, n, "the pointer does not lead to the contiguous %s rows" % np.dtype(dt).name)
            x = inputs[n]
            if x.dtype == dt and x.flags.c_contiguous and x.size:
                assert seen[k][0] == x.ctypes.data, (symbol, n, "an input that needs no conversion was copied")
    for (k, n, dt), arr in zip(outputs, returned):
        if n in gated:
            assert seen[k] is None and arr is None, (symbol, n)
            continue
        shape = (B,) if rows[n] is None else (B, row_length(rows, n, nbytes))
        assert arr.dtype == dt and arr.shape == shape and arr.flags.c_contiguous, (symbol, n, arr.dtype, arr.shape)
        assert arr.nbytes == stub.peek[k] and seen[k][0] == arr.ctypes.data, (symbol, n)
    return result


def host_nbytes(name):
    # a block input of zero bytes per row cannot be shaped ([B][0] does not tell B): those two calls run at 2 bytes per block
    return 2 if name in ("bytes_to_rows", "encrypt_bytes_batch") else SCALARS["nbytes"]


@pytest.mark.parametrize("name", [n for n, (_, forms) in CASES.items() if "host" in forms])
def test_host_methods(stub, name):
    eng = pkg.Engine(0)
    for wants in (True, False):
        drive_host(stub, eng, name, "ntru_", host_nbytes(name), wants)


@pytest.mark.parametrize("name", [n for n, (_, forms) in CASES.items() if "multi" in forms])
def test_multi_engine_methods(stub, name):
    multi = pkg.MultiEngine([0, 0])
    assert stub.calls[0][0] == "ntru_multi_create" and list(stub.calls[0][1][0]) == [0, 0] and stub.calls[0][1][1] == 2
    for wants in (True, False):
        drive_host(stub, multi, name, "ntru_multi_", host_nbytes(name), wants)


def test_row_count_mismatches_are_refused(stub):
    eng = pkg.Engine(0)
    u8, u16 = (lambda n, w=N: np.zeros((n, w), np.uint8)), (lambda n, w=N: np.zeros((n, w), np.uint16))
    with pytest.raises(ValueError, match="^encrypt_peritem_batch: h, r and m need the same number of rows$"):
        eng.encrypt_peritem_batch(N, 64, u16(2), u8(3), u8(3))
    with pytest.raises(ValueError, match="^encrypt_peritem_batch: h, r and m need the same number of rows$"):
        eng.encrypt_peritem_batch(N, 64, u16(3), u8(3), u8(2))
    with pytest.raises(ValueError, match="^decrypt_peritem_batch: f, fp and e need the same number of rows$"):
        eng.decrypt_peritem_batch(N, 64, 3, np.zeros((3, N), np.int8), u8(2), u16(3))
    with pytest.raises(ValueError, match="^decrypt_peritem_batch: f, fp and e need the same number of rows$"):
        eng.decrypt_peritem_batch(N, 64, 3, np.zeros((2, N), np.int8), u8(3), u16(3))
    with pytest.raises(ValueError, match="^encrypt_bytes_batch: 3 rows of r for 2 blocks$"):
        eng.encrypt_bytes_batch(N, 64, 2, np.zeros(N, np.uint16), u8(3), b"abcd")
    assert [c[0] for c in stub.calls] == ["ntru_engine_create"]


def test_device_pointer_wrapper():
    assert pkg.Engine._dp(0) is None and pkg.Engine._dp(None) is None
    assert pkg.Engine._dp(0x1000).value == 0x1000


# the records of test_dev_methods_and_launch_log, as the hand-written _dev methods wrote them for the same calls
LAUNCH_LOG = json.loads(r"""
[
 {"kernel": "k_stub", "N": 5, "items": 3, "bytes_per_item": 40},
 {"kernel": "k_stub", "N": 5, "items": 3, "bytes_per_item": 30},
 {"kernel": "k_stub", "N": 5, "items": 3, "bytes_per_item": 20},
 {"kernel": "k_stub", "N": 5, "items": 3, "bytes_per_item": 30},
 {"kernel": "k_stub", "N": 5, "items": 3, "bytes_per_item": 40},
 {"kernel": "k_stub", "N": 5, "items": 3, "bytes_per_item": 15},
 {"kernel": "k_stub", "N": 5, "items": 3, "bytes_per_item": 40},
 {"kernel": "k_stub", "N": 5, "items": 3, "bytes_per_item": 5},
 {"kernel": "k_stub", "N": 5, "items": 3, "bytes_per_item": 6},
 {"kernel": "k_stub", "N": 5, "items": 3, "bytes_per_item": 5},
 {"kernel": "k_stub", "N": 5, "items": 3, "bytes_per_item": 40},
 {"kernel": "k_stub", "N": 5, "items": 3, "bytes_per_item": 30},
 {"kernel": "k_stub", "N": 5, "items": 3, "bytes_per_item": 50},
 {"kernel": "k_stub", "N": 5, "items": 3, "bytes_per_item": 25},
 {"kernel": "k_stub", "N": 5, "items": 3, "bytes_per_item": 85},
 {"kernel": "k_stub", "N": 5, "items": 3, "bytes_per_item": 25},
 {"kernel": "k_stub", "N": 5, "items": 3, "bytes_per_item": 55},
 {"kernel": "k_stub", "N": 5, "items": 3, "bytes_per_item": 79},
 {"kernel": "k_stub", "N": 5, "items": 3, "bytes_per_item": 45},
 {"kernel": "k_stub", "N": 5, "items": 3, "bytes_per_item": 111},
 {"kernel": "k_stub", "N": 5, "items": 3, "bytes_per_item": 106},
 {"kernel": "k_stub", "N": 5, "items": 3, "bytes_per_item": 116},
 {"kernel": "k_stub", "N": 5, "items": 3, "bytes_per_item": 106}
]
""")


# _dev parameters without a default that may still be None
NULLABLE = {"decrypt_pack_batch": ["d_value"], "encrypt_pack_batch": ["d_e"], "invert_key_batch": ["d_fq", "d_fp"]}


def drive_dev(stub, eng):
    """Every _dev method with all its pointers, then with the optional ones left out (None where they have no default), then -- where
    there is one -- on the pitched symbol; checks the arguments of each call against the header."""
    for name in [n for n, (_, forms) in CASES.items() if "dev" in forms]:
        method = getattr(eng, name + "_dev")
        sig = inspect.signature(method)
        optional = [p for p, v in sig.parameters.items() if p.startswith("d_") and v.default is None]
        variants = [({}, "")] + ([({"omit": True}, "")] if optional or name in NULLABLE else [])
        if "ld" in sig.parameters:
            assert sig.parameters["ld"].default is None
            variants.append(({"ld": SCALARS["ld"]}, "_pitched"))
        for variant, infix in variants:
            symbol = "ntru_%s%s_dev" % (name, infix)
            kwargs, pointers = {}, {}
            for k, pname in enumerate(sig.parameters):
                cname = {"np_": "np"}.get(pname, pname)
                if pname == "B":
                    kwargs[pname] = B
                elif pname == "ld":
                    if "ld" in variant:
                        kwargs[pname] = variant["ld"]
                elif cname in SCALARS:
                    kwargs[pname] = SCALARS[cname]
                elif variant.get("omit") and pname in NULLABLE.get(name, []):
                    kwargs[pname] = None
                elif not (variant.get("omit") and pname in optional):
                    pointers[pname] = kwargs[pname] = 0x10000 * (k + 1)
            stub.peek = {}
            del stub.calls[:]
            assert method(**kwargs) is None
            (got, seen), = [c for c in stub.calls if c[0] != "ntru_engine_last_kernel"]
            assert got == symbol, (got, symbol)
            check_scalars(symbol, seen, SCALARS)
            for k, (htype, pname) in enumerate(PROTOS[symbol][1][1:], 1):
                if htype == "*":
                    assert seen[k] == ((pointers[pname], None) if pname in pointers else None), (symbol, pname, seen[k])


def test_dev_methods_and_launch_log(stub, monkeypatch, tmp_path):
    log = tmp_path / "launch.log"
    log.write_text("")
    monkeypatch.setenv("NTRU_LAUNCH_LOG", str(log))
    drive_dev(stub, pkg.Engine(0))
    assert [json.loads(line) for line in log.read_text().splitlines()] == LAUNCH_LOG
    assert log.read_text() == "".join('{"kernel": "%s", "N": %d, "items": %d, "bytes_per_item": %d}\n'
                                      % (r["kernel"], r["N"], r["items"], r["bytes_per_item"]) for r in LAUNCH_LOG)


def test_the_cases_cover_the_table():
    """A new row of the binding's table needs its case above."""
    forms = {}
    for call in getattr(engine, "_CALLS", []):
        forms.setdefault(call.name, set()).update(call.forms)
    for name, have in forms.items():
        assert name in CASES and have == set(CASES[name][1].split()), name
