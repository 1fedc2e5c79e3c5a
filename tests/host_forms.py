"""The regular host-pointer forms of include/ntru_engine.h and the ntru_multi_* forms, as data: every form's arguments in the
header's order with one valid parameter set, the scalars it must refuse, and the fixed list of bad-argument cases made from them.
tests/golden/record_host_form_errors.py records what a library answers to each case; tests/test_host_forms_gpu.py holds the
library under test to that record, and runs every form against its own _dev form on the same data."""
import collections
import ctypes as C

import numpy as np

Arr = collections.namedtuple("Arr", "role name dt n lo hi")       # n: elements per item (per call for a key), lo <= values < hi
Form = collections.namedtuple("Form", "name vals args bad opt_sets extra")
B = "B"                                                            # the place of int64_t B
POOL = 4096                                                        # elements of every array of an error case: a row of any accepted N
i8, u8, u16, u32, u64 = np.int8, np.uint8, np.uint16, np.uint32, np.uint64


def key(name, dt, n, hi, lo=0):
    """Shared input: the same row for every item."""
    return Arr("key", name, dt, n, lo, hi)


def inp(name, dt, n, hi, lo=0):
    return Arr("in", name, dt, n, lo, hi)


def out(name, dt, n="N"):
    return Arr("out", name, dt, n, 0, 0)


def opt(name, dt, n="N"):
    """Output that may be NULL."""
    return Arr("opt", name, dt, n, 0, 0)


def form(name, vals, args, bad, opt_sets=None, extra=()):
    """vals: one valid value per scalar (and per name an n uses).  args: the arguments after the engine: a scalar's name, B or an Arr.
    bad: (label, scalars to replace) the form must refuse.  opt_sets: which optional outputs the data runs ask for (default: all,
    then none).  extra: further cases (label, scalars to replace, arrays to pass as NULL, B)."""
    opts = tuple(a.name for a in args if isinstance(a, Arr) and a.role == "opt")
    return Form(name, vals, args, bad, opt_sets if opt_sets is not None else ([opts, ()] if opts else [()]), extra)


_NQ = [("q_not_pow2", {"q": 33}), ("N_1", {"N": 1})]
_P = [("p_pow2", {"p": 4})]
_WITNESS = [opt("quot1", u16), opt("rem1", u16), opt("quot2", u8)]
_ELEMENTWISE = [("N_0", {"N": 0}), ("mod_1", {"mod": 1}), ("mod_65537", {"mod": 65537})]
_BYTES = [("N_7", {"N": 7}), ("nbytes_0", {"nbytes": 0}), ("nbytes_over_N_8", {"nbytes": 2})]
_CHECK_N = [("N_1", {"N": 1})]
_SCHEME = {"N": 17, "q": 32, "p": 3}
_BYTES_VALS = {"N": 8, "q": 32, "p": 3, "nbytes": 1}
_CHECK_VALS = {"N": 2, "q": 64, "nq": 5, "p": 3, "np": 4, "M": 64, "n": 5}

_ENCRYPT = ["N", "q", key("h", u16, "N", 32), inp("r", u8, "N", 3), inp("m", u8, "N", 2), B, out("e", u16), opt("quotE", u16)]
_DECRYPT = ["N", "q", "p", key("f", i8, "N", 2, -1), key("fp", u8, "N", 3), inp("e", u16, "N", 32), B, out("value", u8)] + _WITNESS
_POLYMUL = ["N", "mod", inp("a", u16, "N", 32), inp("b", u16, "N", 32), B, out("quot", u16), out("rem", u16)]
_INVERT = ["N", "q", "p", inp("f", i8, "N", 2, -1), B, opt("fq", u16), opt("fp", u8), out("flags", u8, "1")]
_INVERT_SETS = [("fq", "fp"), ("fq",), ("fp",)]                     # "fq or fp, at least one"
_INVERT_EXTRA = [("only_fq", {}, ("fp",), 1), ("only_fp", {}, ("fq",), 1)]
_PUBLIC = ["N", "q", "p", inp("fq", u16, "N", 32), inp("g", i8, "N", 2, -1), B, out("h", u16)]
_VERIFY = ["N", "q", "p", inp("f", i8, "N", 2, -1), inp("g", i8, "N", 2, -1), inp("fq", u16, "N", 32), inp("fp", u8, "N", 3),
           inp("h", u16, "N", 32), B, out("quot_fq", u16), out("rem_fq", u16), out("quot_fp", u8), out("rem_fp", u8), out("quot_h", u16),
           out("rem_h", u16), out("flags", u8, "1")]
_PQ_WIDE = [("p_times_q_wide", {"q": 32768})]

FORMS = [
    form("ntru_encrypt_batch", _SCHEME, _ENCRYPT, _NQ),
    form("ntru_decrypt_batch", _SCHEME, _DECRYPT, _NQ + _P),
    form("ntru_polymul_split", {"N": 17, "mod": 32}, _POLYMUL, [("mod_100", {"mod": 100}), ("N_1", {"N": 1}), ("mod_0", {"mod": 0})]),
    form("ntru_invert_key_batch", _SCHEME, _INVERT, _NQ + [("p_5", {"p": 5})], _INVERT_SETS, _INVERT_EXTRA),
    form("ntru_public_key_batch", _SCHEME, _PUBLIC, _NQ + [("p_0", {"p": 0})] + _PQ_WIDE),
    form("ntru_verify_keys_batch", _SCHEME, _VERIFY, _NQ + _P + _PQ_WIDE),
    form("ntru_split_by_I", {"N": 17, "mod": 32}, ["N", "mod", inp("a", u16, "2 * N", 32), B, out("quot", u16), out("rem", u16)], _ELEMENTWISE),
    form("ntru_add_batch", {"N": 17, "mod": 32}, ["N", "mod", inp("a", u16, "N", 32), inp("b", u16, "N", 32), B, out("out", u16)],
         _ELEMENTWISE),
    # key: eight words the caller keeps on the host in both forms
    form("ntru_sample_ternary", {"N": 17, "n1": 3, "n2": 4, "other": 2, "first_item": 1000},
         ["N", "n1", "n2", "other", Arr("hostkey", "key", u32, "8", 0, 1 << 32), "first_item", B, out("out", u8)],
         [("N_0", {"N": 0}), ("n1_negative", {"n1": -1}), ("n1_n2_over_N", {"n1": 10, "n2": 10}), ("other_256", {"other": 256})]),
    # max_val = 31: five bits, 50 values per field element, three elements (12 limbs) per row of 17
    form("ntru_pack_batch", {"max_val": 31, "data_len": 17}, ["max_val", "data_len", inp("data", u16, "data_len", 32), B, out("out", u64, "12")],
         [("max_val_0", {"max_val": 0}), ("max_val_65536", {"max_val": 65536}), ("data_len_negative", {"data_len": -1})],
         extra=[("data_len_0_data_NULL", {"data_len": 0}, ("data",), 1)]),
    form("ntru_unpack_batch", {"max_val": 31, "packed_bits": 250, "packed_size": 3},
         ["max_val", "packed_bits", inp("in", u64, "4 * packed_size", 1 << 63), "packed_size", B, out("out", u16, "50 * packed_size")],
         [("max_val_0", {"max_val": 0}), ("packed_bits_3", {"packed_bits": 3}), ("packed_bits_300", {"packed_bits": 300}),
          ("packed_size_negative", {"packed_size": -1})],
         extra=[("packed_size_0_all_NULL", {"packed_size": 0}, ("in", "out"), 1),
                ("packed_size_0_B_negative", {"packed_size": 0}, ("in", "out"), -1)]),
    form("ntru_encrypt_peritem_batch", _SCHEME,
         ["N", "q", inp("h", u16, "N", 32), inp("r", u8, "N", 3), inp("m", u8, "N", 2), B, out("e", u16), opt("quotE", u16)], _NQ),
    form("ntru_decrypt_peritem_batch", _SCHEME,
         ["N", "q", "p", inp("f", i8, "N", 2, -1), inp("fp", u8, "N", 3), inp("e", u16, "N", 32), B, out("value", u8)] + _WITNESS, _NQ + _P),
    form("ntru_bytes_to_rows", _BYTES_VALS, ["N", "nbytes", inp("bytes", u8, "nbytes", 256), B, out("m", u8)], _BYTES),
    form("ntru_rows_to_bytes", _BYTES_VALS, ["N", "nbytes", inp("value", u8, "N", 3), B, out("bytes", u8, "nbytes"), opt("flags", u8, "1")],
         _BYTES),
    form("ntru_encrypt_bytes_batch", _BYTES_VALS,
         ["N", "q", "nbytes", key("h", u16, "N", 32), inp("r", u8, "N", 3), inp("bytes", u8, "nbytes", 256), B, out("e", u16), opt("quotE", u16)],
         _BYTES + [("q_not_pow2", {"q": 33})]),
    form("ntru_decrypt_bytes_batch", _BYTES_VALS,
         ["N", "q", "p", "nbytes", key("f", i8, "N", 2, -1), key("fp", u8, "N", 3), inp("e", u16, "N", 32), B, out("bytes", u8, "nbytes"),
          opt("flags", u8, "1")], _BYTES + [("q_not_pow2", {"q": 33})] + _P),
    form("ntru_check_encrypt_batch", _CHECK_VALS,
         ["N", "q", "nq", inp("r", u16, "N", 64), inp("m", u16, "N", 64), inp("h", u16, "N", 64), inp("quotE", u16, "N + 1", 64),
          inp("remE", u16, "N + 1", 64), B, out("flags", u8, "1")],
         _CHECK_N + [("q_1", {"q": 1}), ("q_65537", {"q": 65537}), ("nq_0", {"nq": 0}), ("nq_253", {"nq": 253})]),
    form("ntru_check_decrypt_batch", _CHECK_VALS,
         ["N", "q", "nq", "p", "np", inp("f", u16, "N", 64), inp("fp", u16, "N", 64), inp("e", u16, "N", 64), inp("quot1", u16, "N + 1", 64),
          inp("rem1", u16, "N + 1", 64), inp("quot2", u16, "N + 1", 64), inp("rem2", u16, "N + 1", 64), B, out("flags", u8, "1")],
         _CHECK_N + [("q_odd", {"q": 33}), ("nq_0", {"nq": 0}), ("p_1", {"p": 1}), ("np_0", {"np": 0}), ("np_253", {"np": 253})]),
    form("ntru_check_inverse_batch", _CHECK_VALS,
         ["N", "M", "n", inp("f", u16, "N", 64), inp("fq", u16, "N", 64), inp("quotI", u16, "N + 1", 64), inp("remI", u16, "N + 1", 64), B,
          out("flags", u8, "1")],
         _CHECK_N + [("M_1", {"M": 1}), ("M_65537", {"M": 65537}), ("n_0", {"n": 0}), ("n_253", {"n": 253})]),
]

MULTI_FORMS = [
    form("ntru_multi_encrypt_batch", _SCHEME, _ENCRYPT, _NQ),
    form("ntru_multi_decrypt_batch", _SCHEME, _DECRYPT, _NQ + _P),
    form("ntru_multi_verify_keys_batch", _SCHEME, _VERIFY, _NQ + _P + _PQ_WIDE),
    form("ntru_multi_polymul_split", {"N": 17, "mod": 32}, _POLYMUL, [("mod_100", {"mod": 100}), ("N_1", {"N": 1})]),
    form("ntru_multi_invert_key_batch", _SCHEME, _INVERT, _NQ + [("p_5", {"p": 5})], _INVERT_SETS, _INVERT_EXTRA),
    form("ntru_multi_public_key_batch", _SCHEME, _PUBLIC, _NQ + [("p_0", {"p": 0})] + _PQ_WIDE),
]
assert len(FORMS) == 20 and len(MULTI_FORMS) == 6


def arrays(f):
    return [a for a in f.args if isinstance(a, Arr)]


def row_len(f, a, vals=None):
    return int(eval(a.n, {}, dict(vals or f.vals)))


def invoke(lib, symbol, handle, f, vals, ptrs, count):
    """symbol(handle, arguments of f in order): scalars from vals, addresses (or None) from ptrs, count for B."""
    args = [count if a is B else C.c_void_p(ptrs.get(a.name)) if isinstance(a, Arr) else vals[a] for a in f.args]
    return getattr(lib, symbol)(handle, *args)


def error_cases(f):
    """The fixed case list of one form: (label, handle given?, scalars to replace, arrays passed as NULL, B)."""
    every = tuple(a.name for a in arrays(f) if a.role != "hostkey")
    optional = tuple(a.name for a in arrays(f) if a.role == "opt")
    cases = [("engine_NULL", False, {}, (), 1), ("B_negative", True, {}, (), -1)]
    cases += [(label, True, repl, (), 1) for label, repl in f.bad]
    cases += [("NULL_" + a.name, True, {}, (a.name,), 1) for a in arrays(f) if a.role != "opt"]
    cases += [("B_0_all_NULL", True, {}, every, 0)]
    if optional:
        cases += [("optional_NULL", True, {}, optional, 1)]
    cases += [("engine_NULL_B_negative_" + f.bad[0][0], False, f.bad[0][1], (), -1)]
    cases += [(label, True, repl, null, count) for label, repl, null, count in f.extra]
    return cases


def run_error_cases(lib, f, handle):
    """{label: [return code, ntru_last_error() when the code is not 0]} of every case of f."""
    pool = {a.name: np.zeros(POOL, a.dt) for a in arrays(f)}
    got = {}
    for label, with_handle, repl, null, count in error_cases(f):
        ptrs = {name: None if name in null else arr.ctypes.data for name, arr in pool.items()}
        rc = invoke(lib, f.name, handle if with_handle else None, f, dict(f.vals, **repl), ptrs, count)
        got[label] = [int(rc), lib.ntru_last_error().decode() if rc else ""]
    return got
