"""ctypes binding of include/ntru_engine.h (the engine's C ABI).  No computation happens here."""
import collections
import ctypes as C
import linecache
import os

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
_LIB = None

ERR_NAMES = {1: "NTRU_ERR_NO_DEVICE", 2: "NTRU_ERR_ARG", 3: "NTRU_ERR_UNSUPPORTED", 4: "NTRU_ERR_HIP"}
FLAG_INVALID_FQ, FLAG_INVALID_FP, FLAG_INVALID_H = 1, 2, 4
FLAG_NOT_UNIT_MOD2, FLAG_NOT_UNIT_MODP = 8, 16
# bits of the per-block flags of rows_to_bytes / decrypt_bytes_batch (include/ntru_engine.h)
FLAG_NOT_BITS, FLAG_PAD_NONZERO = 32, 64
# bits of the witness-check flags (include/ntru_engine.h NTRU_CHECK_*); VerifyDecrypt's second stage is shifted left by 3
CHECK_EQ, CHECK_TAIL, CHECK_RANGE = 1, 2, 4
# status codes of the generic family = the errors the reference throws (include/ntru_engine.h NTRU_GENERIC_*)
GENERIC_ERRORS = {1: "Cannot divide by zero polynomial.", 2: "No inverse exists for division.", 3: "invalid_gcd",
                  4: "ntru engine: generic work area exhausted"}


class EngineError(RuntimeError):
    def __init__(self, code, msg):
        super().__init__("%s: %s" % (ERR_NAMES.get(code, "error %d" % code), msg))
        self.code = code


def library_path():
    """The in-tree build; NTRU_ENGINE_LIB selects another build of the same C ABI (A/B measurements)."""
    return os.environ.get("NTRU_ENGINE_LIB") or os.path.join(_HERE, "lib", "libntru_engine.so")


# ---- the C prototypes, one letter per argument in the header's order: the whole ctypes vocabulary of this file --------------
_vp = C.c_void_p
_CT = {"p": _vp, "i": C.c_int, "l": C.c_int64, "u": C.c_uint64, "z": C.c_size_t, "s": C.c_char_p, "-": None,
       "P": C.POINTER(_vp), "I": C.POINTER(C.c_int), "Z": C.POINTER(C.c_size_t)}


def _sig(args, res="i"):
    """(restype, argtypes) of a prototype: p pointer (engine handles included), i int, l int64_t, u uint64_t, z size_t,
    s const char *, P / I / Z pointer to void * / int / size_t, - void; blanks only group."""
    return _CT[res], [_CT[c] for c in args.replace(" ", "")]


def _both(name, args):
    """The host-pointer and the _dev form of one prototype."""
    return {name: _sig(args), name + "_dev": _sig(args)}


# the calls that are written out by hand below
_SIGS = {
    "ntru_engine_device_count": _sig(""),
    "ntru_engine_create": _sig("i P"),
    "ntru_engine_destroy": _sig("p", "-"),
    "ntru_engine_set_stream": _sig("p p"),
    "ntru_engine_synchronize": _sig("p"),
    "ntru_engine_set_kernel_path": _sig("p i"),
    "ntru_engine_last_kernel": _sig("p", "s"),
    "ntru_last_error": _sig("", "s"),
    "ntru_engine_supports": _sig("i i"),
    "ntru_engine_set_sampler_rounds": _sig("p i"),
    "ntru_engine_get_sampler_rounds": _sig("p"),
    # the lift of decryptBits, a mode of the engine: the functions are in lift.py
    "ntru_engine_set_lift": _sig("p i"),
    "ntru_engine_get_lift": _sig("p"),
    **_both("ntru_sample_ternary", "p iiii p u l p"),
    "ntru_pack_params": _sig("i i IIII"),
    **_both("ntru_pack_batch", "p ii p l p"),
    **_both("ntru_unpack_batch", "p ii p i l p"),
    "ntru_pack_bytes_batch_dev": _sig("p ii p l p"),
    "ntru_pipeline_batch": _sig("p iii pppp u ii pp l pppp"),
    "ntru_pipeline_bytes_batch": _sig("p iii pppp u ii p i p l pppp"),
    "ntru_dev_alloc": _sig("p z P"),
    "ntru_dev_free": _sig("p p"),
    "ntru_dev_upload": _sig("p p p z"),
    "ntru_dev_download": _sig("p p p z"),
    "ntru_host_alloc": _sig("z", "p"),
    "ntru_host_free": _sig("p", "-"),
    "ntru_generic_capacity": _sig("i i"),
    "ntru_generic_multiply": _sig("p ii l pp l pp"),
    "ntru_generic_divide": _sig("p ii l pp l ppppp"),
    "ntru_generic_eea": _sig("p ii l pp l ppppp"),
    "ntru_generic_poly_inv": _sig("p ii l pp l ppp"),
    "ntru_multi_create": _sig("p i P"),
    "ntru_multi_destroy": _sig("p", "-"),
    "ntru_multi_engines": _sig("p"),
    "ntru_multi_set_lift": _sig("p i"),
    **_both("ntru_sum_groups", "p ii ppp ll p"),
    **_both("ntru_tally_decrypt_batch", "p iii ppppp ll ppppp"),
    # combining ciphertexts by a weight matrix: the functions are in combine.py
    **_both("ntru_combine_batch", "p ii pp l i p"),
    # a batch times one shared polynomial, with the split: the functions are in shared_product.py
    **_both("ntru_mul_shared_batch", "p ii pp l pp"),
    # the decryption noise of rows under a key, dense and packed: the functions are in noise.py
    **_both("ntru_noise_batch", "p ii pp l pp"),
    **_both("ntru_noise_packed_batch", "p ii pp l pp"),
    # ciphertexts as packOutput(q - 1, N, e) rows: the methods are in packed.py
    **_both("ntru_sum_groups_packed", "p ii ppp ll p"),
    **_both("ntru_tally_decrypt_packed_batch", "p iii ppppp ll ppppp"),
    **_both("ntru_decrypt_packed_batch", "p iii ppp l pppp"),
    # re-randomising and shuffling under the shared public key: the functions are in mix.py
    **_both("ntru_reencrypt_batch", "p ii ppp l p l pp"),
    # auditing a mix, checking revealed re-encryption links: the functions are in audit.py
    **_both("ntru_check_links_batch", "p iiiii pp p l p p l p l pp"),
    # the order of a mix step drawn on the device, and a whole mix step from a key: also in mix.py
    "ntru_argsort_keys_dev": _sig("p p l p"),
    **_both("ntru_draw_permutation", "p p u l pp"),
    **_both("ntru_mix_batch", "p iii pp u ii u p l pppp"),
    # scanning a batch for the rows a key decrypts to a tagged message: the functions are in scan.py
    **_both("ntru_scan_bytes_batch", "p iiiii ppp l ii p l ppp"),
    **_both("ntru_scan_bytes_packed_batch", "p iiiii ppp l ii p l ppp"),
    # counting the decrypted byte messages of a batch by choice and group: the functions are in count.py
    **_both("ntru_count_bytes_batch", "p iiii ppp l ii p ii u ii ppp"),
    **_both("ntru_count_bytes_packed_batch", "p iiii ppp l ii p ii u ii ppp"),
    # removing duplicates, dense and packed: the functions are in dedup.py
    "ntru_dedup_workspace_bytes": _sig("i l Z"),
    "ntru_dedup_rows": _sig("p ii p l p l u i ppp"), "ntru_dedup_rows_dev": _sig("p ii p l p l u i pppp"),
    "ntru_dedup_packed": _sig("p ii p l p l u i ppp"), "ntru_dedup_packed_dev": _sig("p ii p l p l u i pppp"),
    "ntru_keygen_workspace_bytes": _sig("i l Z"),
    **_both("ntru_keygen_batch", "p iiiii p u i l pppppppp"),
}

# ---- the regular batch calls, one row each ---------------------------------------------------------------------------------
# A regular call is  ntru_<name>(engine, scalars..., arrays with the batch count B among them).  From its row come the prototypes
# of its forms (_SIGS), the Engine host method (numpy arrays in and out), the Engine <name>_dev method (device pointers, plus
# its launch-log record) and the MultiEngine method (the ntru_multi_ symbol).  _derive() compiles them once, at import; print
# _host_source(row, "ntru_") / _dev_source(row) to read a method.
_Arr = collections.namedtuple("_Arr", "role name dt n want host blocks")
_Call = collections.namedtuple("_Call", "name scalars args forms note mismatch ret pitched doc dev_doc")
_B = None                # the place of the batch count (int64_t B) among the arrays
_i8, _u8, _u16, _u64 = np.int8, np.uint8, np.uint16, np.uint64


def _key(name, dt):
    """Shared input of shape (N,): a key every item uses."""
    return _Arr("key", name, dt, "N", None, name, False)


def _in(name, dt, n="N", host=None, blocks=False):
    """Per-item input [B][n], n an expression in the scalars; host: its name in the host method where that differs from d_<name>;
    blocks: message bytes, which may also come as a bytes object (_blocks)."""
    return _Arr("in", name, dt, n, None, host or name, blocks)


def _out(name, dt, n="N", want=None):
    """Output [B][n] ([B] with n None).  want: the keyword of the host method that gates an optional output; in the _dev method
    the pointer may then be None, and defaults to None where no required parameter follows."""
    return _Arr("out", name, dt, n, want, name, False)


def _call(name, scalars, *args, forms="host dev", note="sum", mismatch=None, ret=tuple, pitched=False, doc=None, dev_doc=None):
    """scalars: the int parameters after the engine, by name.  forms: which of host / dev / multi exist.  note: the bytes per item of
    the _dev method's launch-log record: "sum" = the row bytes of the per-item arrays passed, None = no record, else the expression.
    mismatch: the message (an expression) of the ValueError when per-item inputs differ in rows; unchecked without.  ret: dict returns
    the outputs by name.  pitched: ntru_<name>_pitched_dev exists (int ld after the scalars), selected by the _dev method's ld=."""
    return _Call(name, scalars.split(), args, forms.split(), note, mismatch, ret, pitched, doc, dev_doc)


_MSG = _in("bytes", _u8, "nbytes", host="data", blocks=True)
_WITNESS = (_out("quot1", _u16, want="want_witness"), _out("rem1", _u16, want="want_witness"), _out("quot2", _u8, want="want_witness"))
_CALLS = [
    _call("polymul_split", "N mod", _in("a", _u16), _in("b", _u16), _B, _out("quot", _u16), _out("rem", _u16), forms="host dev multi"),
    _call("split_by_I", "N mod", _in("a", _u16, "2 * N"), _B, _out("quot", _u16), _out("rem", _u16), note=None),
    _call("add_batch", "N mod", _in("a", _u16), _in("b", _u16), _B, _out("out", _u16), note=None),
    _call("encrypt_batch", "N q", _key("h", _u16), _in("r", _u8), _in("m", _u8), _B, _out("e", _u16),
          _out("quotE", _u16, want="want_quot"), forms="host dev multi", pitched=True,           # r, m in; e (+ quotientE) out
          dev_doc="ld: row pitch of r, m, e, quotE in elements (None = dense rows of N; see ntru_encrypt_batch_pitched_dev)."),
    _call("decrypt_batch", "N q p", _key("f", _i8), _key("fp", _u8), _in("e", _u16), _B, _out("value", _u8), *_WITNESS,
          forms="host dev multi", pitched=True,
          dev_doc="ld: row pitch of e, value, quot1, rem1, quot2 in elements (None = dense rows of N)."),
    # byte messages as packed bits (include/ntru_engine.h "byte messages"): blocks of nbytes <= N // 8 bytes, bit 7 first
    _call("bytes_to_rows", "N nbytes", _MSG, _B, _out("m", _u8),
          doc="[B][nbytes] message bytes -> [B][N] coefficient rows (stringToBits per block, zero pad)."),
    _call("rows_to_bytes", "N nbytes", _in("value", _u8), _B, _out("bytes", _u8, "nbytes"), _out("flags", _u8, None, want="want_flags"),
          doc="[B][N] rows -> ([B][nbytes] bytes of the low bits, [B] flags: FLAG_NOT_BITS | FLAG_PAD_NONZERO, or None)."),
    _call("encrypt_bytes_batch", "N q nbytes", _key("h", _u16), _in("r", _u8), _MSG, _B, _out("e", _u16),
          _out("quotE", _u16, want="want_quot"), note=None,
          mismatch='"encrypt_bytes_batch: %d rows of r for %d blocks" % (B, data.shape[0])',
          doc="encrypt_batch on the rows of bytes_to_rows(data); only nbytes per block go up."),
    _call("decrypt_bytes_batch", "N q p nbytes", _key("f", _i8), _key("fp", _u8), _in("e", _u16), _B, _out("bytes", _u8, "nbytes"),
          _out("flags", _u8, None, want="want_flags"), note=None,
          doc="rows_to_bytes of the value-only decrypt_batch; only nbytes (+ 1 flag byte) per block come down.  Returns (bytes, flags)."),
    _call("encrypt_peritem_batch", "N q", _in("h", _u16), _in("r", _u8), _in("m", _u8), _B, _out("e", _u16),
          _out("quotE", _u16, want="want_quot"), mismatch='"encrypt_peritem_batch: h, r and m need the same number of rows"',
          doc="encrypt_batch with a separate public key per item: h, r, m are [B][N]; row b of e / quotE is encrypt_batch of row b "
              "under h[b].", dev_doc="d_h: [B][N] public keys, one per item."),
    _call("decrypt_peritem_batch", "N q p", _in("f", _i8), _in("fp", _u8), _in("e", _u16), _B, _out("value", _u8), *_WITNESS,
          mismatch='"decrypt_peritem_batch: f, fp and e need the same number of rows"',
          doc="decrypt_batch with a separate private key per item: f, fp, e are [B][N]; row b is decrypt_batch of e[b] under f[b], fp[b].",
          dev_doc="d_f, d_fp: [B][N] private keys, one per item."),
    _call("verify_keys_batch", "N q p", _in("f", _i8), _in("g", _i8), _in("fq", _u16), _in("fp", _u8), _in("h", _u16), _B,
          _out("quot_fq", _u16), _out("rem_fq", _u16), _out("quot_fp", _u8), _out("rem_fp", _u8), _out("quot_h", _u16),
          _out("rem_h", _u16), _out("flags", _u8, None), forms="host dev multi", ret=dict,
          note="17 * N"),                      # the five operands and six witness rows; the flags byte was never counted
    _call("public_key_batch", "N q p", _in("fq", _u16), _in("g", _i8), _B, _out("h", _u16), forms="host dev multi",
          doc="generatePublicKeyH for B keys: rows of (p*fq mod q) * g mod (x^N - 1, q), untrimmed."),
    _call("invert_key_batch", "N q p", _in("f", _i8), _B, _out("fq", _u16, want="want_fq"), _out("fp", _u8, want="want_fp"),
          _out("flags", _u8, None), note=None,
          doc="loadPrivateKeyF / polyInv for B keys: (fq [B][N] u16, fp [B][N] u8, flags [B]); a set flag = not a unit.  "
              "want_fq / want_fp = False skips that half (its array comes back as None)."),
    # MultiEngine's form always computes both inverses
    _call("invert_key_batch", "N q p", _in("f", _i8), _B, _out("fq", _u16), _out("fp", _u8), _out("flags", _u8, None), forms="multi"),
    # witness checks (VerifyEncrypt / VerifyDecrypt / VerifyInverse): uint16 rows [B][N] and [B][N + 1] -> flags uint8[B]
    _call("check_encrypt_batch", "N q nq", _in("r", _u16), _in("m", _u16), _in("h", _u16), _in("quotE", _u16, "N + 1"),
          _in("remE", _u16, "N + 1"), _B, _out("flags", _u8, None)),
    _call("check_decrypt_batch", "N q nq p np_", _in("f", _u16), _in("fp", _u16), _in("e", _u16), _in("quot1", _u16, "N + 1"),
          _in("rem1", _u16, "N + 1"), _in("quot2", _u16, "N + 1"), _in("rem2", _u16, "N + 1"), _B, _out("flags", _u8, None)),
    _call("check_inverse_batch", "N M n", _in("f", _u16), _in("fq", _u16), _in("quotI", _u16, "N + 1"), _in("remI", _u16, "N + 1"),
          _B, _out("flags", _u8, None)),
    # scheme kernel + packOutput in one call.  A packed row is packOutput's output_size field elements of 32 bytes, which follows
    # from the value range (p - 1, q - 1) and is none of the row lengths above: the records spell it out (decrypt's for p = 3)
    _call("decrypt_pack_batch", "N q p", _key("f", _i8), _key("fp", _u8), _in("e", _u16), _B, _out("value", _u8),
          _out("packed", _u64, "4 * output_size"), forms="dev",
          note="2 * N + 32 * max(3, -(-N // 126)) + (N if d_value else 0)",                   # e in; packed rows (+ the plain values) out
          dev_doc="decryptBits + packOutput(p - 1, N, value) (one kernel on the matrix path); d_value may be None there."),
    _call("encrypt_pack_batch", "N q", _key("h", _u16), _in("r", _u8), _in("m", _u8), _B, _out("e", _u16),
          _out("packed", _u64, "4 * output_size"), forms="dev",                                            # r, m in; packed rows (+ e) out
          note="2 * N + 32 * max(3, -(-N // (252 // max(1, (q - 1).bit_length())))) + (2 * N if d_e else 0)",
          dev_doc="encryptBits + packOutput(q - 1, N, e) (one kernel with d_e None where the row-image matrix kernel applies)."),
]
for _c in _CALLS:
    _args = "p" + "i" * len(_c.scalars) + "".join("l" if a is _B else "p" for a in _c.args)
    _SIGS.update({"ntru_" + _c.name + ("_dev" if f == "dev" else ""): _sig(_args) for f in _c.forms if f != "multi"})
    if "multi" in _c.forms:
        _SIGS["ntru_multi_" + _c.name] = _sig(_args)
    if _c.pitched:
        _SIGS["ntru_%s_pitched_dev" % _c.name] = _sig(_args[:1 + len(_c.scalars)] + "i" + _args[1 + len(_c.scalars):])


def _preload_hip_runtime():
    """Keep ONE HIP runtime per process.  The PyTorch wheel bundles its own libamdhip64.so (same SONAME as
    /opt/rocm's, found through an RPATH under the plain name); if the engine pulled /opt/rocm's copy in first, a
    later `import torch` would load a second runtime that sees no device.  When torch is installed, load its copy
    first: the engine's NEEDED libamdhip64.so.7 then binds to it by SONAME.  Without torch (C, Node.js) the
    engine's RUNPATH finds /opt/rocm as usual."""
    import importlib.util
    try:
        spec = importlib.util.find_spec("torch")
    except (ImportError, ValueError):
        spec = None
    if spec and spec.submodule_search_locations:
        cand = os.path.join(list(spec.submodule_search_locations)[0], "lib", "libamdhip64.so")
        if os.path.exists(cand):
            C.CDLL(cand, mode=C.RTLD_GLOBAL)


def load_library():
    """dlopen the HIP engine.  Fails loudly when it has not been built (no fallback exists)."""
    global _LIB
    if _LIB is None:
        path = library_path()
        if not os.path.exists(path):
            raise EngineError(0, "HIP engine library %s is missing; run `python -c 'import __graft_entry__ as g; "
                                 "g.build()'` or `make -C ntru-circom_amd/csrc`" % path)
        _preload_hip_runtime()
        lib = C.CDLL(path)
        for name, (res, args) in _SIGS.items():
            fn = getattr(lib, name)
            fn.restype, fn.argtypes = res, args
        _LIB = lib
    return _LIB


def _np(a, dt, shape=None):
    arr = np.ascontiguousarray(np.asarray(a, dtype=dt))
    return arr.reshape(shape) if shape is not None else arr


def _ptr(arr):
    return None if arr is None else arr.ctypes.data_as(C.c_void_p)


def _blocks(a, nbytes):
    if isinstance(a, (bytes, bytearray, memoryview)):
        a = np.frombuffer(bytes(a), np.uint8)
    return _np(a, np.uint8).reshape(-1, nbytes)


# ---- the methods of the table's rows, as source text compiled once ---------------------------------------------------------
def _host_source(c, prefix):
    """Host method of a row: coerce every input (no copy where it already is contiguous and of the dtype), B from the first per-item
    input, allocate the outputs, call, return them."""
    arrays = [a for a in c.args if a is not _B]
    ins, outs = [a for a in arrays if a.role != "out"], [a for a in arrays if a.role == "out"]
    wants = list(dict.fromkeys(a.want for a in outs if a.want))
    items = [a.host for a in ins if a.role == "in"]
    body = []
    for a in ins:
        dt = "np." + np.dtype(a.dt).name
        body.append("%s = %s" % (a.host, "_np(%s, %s, (N,))" % (a.host, dt) if a.role == "key" else
                                 "_blocks(%s, %s)" % (a.host, a.n) if a.blocks else "_np(%s, %s).reshape(-1, %s)" % (a.host, dt, a.n)))
    body.append("B = %s.shape[0]" % items[0])
    if c.mismatch:
        body.append("if %s:" % " or ".join("%s.shape[0] != B" % x for x in items[1:]))
        body.append("    raise ValueError(%s)" % c.mismatch)
    for a in outs:
        body.append("%s = np.empty(%s, np.%s)%s" % (a.name, "(B, %s)" % a.n if a.n else "B", np.dtype(a.dt).name,
                                                  " if %s else None" % a.want if a.want else ""))
    call = ["self._h"] + c.scalars + ["B" if a is _B else "_ptr(%s)" % a.host for a in c.args]
    body.append("self._chk(self._lib.%s%s(%s))" % (prefix, c.name, ", ".join(call)))
    body.append("return " + ("{%s}" % ", ".join('"%s": %s' % (a.name, a.name) for a in outs) if c.ret is dict else
                             ", ".join(a.name for a in outs)))
    params = ["self"] + c.scalars + [a.host for a in ins] + [w + "=True" for w in wants]
    return "def %s(%s):\n    %s\n" % (c.name, ", ".join(params), "\n    ".join(body))


def _dev_source(c):
    """_dev method of a row: every pointer through _dp, then the launch-log record."""
    params, call, fixed, optional = [], [], {}, []
    for k, a in enumerate(c.args):
        if a is _B:
            params.append("B"), call.append("B")
            continue
        trailing = all(x is not _B and x.want for x in c.args[k:])
        params.append("d_%s%s" % (a.name, "=None" if trailing else "")), call.append("dp(d_%s)" % a.name)
        n = "1" if a.n is None else "(%s)" % a.n if " " in a.n else a.n
        if a.want:
            optional.append("(%d * %s if d_%s else 0)" % (np.dtype(a.dt).itemsize, n, a.name))
        elif a.role != "key":
            fixed[n] = fixed.get(n, 0) + np.dtype(a.dt).itemsize          # bytes per item of the arrays that are always passed
    note = ["%d * %s" % (size, n) for n, size in fixed.items()] + optional
    head = ["self._h"] + c.scalars
    sym = "self._chk(self._lib.ntru_%s%s_dev(%s))"
    body = ["dp = self._dp"]
    if c.pitched:
        params.append("ld=None")
        body += ["if ld is None:", "    " + sym % (c.name, "", ", ".join(head + call)),
                 "else:", "    " + sym % (c.name, "_pitched", ", ".join(head + ["int(ld)"] + call))]
    else:
        body.append(sym % (c.name, "", ", ".join(head + call)))
    if c.note:
        body.append("self._note(N, B, %s)" % (" + ".join(note) if c.note == "sum" else c.note))
    return "def %s_dev(%s):\n    %s\n" % (c.name, ", ".join(["self"] + c.scalars + params), "\n    ".join(body))


def _derive(cls, form):
    """Give cls the methods of every row that has the form: host, dev or multi."""
    for c in _CALLS:
        if form in c.forms:
            src = _dev_source(c) if form == "dev" else _host_source(c, "ntru_multi_" if form == "multi" else "ntru_")
            name = c.name + ("_dev" if form == "dev" else "")
            filename = "<%s.%s of %s>" % (cls.__name__, name, os.path.basename(__file__))
            linecache.cache[filename] = (len(src), None, src.splitlines(True), filename)    # tracebacks and inspect show the text
            ns = {}
            exec(compile(src, filename, "exec"), globals(), ns)
            fn = ns[name]
            fn.__qualname__, fn.__doc__ = "%s.%s" % (cls.__name__, name), c.dev_doc if form == "dev" else c.doc
            setattr(cls, name, fn)


class _Handle:
    """What Engine and MultiEngine share: the library, a handle from it, the error check, and the handle's release."""
    _destroy = None          # name of the C call that frees the handle

    def _chk(self, rc):
        if rc:
            raise EngineError(rc, self._lib.ntru_last_error().decode())

    def close(self):
        if self._h is not None:
            getattr(self._lib, self._destroy)(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class Engine(_Handle):
    """One engine per HIP device.  Host-buffer methods take/return numpy arrays; *_dev methods take raw
    device pointers (ints, e.g. torch.Tensor.data_ptr()) and only enqueue work on the engine's stream.
    The regular batch calls (encrypt_batch, decrypt_batch_dev, ...) are not written out here: they come from _CALLS."""
    _destroy = "ntru_engine_destroy"

    def __init__(self, device=0):
        self._lib = load_library()
        h = C.c_void_p()
        self._h = None
        self._chk(self._lib.ntru_engine_create(int(device), C.byref(h)))
        self._h = h
        self.device = int(device)

    # ---- launch log (profiling aid) ----------------------------------------------------------------------------
    # NTRU_LAUNCH_LOG=<path>: every single-kernel *_dev call appends {"kernel", "N", "items", "bytes_per_item"} in launch order;
    # tools/pmc_summary.py matches the k-th rocprofv3 dispatch of a kernel with the k-th record, so that per-launch counters are
    # scaled by the size of THAT launch (bench.py and tools/bench_configs.py launch one kernel at several sizes).
    def _note(self, N, items, bytes_per_item):
        path = os.environ.get("NTRU_LAUNCH_LOG")
        if path:
            with open(path, "a") as fh:
                fh.write('{"kernel": "%s", "N": %d, "items": %d, "bytes_per_item": %d}\n'
                         % (self.last_kernel(), int(N), int(items), int(bytes_per_item)))

    def set_stream(self, hip_stream):
        self._chk(self._lib.ntru_engine_set_stream(self._h, C.c_void_p(int(hip_stream) if hip_stream else None)))

    def set_kernel_path(self, path):
        """0 auto, 1 packed-u16 MAC kernels, 2 ternary add path, 3 add path without dot8, 4 int8 matrix-core path
        (matrix cores, two workgroups per CU), 5 (matrix cores, lock-step decrypt); each where applicable, same results."""
        self._chk(self._lib.ntru_engine_set_kernel_path(self._h, int(path)))

    def last_kernel(self):
        return self._lib.ntru_engine_last_kernel(self._h).decode()

    def synchronize(self):
        self._chk(self._lib.ntru_engine_synchronize(self._h))

    def supports(self, N, mod):
        return bool(self._lib.ntru_engine_supports(int(N), int(mod)))

    # ---- host buffers ------------------------------------------------------------------------------------
    @staticmethod
    def _groups(rows, offsets, K, weights):
        """(offsets as int64 or None, K, G, weights as uint16 or None) of a sum over the rows [B][N]."""
        B = rows.shape[0]
        if offsets is not None:
            offsets = _np(offsets, np.int64).reshape(-1)
            if offsets.size < 1 or (offsets.size > 1 and int(offsets[-1]) > B) or (offsets.size == 1 and int(offsets[0]) > B):
                raise ValueError("sum_groups: offsets must hold G + 1 row indices within the %d rows" % B)
            K, G = 0, offsets.size - 1
        else:
            K = B if K is None else int(K)
            if K < 1 or B % K:
                raise ValueError("sum_groups: %d rows are not whole groups of K = %s" % (B, K))
            G = B // K
        if weights is not None:
            weights = _np(weights, np.uint16).reshape(-1)
            if weights.size != B:
                raise ValueError("sum_groups: need one weight per row")
        return offsets, K, G, weights

    def sum_groups(self, N, mod, rows, offsets=None, K=None, weights=None):
        """out[g] = (sum of weights[row] * rows[row] over group g) % mod.  offsets: [G + 1] row indices (CSR), else uniform groups of K
        rows (K=None: one group of every row).  Returns [G][N] uint16."""
        rows = _np(rows, np.uint16).reshape(-1, N)
        offsets, K, G, weights = self._groups(rows, offsets, K, weights)
        out = np.empty((G, N), np.uint16)
        self._chk(self._lib.ntru_sum_groups(self._h, N, mod, _ptr(rows), _ptr(weights), _ptr(offsets), K, G, _ptr(out)))
        return out

    def tally_decrypt_batch(self, N, q, p, f, fp, rows, offsets=None, K=None, weights=None, want_witness=True):
        """sum_groups modulo q, then decrypt_batch of the sums.  Returns (sum, value, quot1, rem1, quot2)."""
        f, fp = _np(f, np.int8, (N,)), _np(fp, np.uint8, (N,))
        rows = _np(rows, np.uint16).reshape(-1, N)
        offsets, K, G, weights = self._groups(rows, offsets, K, weights)
        total = np.empty((G, N), np.uint16)
        value = np.empty((G, N), np.uint8)
        q1 = np.empty((G, N), np.uint16) if want_witness else None
        r1 = np.empty((G, N), np.uint16) if want_witness else None
        q2 = np.empty((G, N), np.uint8) if want_witness else None
        self._chk(self._lib.ntru_tally_decrypt_batch(self._h, N, q, p, _ptr(f), _ptr(fp), _ptr(rows), _ptr(weights), _ptr(offsets), K, G,
                                                     _ptr(total), _ptr(value), _ptr(q1), _ptr(r1), _ptr(q2)))
        return total, value, q1, r1, q2

    def pack_params(self, max_val, data_len):
        v = [C.c_int(0) for _ in range(4)]
        self._chk(self._lib.ntru_pack_params(int(max_val), int(data_len), *[C.byref(x) for x in v]))
        return dict(zip(("maxInputBits", "numInputsPerOutput", "arrLen", "outputSize"), (x.value for x in v)))

    def pack_batch(self, max_val, data_len, data):
        """[B][data_len] values -> [B][outputSize][4] little-endian uint64 limbs (index.js:572-596)."""
        data = _np(data, np.uint16).reshape(-1, data_len) if data_len else np.zeros((len(data), 0), np.uint16)
        B = data.shape[0]
        out = np.empty((B, self.pack_params(max_val, data_len)["outputSize"], 4), np.uint64)
        self._chk(self._lib.ntru_pack_batch(self._h, max_val, data_len, _ptr(data), B, _ptr(out)))
        return out

    def unpack_batch(self, max_val, packed_bits, limbs):
        """[B][packedSize][4] limbs -> [B][packedSize * per] values (index.js:598-620, untrimmed)."""
        limbs = _np(limbs, np.uint64)
        B, S = limbs.shape[0], limbs.shape[1]
        per = packed_bits // self.pack_params(max_val, 0)["maxInputBits"]
        out = np.empty((B, S * per), np.uint16)
        self._chk(self._lib.ntru_unpack_batch(self._h, max_val, packed_bits, _ptr(limbs), S, B, _ptr(out)))
        return out

    def set_sampler_rounds(self, rounds):
        """Rounds of the sampler's ChaCha block function: 20 (RFC 8439, default), 12 or 8."""
        self._chk(self._lib.ntru_engine_set_sampler_rounds(self._h, int(rounds)))

    def sampler_rounds(self):
        return int(self._lib.ntru_engine_get_sampler_rounds(self._h))

    def sample_ternary(self, N, n1, n2, other, key, first_item, B):
        """generateCustomArray on the device (ChaCha20 draw stream under `key`, 8 uint32)."""
        key = _np(key, np.uint32, (8,))
        out = np.empty((B, N), np.uint8)
        self._chk(self._lib.ntru_sample_ternary(self._h, N, n1, n2, other, _ptr(key), int(first_item), B, _ptr(out)))
        return out

    def sample_ternary_dev(self, N, n1, n2, other, key, first_item, B, d_out):
        key = _np(key, np.uint32, (8,))
        self._chk(self._lib.ntru_sample_ternary_dev(self._h, N, n1, n2, other, _ptr(key), int(first_item), B,
                                                    self._dp(d_out)))
        self._note(N, B, N)

    def pipeline_batch(self, N, q, p, h, m, f=None, fp=None, key=None, first_item=0, n1=0, n2=0, r=None,
                       want_r=False, want_e=False, want_value=False, want_packed=False):
        """ntru_pipeline_batch: sampler (key) or given r -> encryptBits -> decryptBits (f, fp) -> packOutput, device-resident between
        the stages; host arrays in and out.  Returns a dict of the outputs asked for."""
        h = _np(h, np.uint16, (N,))
        m = _np(m, np.uint8).reshape(-1, N)
        B = m.shape[0]
        f = None if f is None else _np(f, np.int8, (N,))
        fp = None if fp is None else _np(fp, np.uint8, (N,))
        key = None if key is None else _np(key, np.uint32, (8,))
        r = None if r is None else _np(r, np.uint8).reshape(-1, N)
        out = {}
        if want_r: out["r"] = np.empty((B, N), np.uint8)
        if want_e: out["e"] = np.empty((B, N), np.uint16)
        if want_value: out["value"] = np.empty((B, N), np.uint8)
        if want_packed:
            osz = self.pack_params(p - 1 if f is not None else q - 1, N)["outputSize"]
            out["packed"] = np.empty((B, osz, 4), np.uint64)
        self._chk(self._lib.ntru_pipeline_batch(self._h, N, q, p, _ptr(h), _ptr(f), _ptr(fp), _ptr(key), int(first_item), int(n1), int(n2),
                                                _ptr(r), _ptr(m), B, _ptr(out.get("r")), _ptr(out.get("e")), _ptr(out.get("value")),
                                                _ptr(out.get("packed"))))
        return out

    # ---- plain device buffers (for callers without torch: what the N-API addon hands to JavaScript) ----------------
    def dev_alloc(self, nbytes):
        p = _vp()
        self._chk(self._lib.ntru_dev_alloc(self._h, int(nbytes), C.byref(p)))
        return p.value

    def dev_free(self, d_ptr):
        self._chk(self._lib.ntru_dev_free(self._h, self._dp(d_ptr)))

    def dev_upload(self, d_ptr, host):
        host = np.ascontiguousarray(host)
        self._chk(self._lib.ntru_dev_upload(self._h, self._dp(d_ptr), _ptr(host), host.nbytes))

    def dev_download(self, d_ptr, shape, dtype):
        out = np.empty(shape, dtype)
        self._chk(self._lib.ntru_dev_download(self._h, _ptr(out), self._dp(d_ptr), out.nbytes))
        return out

    def pack_bytes_batch_dev(self, max_val, data_len, d_data, B, d_out):
        self._chk(self._lib.ntru_pack_bytes_batch_dev(self._h, int(max_val), int(data_len), self._dp(d_data), B, self._dp(d_out)))

    # ---- byte messages as packed bits (include/ntru_engine.h "byte messages"): blocks of nbytes <= N // 8 bytes, bit 7 first
    def pipeline_bytes_batch(self, N, q, p, nbytes, h, msg, f=None, fp=None, key=None, first_item=0, n1=0, n2=0, r=None,
                             want_r=False, want_e=False, want_msg=False, want_flags=False, out=None):
        """ntru_pipeline_bytes_batch: pipeline_batch with msg [B][nbytes] in place of m and msg_out / flags in place of value.
        `out` may hold preallocated arrays (e.g. pinned_empty) under "r", "e", "msg", "flags".  Returns a dict of the outputs."""
        h = _np(h, np.uint16, (N,))
        msg = _blocks(msg, nbytes)
        B = msg.shape[0]
        f = None if f is None else _np(f, np.int8, (N,))
        fp = None if fp is None else _np(fp, np.uint8, (N,))
        key = None if key is None else _np(key, np.uint32, (8,))
        r = None if r is None else _np(r, np.uint8).reshape(-1, N)
        out = dict(out or {})
        for name, want, shape, dt in (("r", want_r, (B, N), np.uint8), ("e", want_e, (B, N), np.uint16),
                                      ("msg", want_msg, (B, nbytes), np.uint8), ("flags", want_flags, (B,), np.uint8)):
            if want and name not in out:
                out[name] = np.empty(shape, dt)
            if name in out and (out[name].shape != shape or out[name].dtype != dt or not out[name].flags.c_contiguous):
                raise ValueError("pipeline_bytes_batch: out[%r] must be a contiguous %s array of shape %r" % (name, np.dtype(dt).name, shape))
        self._chk(self._lib.ntru_pipeline_bytes_batch(self._h, N, q, p, _ptr(h), _ptr(f), _ptr(fp), _ptr(key), int(first_item), int(n1),
                                                      int(n2), _ptr(r), nbytes, _ptr(msg), B, _ptr(out.get("r")), _ptr(out.get("e")),
                                                      _ptr(out.get("msg")), _ptr(out.get("flags"))))
        return out

    # ---- pinned host memory ---------------------------------------------------------------------------------
    def pinned_empty(self, shape, dtype):
        """numpy array over page-locked memory (ntru_host_alloc): the batch entry points DMA it in place.  The memory is
        released when the array (and every view of it) is gone."""
        dt = np.dtype(dtype)
        n = int(np.prod(shape)) * dt.itemsize
        p = self._lib.ntru_host_alloc(n)
        if not p:
            raise EngineError(4, self._lib.ntru_last_error().decode())
        lib = self._lib

        class _Owner:
            def __init__(self, ptr): self.ptr = ptr
            def __del__(self): lib.ntru_host_free(self.ptr)
        buf = (C.c_char * max(n, 1)).from_address(p)
        buf._owner = _Owner(p)
        return np.frombuffer(buf, dtype=dt, count=int(np.prod(shape))).reshape(shape)

    # ---- generic family (ntru_generic_*): int64 coefficients, uniform operand lengths per batch ---------------
    def _generic(self, op, a, b, mod, two):
        a, b = np.ascontiguousarray(a, dtype=np.int64), np.ascontiguousarray(b, dtype=np.int64)
        if a.ndim == 1: a = a[None]
        if b.ndim == 1: b = b[None]
        B, la, lb = a.shape[0], a.shape[1], b.shape[1]
        cap = self._lib.ntru_generic_capacity(la, lb)
        o0, l0 = np.zeros((B, cap), np.int64), np.zeros(B, np.int32)
        o1, l1 = (np.zeros((B, cap), np.int64), np.zeros(B, np.int32)) if two else (None, None)
        st = np.zeros(B, np.uint8)
        fn = [self._lib.ntru_generic_multiply, self._lib.ntru_generic_divide, self._lib.ntru_generic_eea,
              self._lib.ntru_generic_poly_inv][op]
        if op == 0:
            rc = fn(self._h, la, lb, int(mod), _ptr(a), _ptr(b), B, _ptr(o0), _ptr(l0))
        elif op == 3:
            rc = fn(self._h, la, lb, int(mod), _ptr(a), _ptr(b), B, _ptr(o0), _ptr(l0), _ptr(st))
        else:
            rc = fn(self._h, la, lb, int(mod), _ptr(a), _ptr(b), B, _ptr(o0), _ptr(l0), _ptr(o1), _ptr(l1), _ptr(st))
        self._chk(rc)
        rows = lambda o, l: [o[i, :l[i]].tolist() for i in range(B)]
        return rows(o0, l0), (rows(o1, l1) if two else None), st

    def generic_multiply(self, a, b, mod):
        """multiplyPolynomials per row (index.js:319-355), any modulus up to 2^26 -> list of trimmed lists."""
        return self._generic(0, a, b, mod, False)[0]

    def generic_divide(self, a, b, mod):
        """dividePolynomials per row (index.js:358-401) -> (quotients, remainders, status[B])."""
        return self._generic(1, a, b, mod, True)

    def generic_eea(self, a, b, mod):
        """extendedEuclideanAlgorithm per row (index.js:425-459) -> (gcds, inverses, status[B])."""
        return self._generic(2, a, b, mod, True)

    def generic_poly_inv(self, a, poly_i, mod):
        """polyInv per row (index.js:491-514) -> (inverses, status[B])."""
        r = self._generic(3, a, poly_i, mod, False)
        return r[0], r[2]

    # ---- key generation (generatePrivateKeyF + generateNewPublicKeyGH for B items, non-units redrawn on the device) -----------
    def keygen_workspace_bytes(self, N, B):
        n = C.c_size_t()
        self._chk(self._lib.ntru_keygen_workspace_bytes(int(N), int(B), C.byref(n)))
        return int(n.value)

    def keygen_batch(self, N, q, p, df, dg, key, B, first_item=0, max_tries=100, want=("f", "g", "fq", "fp", "h", "tries"),
                     packed_h=False, out=None):
        """ntru_keygen_batch: item i = first_item + b from the stream positions of include/ntru_engine.h.  Returns a dict of numpy
        arrays: `flags` always, the arrays named in `want` (f, g int8 [B][N]; fq, h uint16; fp uint8; tries uint8 [B]), and
        `packed_h` ([B][output_size][4] uint64, packOutput(q - 1, N, h)) on request.  out: dict of preallocated arrays to fill
        (e.g. from pinned_empty)."""
        key = _np(key, np.uint32, (8,))
        B = int(B)
        shapes = {"f": ((B, N), np.int8), "g": ((B, N), np.int8), "fq": ((B, N), np.uint16), "fp": ((B, N), np.uint8),
                  "h": ((B, N), np.uint16), "tries": ((B,), np.uint8), "flags": ((B,), np.uint8)}
        if packed_h:
            shapes["packed_h"] = ((B, self.pack_params(q - 1, N)["outputSize"], 4), np.uint64)
        out = dict(out or {})
        res = {}
        for name, (shape, dt) in shapes.items():
            if name in out:
                res[name] = out[name]
                assert res[name].dtype == dt and res[name].shape == shape and res[name].flags.c_contiguous, name
            elif name in want or name in ("flags", "packed_h"):
                res[name] = np.empty(shape, dt)
        g = lambda n: _ptr(res.get(n))
        self._chk(self._lib.ntru_keygen_batch(self._h, N, q, p, df, dg, _ptr(key), int(first_item), int(max_tries), B, g("f"), g("g"),
                                              g("fq"), g("fp"), g("h"), g("tries"), g("flags"), g("packed_h")))
        return res

    def keygen_batch_dev(self, N, q, p, df, dg, key, first_item, max_tries, B, d_work, d_f, d_g, d_fq, d_fp, d_h, d_tries, d_flags):
        """ntru_keygen_batch_dev on device pointers; d_work of keygen_workspace_bytes(N, B) bytes.  Synchronises the engine's stream
        (one 4-byte readback per call and per redraw pass)."""
        key = _np(key, np.uint32, (8,))
        dp = self._dp
        self._chk(self._lib.ntru_keygen_batch_dev(self._h, N, q, p, df, dg, _ptr(key), int(first_item), int(max_tries), int(B), dp(d_work),
                                                  dp(d_f), dp(d_g), dp(d_fq), dp(d_fp), dp(d_h), dp(d_tries), dp(d_flags)))

    # ---- device pointers (asynchronous) -------------------------------------------------------------------
    @staticmethod
    def _dp(x):
        return C.c_void_p(int(x)) if x else None

    def sum_groups_dev(self, N, mod, d_rows, d_out, G, d_offsets=None, K=None, d_weights=None):
        """d_offsets: DEVICE int64 [G + 1], or None for uniform groups of K rows."""
        dp = self._dp
        self._chk(self._lib.ntru_sum_groups_dev(self._h, N, mod, dp(d_rows), dp(d_weights), dp(d_offsets), int(K or 0), int(G), dp(d_out)))

    def tally_decrypt_batch_dev(self, N, q, p, d_f, d_fp, d_rows, d_sum, d_value, G, d_offsets=None, K=None, d_weights=None,
                                d_quot1=None, d_rem1=None, d_quot2=None):
        dp = self._dp
        self._chk(self._lib.ntru_tally_decrypt_batch_dev(self._h, N, q, p, dp(d_f), dp(d_fp), dp(d_rows), dp(d_weights), dp(d_offsets),
                                                         int(K or 0), int(G), dp(d_sum), dp(d_value), dp(d_quot1), dp(d_rem1),
                                                         dp(d_quot2)))


class MultiEngine(_Handle):
    """Several devices in one process (ntru_multi_*): a host batch is cut into contiguous shards, one engine + host thread per
    listed device id (an id may repeat).  Host numpy arrays in and out, same results as Engine; its batch methods come from _CALLS."""
    _destroy = "ntru_multi_destroy"

    def __init__(self, device_ids):
        self._lib = load_library()
        ids = (C.c_int * len(device_ids))(*[int(d) for d in device_ids])
        h = C.c_void_p()
        self._h = None
        self._chk(self._lib.ntru_multi_create(ids, len(device_ids), C.byref(h)))
        self._h = h

    def engines(self):
        return int(self._lib.ntru_multi_engines(self._h))


_derive(Engine, "host")
_derive(Engine, "dev")
_derive(MultiEngine, "multi")
