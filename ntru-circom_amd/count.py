"""Counting the decrypted byte messages of a batch by choice and group (include/ntru_engine.h "counting"): decryptStr (index.js:84-86) on
decryptBits (index.js:111-140) for every row under one key, classified on the device -- malformed, wrong tag, a choice outside the
range, or choice v - first_choice -- so that only the table count [G][n_choices + 3] and, when asked for, one class id per row cross the
bus.  Functions on an Engine: its class keeps the methods it had."""
import numpy as np

from .engine import _np, _ptr
from .packed import _packed
from .scan import _tag

MAX_CHOICES = 65536          # NTRU_COUNT_MAX_CHOICES
MAX_BINS = 1 << 24           # NTRU_COUNT_MAX_BINS


def other(n_choices):
    """NTRU_COUNT_OTHER: the bin of a well-formed, tagged message whose choice lies outside [first_choice, first_choice + n_choices)."""
    return n_choices


def bad_tag(n_choices):
    """NTRU_COUNT_BAD_TAG: the bin of a well-formed message that does not carry the tag."""
    return n_choices + 1


def malformed(n_choices):
    """NTRU_COUNT_MALFORMED: the bin of a row that does not decrypt to bits with an empty pad."""
    return n_choices + 2


def _host(eng, fn, N, q, p, nbytes, f, fp, rows, first_choice, n_choices, field_off, field_len, tag, tag_off, groups, G, classes):
    f, fp = _np(f, np.int8, (N,)), _np(fp, np.uint8, (N,))
    tag = _tag(tag)
    B = rows.shape[0]
    n_choices, G = int(n_choices), int(G)
    if groups is not None:
        groups = _np(groups, np.int32).reshape(-1)
        if groups.size != B:
            raise ValueError("count: %d group ids for %d rows" % (groups.size, B))
    # (a table the engine is going to refuse is not allocated at its stated size)
    ok = G >= 1 and 1 <= n_choices <= MAX_CHOICES and G * (n_choices + 3) <= MAX_BINS
    count = np.zeros((G, n_choices + 3) if ok else (1, 1), np.int64)
    cls = np.empty(B, np.int32) if classes else None
    eng._chk(fn(eng._h, N, q, p, nbytes, _ptr(f), _ptr(fp), _ptr(rows), B, int(tag_off), tag.size, _ptr(tag) if tag.size else None,
                int(field_off), int(field_len), int(first_choice), n_choices, G, _ptr(groups), _ptr(count), _ptr(cls)))
    return count, cls


def count_bytes_batch(eng, N, q, p, nbytes, f, fp, e, first_choice, n_choices, field_off, field_len, tag=b"", tag_off=0, groups=None, G=1,
                      classes=False):
    """f [N], fp [N]: one private key; e [B][N] uint16.  Row b's class, from what decrypt_bytes_batch gives for it, is the first that
    applies of: flag != 0 -> malformed(n_choices); bytes [tag_off, tag_off + len(tag)) != tag -> bad_tag(n_choices); v = the big-endian
    integer of bytes [field_off, field_off + field_len), v outside [first_choice, first_choice + n_choices) -> other(n_choices); else
    v - first_choice.  groups: [B] int32 ids in [0, G), or None (one group).  Returns (count [G][n_choices + 3] int64, classes [B] int32
    or None)."""
    return _host(eng, eng._lib.ntru_count_bytes_batch, N, q, p, nbytes, f, fp, _np(e, np.uint16).reshape(-1, N), first_choice, n_choices,
                 field_off, field_len, tag, tag_off, groups, G, classes)


def count_bytes_packed_batch(eng, N, q, p, nbytes, f, fp, packed, first_choice, n_choices, field_off, field_len, tag=b"", tag_off=0,
                             groups=None, G=1, classes=False):
    """count_bytes_batch on rows that arrive as packOutput(q - 1, N, e): uint64 [B][outputSize][4]."""
    return _host(eng, eng._lib.ntru_count_bytes_packed_batch, N, q, p, nbytes, f, fp, _packed(eng, N, q, packed), first_choice, n_choices,
                 field_off, field_len, tag, tag_off, groups, G, classes)


def _dev(eng, fn, N, q, p, nbytes, d_f, d_fp, d_rows, B, d_count, first_choice, n_choices, field_off, field_len, tag, tag_off, d_group, G,
         d_cls):
    dp = eng._dp
    tag = _tag(tag)
    eng._chk(fn(eng._h, N, q, p, nbytes, dp(d_f), dp(d_fp), dp(d_rows), int(B), int(tag_off), tag.size, _ptr(tag) if tag.size else None,
                int(field_off), int(field_len), int(first_choice), int(n_choices), int(G), dp(d_group), dp(d_count), dp(d_cls)))


def count_bytes_batch_dev(eng, N, q, p, nbytes, d_f, d_fp, d_e, B, d_count, first_choice, n_choices, field_off, field_len, tag=b"",
                          tag_off=0, d_group=None, G=1, d_cls=None):
    """The same on DEVICE pointers, enqueued on the engine's stream without synchronising: d_f [N] int8, d_fp [N] uint8, d_e [B][N]
    uint16, d_count [G][n_choices + 3] int64 (set, not accumulated), d_group [B] int32 or None (then G is 1), d_cls [B] int32 or None.
    tag is host data, read now.  A row whose group id lies outside [0, G) is counted nowhere and gets class -1."""
    _dev(eng, eng._lib.ntru_count_bytes_batch_dev, N, q, p, nbytes, d_f, d_fp, d_e, B, d_count, first_choice, n_choices, field_off,
         field_len, tag, tag_off, d_group, G, d_cls)


def count_bytes_packed_batch_dev(eng, N, q, p, nbytes, d_f, d_fp, d_packed, B, d_count, first_choice, n_choices, field_off, field_len,
                                 tag=b"", tag_off=0, d_group=None, G=1, d_cls=None):
    """count_bytes_batch_dev with d_packed, DEVICE uint64 [B][outputSize][4], in place of d_e."""
    _dev(eng, eng._lib.ntru_count_bytes_packed_batch_dev, N, q, p, nbytes, d_f, d_fp, d_packed, B, d_count, first_choice, n_choices,
         field_off, field_len, tag, tag_off, d_group, G, d_cls)
