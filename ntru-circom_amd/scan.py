"""Scanning a batch of ciphertexts for the rows a key decrypts to a well-formed message that carries an expected tag
(include/ntru_engine.h "scanning"): decryptStr (index.js:84-86) on decryptBits (index.js:111-140) for every row under each of K keys,
tested and compacted on the device, so that only the hits cross the bus.  Functions on an Engine: its class keeps the methods it had."""
import numpy as np

from .engine import _np, _ptr
from .packed import _packed

MAX_TAG = 32          # NTRU_SCAN_MAX_TAG


def _keys(N, f, fp):
    """f [K][N] int8 (or (N,) for one key), fp likewise uint8."""
    f, fp = _np(f, np.int8).reshape(-1, N), _np(fp, np.uint8).reshape(-1, N)
    if f.shape[0] != fp.shape[0]:
        raise ValueError("scan: %d rows of f for %d rows of fp" % (f.shape[0], fp.shape[0]))
    return f, fp, f.shape[0]


def _tag(tag):
    tag = np.frombuffer(bytes(tag), np.uint8) if isinstance(tag, (bytes, bytearray, memoryview)) else _np(tag, np.uint8).reshape(-1)
    return np.ascontiguousarray(tag)


def _host(eng, fn, N, q, p, nbytes, f, fp, rows, tag, tag_off, max_hits):
    f, fp, K = _keys(N, f, fp)
    tag = _tag(tag)
    B = rows.shape[0]
    max_hits = B if max_hits is None else int(max_hits)
    count = np.zeros(K, np.int64)
    hit_row = np.empty((K, max(max_hits, 0)), np.int64)
    hit_bytes = np.empty((K, max(max_hits, 0), nbytes), np.uint8)
    eng._chk(fn(eng._h, N, q, p, nbytes, K, _ptr(f), _ptr(fp), _ptr(rows), B, int(tag_off), tag.size, _ptr(tag) if tag.size else None,
                max_hits, _ptr(hit_row) if max_hits > 0 else None, _ptr(hit_bytes) if max_hits > 0 else None, _ptr(count)))
    stored = np.minimum(count, max_hits)
    return count, [hit_row[k, :stored[k]].copy() for k in range(K)], [hit_bytes[k, :stored[k]].copy() for k in range(K)]


def scan_bytes_batch(eng, N, q, p, nbytes, f, fp, e, tag=b"", tag_off=0, max_hits=None):
    """f [K][N], fp [K][N] private keys, e [B][N] uint16.  Row b is a hit for key k when decrypt_bytes_batch under key k gives flag 0
    and bytes [tag_off, tag_off + len(tag)) equal to tag.  Returns (count [K] int64 -- every hit, may exceed max_hits --, hit_row,
    hit_bytes): lists of K arrays with the first min(count[k], max_hits) hits in ascending row order, [.] int64 and [.][nbytes] uint8.
    max_hits=None keeps every hit; 0 only counts."""
    return _host(eng, eng._lib.ntru_scan_bytes_batch, N, q, p, nbytes, f, fp, _np(e, np.uint16).reshape(-1, N), tag, tag_off, max_hits)


def scan_bytes_packed_batch(eng, N, q, p, nbytes, f, fp, packed, tag=b"", tag_off=0, max_hits=None):
    """scan_bytes_batch on rows that arrive as packOutput(q - 1, N, e): uint64 [B][outputSize][4]."""
    return _host(eng, eng._lib.ntru_scan_bytes_packed_batch, N, q, p, nbytes, f, fp, _packed(eng, N, q, packed), tag, tag_off, max_hits)


def _dev(eng, fn, N, q, p, nbytes, K, d_f, d_fp, d_rows, B, d_count, tag, tag_off, max_hits, d_hit_row, d_hit_bytes):
    dp = eng._dp
    tag = _tag(tag)
    eng._chk(fn(eng._h, N, q, p, nbytes, int(K), dp(d_f), dp(d_fp), dp(d_rows), int(B), int(tag_off), tag.size,
                _ptr(tag) if tag.size else None, int(max_hits), dp(d_hit_row), dp(d_hit_bytes), dp(d_count)))


def scan_bytes_batch_dev(eng, N, q, p, nbytes, K, d_f, d_fp, d_e, B, d_count, tag=b"", tag_off=0, max_hits=0, d_hit_row=None,
                         d_hit_bytes=None):
    """The same on DEVICE pointers, enqueued on the engine's stream without synchronising: d_f [K][N] int8, d_fp [K][N] uint8, d_e
    [B][N] uint16, d_count [K] int64 (set, not accumulated), d_hit_row [K][max_hits] int64, d_hit_bytes [K][max_hits][nbytes] uint8
    (both may be None with max_hits = 0).  tag is host data, read now.  Nothing behind the stored prefixes is written."""
    _dev(eng, eng._lib.ntru_scan_bytes_batch_dev, N, q, p, nbytes, K, d_f, d_fp, d_e, B, d_count, tag, tag_off, max_hits, d_hit_row,
         d_hit_bytes)


def scan_bytes_packed_batch_dev(eng, N, q, p, nbytes, K, d_f, d_fp, d_packed, B, d_count, tag=b"", tag_off=0, max_hits=0, d_hit_row=None,
                                d_hit_bytes=None):
    """scan_bytes_batch_dev with d_packed, DEVICE uint64 [B][outputSize][4], in place of d_e."""
    _dev(eng, eng._lib.ntru_scan_bytes_packed_batch_dev, N, q, p, nbytes, K, d_f, d_fp, d_packed, B, d_count, tag, tag_off, max_hits,
         d_hit_row, d_hit_bytes)
