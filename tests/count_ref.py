"""Restatement of the count (include/ntru_engine.h "counting") without the engine, and the count fixture: decryptBits through the oracle
under either lift (tests/lift_ref.py), the byte codec and its flags from tests/message_bytes_ref.py, the classification in numpy.  The
checker of tests/test_count_gpu.py, tied to the reference by tests/test_count_cpu.py.  Not a test module."""
import json
import os

import numpy as np

import lift_ref
import message_bytes_ref as mb
from scan_ref import unpack

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "count_cases.json")
CT_LDS_BINS = 8192          # the largest table count_bytes.hip counts in LDS; pinned to the source by tests/test_count_cpu.py
MAX_CHOICES, MAX_BINS = 65536, 1 << 24


def load_cases():
    """The fixture with every packed array expanded: f, fp, h [2][N] (0 the counting key, 1 the foreign key), e [B][N] uint16, value
    [B][N] uint8, group and cls [B] int32, count [G][nChoices + 3] int64, tag as bytes."""
    with open(GOLDEN) as fh:
        cases = json.load(fh)["cases"]
    for c in cases:
        N = c["options"]["N"]
        for name, dt in (("f", np.int8), ("fp", np.uint8), ("h", np.uint16)):
            c[name] = np.array([unpack(k[name]) for k in c["keys"]]).astype(dt)
        c["e"] = unpack(c["e"]).reshape(-1, N).astype(np.uint16)
        c["value"] = unpack(c["value"]).reshape(-1, N).astype(np.uint8)
        c["group"], c["cls"], c["count"] = np.array(c["group"], np.int32), np.array(c["cls"], np.int32), np.array(c["count"], np.int64)
        c["tag"] = bytes(c["tag"])
    return cases


def layout(c):
    """The keyword arguments of classify / count_bytes / the calls under test that a fixture case fixes."""
    return dict(first_choice=c["firstChoice"], n_choices=c["nChoices"], field_off=c["fieldOffset"], field_len=c["fieldLength"],
                tag=c["tag"], tag_off=c["tagOffset"])


def classify(data, flags, first_choice, n_choices, field_off, field_len, tag=b"", tag_off=0):
    """cls [B] int32 of what decrypt_bytes_batch returns: data [B][nbytes], flags [B]."""
    data = np.asarray(data, np.uint8)
    tag = np.frombuffer(bytes(tag), np.uint8)
    assert 0 <= tag_off and tag_off + tag.size <= data.shape[1] and tag.size <= 32
    assert 1 <= field_len <= 4 and 0 <= field_off and field_off + field_len <= data.shape[1]
    assert 1 <= n_choices <= MAX_CHOICES and 0 <= first_choice < 1 << 32
    v = np.zeros(data.shape[0], np.int64)
    for j in range(field_len):
        v = v * 256 + data[:, field_off + j]
    cls = np.where((v < first_choice) | (v - first_choice >= n_choices), n_choices, v - first_choice)
    cls = np.where((data[:, tag_off:tag_off + tag.size] == tag).all(axis=1), cls, n_choices + 1)
    return np.where(np.asarray(flags) == 0, cls, n_choices + 2).astype(np.int32)


def tabulate(cls, n_choices, groups=None, G=1):
    """(count [G][n_choices + 3] int64, cls with -1 where the group id lies outside [0, G))."""
    cls = np.asarray(cls, np.int32).copy()
    groups = np.zeros(cls.size, np.int64) if groups is None else np.asarray(groups, np.int64)
    valid = (groups >= 0) & (groups < G)
    cls[~valid] = -1
    n_bins = n_choices + 3
    assert G >= 1 and G * n_bins <= MAX_BINS
    count = np.bincount(groups[valid] * n_bins + cls[valid], minlength=G * n_bins).astype(np.int64).reshape(G, n_bins)
    return count, cls


def count_data(data, flags, first_choice, n_choices, field_off, field_len, tag=b"", tag_off=0, groups=None, G=1):
    """The count of what decrypt_bytes_batch returns: (count, cls)."""
    return tabulate(classify(data, flags, first_choice, n_choices, field_off, field_len, tag, tag_off), n_choices, groups, G)


def count_values(value, nbytes, **kw):
    """count_data on decrypted coefficient rows value [B][N]."""
    return count_data(*mb.np_rows_to_bytes(value, nbytes), **kw)


def count_bytes(N, q, p, nbytes, f, fp, e, mode=lift_ref.REFERENCE, **kw):
    """The definition: decryptBits of every row of e under (f, fp) and the lift `mode`, then the classification: (count, cls)."""
    value = lift_ref.decrypt(N, q, p, np.asarray(f, np.int8), np.asarray(fp, np.uint8), e, mode)[0]
    return count_values(value, nbytes, **kw)
