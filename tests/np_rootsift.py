"""Plain numpy statement of the RootSIFT conversion (vksift_hip_root_descriptors, vksift_ext_convertToRootSift): the specification. Integers and
bytes only, no float, no torch, no GPU.

A descriptor row d[0..127] (uint8) with s = sum(d), 0 <= s <= 32640:

  * s == 0: the row stays as it is (all zero)
  * otherwise out[i] = min(255, r_i), r_i the unique integer with (2 r_i - 1)^2 s <= 2^20 d[i] < (2 r_i + 1)^2 s, and 0 for d[i] == 0:
    512 sqrt(d[i] / s) rounded half up, exactly. COLMAP's round(512 x) of the L1-normalised, square-rooted bin, saturated to 255, without its
    floating-point rounding
  * of a 164-byte record only bytes 36..163 change

root_bins() restates r without a search: with m = floor(sqrt(2^20 d / s)) = isqrt(2^20 d // s), the inequalities say 2r - 1 <= m < 2r + 1, so
r = (m + 1) // 2; a bin is at most its row's sum, so 2^20 d // s is at most 2^20 and its integer square root is read off a table: m takes the
2m + 1 places m^2 .. (m + 1)^2 - 1. tests/test_np_rootsift.py compares it with big-integer arithmetic over the whole domain."""
import numpy as np

REC, DESC_AT = 164, 36
S_MAX = 128 * 255
_M = np.arange(1025, dtype=np.int64)
_ISQRT = np.repeat(_M, 2 * _M + 1)[:(1 << 20) + 1]    # isqrt(q) for 0 <= q <= 2^20


def root_bins(d, s):
    """r for bins d <= s of rows with byte sum s >= 1 (arrays that broadcast), unsaturated, as int64"""
    d, s = np.asarray(d, np.int64), np.asarray(s, np.int64)
    return (_ISQRT[(d << 20) // s] + 1) >> 1


def root_rows(rows):
    """(n, 128) uint8 descriptor rows -> their RootSIFT rows"""
    rows = np.asarray(rows, np.uint8).reshape(-1, 128)
    s = rows.sum(1, dtype=np.int64)[:, None]
    return np.minimum(root_bins(rows, np.maximum(s, 1)), 255).astype(np.uint8)   # (s == 0: every bin is 0, and r(0) = 0)


def convert_records(recs):
    """(n, 164) record bytes -> the records after the conversion: bytes 36..163 replaced, the nine head words as they were"""
    out = np.array(np.asarray(recs, np.uint8).reshape(-1, REC), copy=True)
    out[:, DESC_AT:] = root_rows(out[:, DESC_AT:])
    return out


def convert_buffer(buf, rows):
    """a SIFT buffer ((records, 164) bytes) after the conversion of its stored rows `rows` (test_section_walk.stored_rows); every other record as it was"""
    out = np.array(np.asarray(buf, np.uint8).reshape(-1, REC), copy=True)
    out[rows] = convert_records(out[rows])
    return out
