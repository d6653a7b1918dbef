"""Plain numpy restatement of the seven record-moving launches of include/vksift_hip.h (records.hip, k_shifted_norms of match.hip,
k_gather_corr of verify.hip, k_gather_xy of guided.hip): integers, bytes, and IEEE fp32 operations spelled out with np.float32. No torch,
no GPU. Every function works on the arrays a test lays out, never on the product's own buffers:

  * a SIFT buffer is a (records, 164) uint8 array, a 2-NN table an (n, 5) uint32 array {idx_a, idx_b1, idx_b2, dist1 bits, dist2 bits}
  * a section table is (nsec, off[16], cap[16]) and the raw counters `found`; the stored rows of a buffer in download order are
    test_section_walk.stored_rows — the ONE statement of the walk, which tests/test_section_walk.py compares with records.h row by row
  * a layout word is LAYOUT_DENSE | n (n dense records) or the index of a 33-word table {nsec, off[16], cap[16]} in `layouts`

tests/test_np_records.py pins these against the CPU oracle and against int64 arithmetic."""
import numpy as np

from test_section_walk import MAX_SECTIONS, stored_rows

f32 = np.float32
REC, REC_WORDS, DESC_AT = 164, 41, 36
LAYOUT_DENSE = 0x80000000
LAYOUT_WORDS = 1 + 2 * MAX_SECTIONS
QUIET_NAN = 0x7FC00000
ZERO_ROW_NORM = 128 ** 3   # shifted norm of an all-zero descriptor (the padding rows of quirk Q6)


def descriptors(recs):
    """(n, 164) record bytes -> (n, 128) descriptor rows"""
    return np.asarray(recs, np.uint8).reshape(-1, REC)[:, DESC_AT:DESC_AT + 128]


def shifted_norms(rows):
    """sum over the 128 bytes of (byte - 128)^2, in int64"""
    rows = np.asarray(rows, np.uint8).reshape(-1, 128)
    return ((rows.astype(np.int64) - 128) ** 2).sum(1)


def gather_descriptors(recs, n):
    return descriptors(recs)[:n].copy()


def gather_sections(buf, nsec, off, cap, counts, pad_rows_to):
    """(dense rows incl. the zero padding rows below pad_rows_to, their norms as uint32, the row total) of one buffer; counts: found, or the
    fixed counts of the call"""
    rows = stored_rows(nsec, off, cap, counts)
    total = len(rows)
    out = np.zeros((max(total, pad_rows_to), 128), np.uint8)
    out[:total] = descriptors(buf)[rows]
    return out, shifted_norms(out).astype(np.uint32), total


def pack_features(buf, nsec, off, cap, found):
    """the stored records of one buffer in download order, (total, 164) bytes"""
    return np.asarray(buf, np.uint8).reshape(-1, REC)[stored_rows(nsec, off, cap, found)].copy()


def quotient_below(d1_bits, d2_bits, ratio):
    """fl32(d1 / d2) < ratio on raw bit patterns (a NaN quotient compares false)"""
    with np.errstate(all="ignore"):
        q = np.asarray(d1_bits, np.uint32).view(f32) / np.asarray(d2_bits, np.uint32).view(f32)
        return q < f32(ratio)


def filter_matches(fwd, rev, nb, ratio):
    """fwd: (na, 5) uint32 forward records; rev: None or the reverse table (any number of rows: only rows below nb are looked at).
    -> (kept, 4) uint32 {fwd[i].idx_a, j, d1 bits, d2 bits} in increasing i"""
    fwd = np.asarray(fwd, np.uint32).reshape(-1, 5)
    keep = quotient_below(fwd[:, 3], fwd[:, 4], ratio)
    if rev is not None:
        rev = np.asarray(rev, np.uint32).reshape(-1, 5)
        for i in np.flatnonzero(keep):
            j = int(fwd[i, 1])
            keep[i] = j < nb and int(rev[j, 1]) == i and bool(quotient_below(rev[j, 3:4], rev[j, 4:5], ratio)[0])
    return fwd[keep][:, [0, 1, 3, 4]].copy()


def layout_rows(word, layouts, found, found_buf_stride):
    """stored rows, in download order, of a buffer named with layout word `word`; found: the counters from the buffer's own first one on
    (sections at or beyond found_buf_stride count as empty and their counters are never looked at)"""
    word = int(word)
    if word & LAYOUT_DENSE:
        return np.arange(word & 0x7FFFFFFF, dtype=np.int64)
    t = np.asarray(layouts, np.uint32).reshape(-1)[word * LAYOUT_WORDS:(word + 1) * LAYOUT_WORDS]
    nsec = min(int(t[0]), int(found_buf_stride), MAX_SECTIONS)
    return stored_rows(nsec, [int(v) for v in t[1:1 + MAX_SECTIONS]], [int(v) for v in t[1 + MAX_SECTIONS:]], [int(v) for v in found[:nsec]])


def xy_words(buf, rows):
    """words 0, 1 (x, y) of the given stored rows, as bit patterns"""
    return np.asarray(buf, np.uint8).reshape(-1, REC)[rows][:, :8].copy().view(np.uint32).reshape(-1, 2)


def gather_correspondences(buf_a, rows_a, buf_b, rows_b, filtered, n):
    """(n, 4) uint32 bit patterns {xa, ya, xb, yb} of the first n filtered records (n already clamped to max_n); a side whose row is >= its
    buffer's total is a quiet NaN, the other side is not affected"""
    out = np.full((n, 4), QUIET_NAN, np.uint32)
    filtered = np.asarray(filtered, np.uint32).reshape(-1, 4)
    for side, (buf, rows) in enumerate(((buf_a, rows_a), (buf_b, rows_b))):
        idx = filtered[:n, side].astype(np.int64)
        ok = idx < len(rows)
        if ok.any():
            out[ok, 2 * side:2 * side + 2] = xy_words(buf, rows[idx[ok]])
    return out


def gather_xy(buf, rows, max_n):
    """(min(total, max_n), 2) uint32 bit patterns of one side"""
    return xy_words(buf, rows[:min(len(rows), max_n)])
