"""Plain numpy statement of the feature budget (vksift_hip_keep_strongest, vksift_ext_keepStrongestFeatures): the specification. Integers and
bytes only, no torch, no GPU. A SIFT buffer is a (records, 164) uint8 array with a section table (nsec, off[16], cap[16]) and raw counters,
as in tests/np_records.py; an uploaded buffer is the table (1, [0], [n]) with the counter n.

  * rows are numbered in download order (test_section_walk.stored_rows)
  * key(row) = the 32 bits of the record's intensity field (byte 32) with the sign bit cleared, compared as an unsigned integer
  * rows ranked by (key descending, row ascending); the first min(total, max_features) are kept
  * kept rows stay in their section, keep their order and move to its front; the counters become the kept counts
  * total <= max_features: nothing changes, not even a counter above its capacity

keep_strongest() is written as a walk (threshold key, then a quota of ties in row order); tests/test_np_strongest.py compares it with a
sort."""
import numpy as np

from test_section_walk import stored_rows

REC = 164
KEY_AT = 32


def keys_of(recs):
    """(n, 164) record bytes -> (n,) uint32 keys"""
    recs = np.ascontiguousarray(np.asarray(recs, np.uint8).reshape(-1, REC)[:, KEY_AT:KEY_AT + 4])
    return recs.view("<u4").reshape(-1) & np.uint32(0x7FFFFFFF)


def keep_mask(keys, max_features):
    """which download-order rows are kept: every row above the threshold key, and the first rows at it until the budget is used up"""
    keys = np.asarray(keys, np.uint32)
    n = len(keys)
    if n <= max_features:
        return np.ones(n, bool)
    uniq = np.unique(keys)[::-1]
    above = 0
    for t in uniq:
        at = int((keys == t).sum())
        if above + at >= max_features:
            break
        above += at
    keep = keys > t
    quota = max_features - above
    ties = np.flatnonzero(keys == t)
    keep[ties[:quota]] = True
    return keep


def keep_strongest(buf, nsec, off, cap, found, max_features):
    """-> (buffer bytes after the call, counters after the call, stale: bool mask of the RECORDS of buf whose bytes are unspecified afterwards,
    kept: the download-order rows kept). Counters are the nsec raw counters; entries beyond nsec are returned as given."""
    assert max_features >= 1
    buf = np.asarray(buf, np.uint8).reshape(-1, REC)
    out, found_out = buf.copy(), [int(v) for v in found]
    stale = np.zeros(len(buf), bool)
    rows = stored_rows(nsec, off, cap, found)
    total = len(rows)
    if total <= max_features:
        return out, found_out, stale, np.arange(total)
    keep = keep_mask(keys_of(buf[rows]), max_features)
    base = 0
    for o in range(nsec):
        n = min(found[o], cap[o])
        k = keep[base:base + n]
        src = rows[base:base + n][k]
        out[off[o]:off[o] + len(src)] = buf[src]
        stale[off[o] + len(src):off[o] + n] = True
        found_out[o] = len(src)
        base += n
    return out, found_out, stale, np.flatnonzero(keep)


def selected_records(recs, max_features):
    """dense (n, 164) records in download order -> the kept ones, in order (what vksift_downloadFeatures returns after the call)"""
    recs = np.asarray(recs, np.uint8).reshape(-1, REC)
    return recs[keep_mask(keys_of(recs), max_features)].copy()
