"""Plain numpy statement of the spatially distributed feature budget (vksift_hip_keep_grid, vksift_ext_keepStrongestFeaturesGrid): the
specification. Integers, bytes and float comparisons only, no torch, no GPU. Buffers, section tables, rows and key(row) are those of
tests/np_strongest.py.

  * x = the fp32 at byte 0 of the record, y = the fp32 at byte 4
  * bounds(size, n): the n - 1 bounds b[j] = (float)((double)j * size / n), j = 1 .. n - 1
  * cx = the number of column bounds with x >= b, cy likewise from y and the row bounds, cell = cy * grid_cols + cx. A comparison with a NaN
    is false: a NaN or a negative coordinate falls into column / row 0; -0.0 >= 0.0 holds; the bounds may be anything, in any order
  * C = grid_cols * grid_rows, q = N // C. total <= N: nothing changes. Otherwise
      phase 1: every cell keeps the first min(n_cell, q) of its rows by (key descending, row ascending)
      phase 2: of the rows not kept, the first N - (rows kept in phase 1) by (key descending, row ascending) are kept too
  * kept rows stay in their section, keep their order and move to its front; the counters become the kept counts (np_strongest.keep_strongest)

keep_mask_grid() is written with np_strongest.keep_mask's walk (threshold key, then a quota of ties in row order), cell by cell and then over
the rest; tests/test_np_spread.py compares it with stable sorts."""
import numpy as np

import np_strongest as NS
from test_section_walk import stored_rows

REC = NS.REC


def bounds(size, n):
    """the n - 1 bounds of n cells over `size` pixels, float32"""
    return np.array([np.float32(float(j) * int(size) / int(n)) for j in range(1, n)], np.float32)


def coords_of(recs):
    """(n, 164) record bytes -> x, y as float32 arrays"""
    xy = np.ascontiguousarray(np.asarray(recs, np.uint8).reshape(-1, REC)[:, :8]).view("<f4").reshape(-1, 2)
    return xy[:, 0].copy(), xy[:, 1].copy()


def cells_of(recs, grid_cols, col_bounds, row_bounds):
    """the cell of every record; col_bounds / row_bounds: any floats (grid_cols - 1 and grid_rows - 1 of them)"""
    x, y = coords_of(recs)
    bx, by = np.asarray(col_bounds, np.float32).reshape(-1), np.asarray(row_bounds, np.float32).reshape(-1)
    assert len(bx) == grid_cols - 1
    with np.errstate(invalid="ignore"):
        cx = (x[:, None] >= bx[None, :]).sum(axis=1)
        cy = (y[:, None] >= by[None, :]).sum(axis=1)
    return (cy * grid_cols + cx).astype(np.int64)


def keep_mask_grid(keys, cells, ncell, max_features):
    """which download-order rows are kept"""
    keys, cells = np.asarray(keys, np.uint32), np.asarray(cells)
    n = len(keys)
    if n <= max_features:
        return np.ones(n, bool)
    q = max_features // ncell
    keep = np.zeros(n, bool)
    for c in range(ncell if q else 0):
        idx = np.flatnonzero(cells == c)
        keep[idx[NS.keep_mask(keys[idx], q)]] = True
    left = max_features - int(keep.sum())
    rest = np.flatnonzero(~keep)
    assert len(rest) >= left
    if left:
        keep[rest[NS.keep_mask(keys[rest], left)]] = True
    return keep


def keep_grid(buf, nsec, off, cap, found, max_features, grid_cols, grid_rows, col_bounds, row_bounds):
    """np_strongest.keep_strongest with the grid rule: -> (buffer bytes after the call, counters after the call, stale: bool mask of the RECORDS of
    buf whose bytes are unspecified afterwards, kept: the download-order rows kept)"""
    assert max_features >= 1 and 1 <= grid_cols <= 16 and 1 <= grid_rows <= 16
    buf = np.asarray(buf, np.uint8).reshape(-1, REC)
    out, found_out = buf.copy(), [int(v) for v in found]
    stale = np.zeros(len(buf), bool)
    rows = stored_rows(nsec, off, cap, found)
    total = len(rows)
    if total <= max_features:
        return out, found_out, stale, np.arange(total)
    keep = keep_mask_grid(NS.keys_of(buf[rows]), cells_of(buf[rows], grid_cols, col_bounds, row_bounds), grid_cols * grid_rows, max_features)
    base = 0
    for o in range(nsec):
        n = min(found[o], cap[o])
        src = rows[base:base + n][keep[base:base + n]]
        out[off[o]:off[o] + len(src)] = buf[src]
        stale[off[o] + len(src):off[o] + n] = True
        found_out[o] = len(src)
        base += n
    return out, found_out, stale, np.flatnonzero(keep)


def selected_records(recs, max_features, image_width, image_height, grid_cols, grid_rows):
    """dense (n, 164) records in download order -> the kept ones, in order (what vksift_downloadFeatures returns after
    vksift_ext_keepStrongestFeaturesGrid)"""
    recs = np.asarray(recs, np.uint8).reshape(-1, REC)
    cells = cells_of(recs, grid_cols, bounds(image_width, grid_cols), bounds(image_height, grid_rows))
    return recs[keep_mask_grid(NS.keys_of(recs), cells, grid_cols * grid_rows, max_features)].copy()


def cell_counts(recs, image_width, image_height, grid_cols, grid_rows):
    """how many of the records lie in each cell"""
    recs = np.asarray(recs, np.uint8).reshape(-1, REC)
    cells = cells_of(recs, grid_cols, bounds(image_width, grid_cols), bounds(image_height, grid_rows))
    return np.bincount(cells, minlength=grid_cols * grid_rows)
