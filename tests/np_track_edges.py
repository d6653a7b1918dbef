"""Restatement of the edge store of vksift_ext_beginTrackAccumulation / vksift_ext_accumulateTrackEdges / vksift_ext_buildTracksAccumulated and of the launchers
under them, vksift_hip_append_track_edges / vksift_hip_build_tracks_from_edges (plain module, no GPU). The union step and the numbering are those of
tests/np_tracks.py, imported.

  * the store: `edges` (at most max_edges rows {A, idx_a, B, idx_b}, in the order they were appended), nb_dropped, nb_calls, nb_changed_buffers, and the row
    table {gpu_buffer_id: row count} of every buffer a call has named
  * accumulate(store, rows, pairs): `rows` {gpu_buffer_id: raw row count} of the buffers of the call, `pairs` [(A, B, edges)] in slot order with edges the
    (idx_a, idx_b) the source takes (np_tracks.pair_edges), in record order. An edge is appended iff both its rows are stored, i.e. below min(rows[b],
    max_rows); appended means written while the store holds fewer than max_edges, counted in nb_dropped afterwards. Then the row table: a buffer (below
    nb_buffers, if that is given) the table does not know gets its raw count; one whose count differs from the table's adds 1 to nb_changed_buffers
  * build(store, max_rows): np_tracks.build over the buffers of the table with min(table[b], max_rows) rows each and the stored edges; an edge that names a
    buffer the table does not know, or a row that is not stored, is no edge
"""
import numpy as np

import np_tracks as NT

EDGE_DTYPE = np.dtype([("gpu_buffer_id_a", "<u4"), ("row_a", "<u4"), ("gpu_buffer_id_b", "<u4"), ("row_b", "<u4")])
STATS = ("nb_edges", "nb_dropped", "nb_calls", "nb_changed_buffers")
UNSET = 0xFFFFFFFF


def begin(max_edges):
    assert max_edges > 0
    return dict(max_edges=int(max_edges), edges=[], nb_dropped=0, nb_calls=0, nb_changed_buffers=0, table={})


def accumulate(store, rows, pairs, max_rows=None, nb_buffers=None):
    stored = {b: int(n) if max_rows is None else min(int(n), max_rows) for b, n in rows.items()}
    for a, b, edges in pairs:
        for ia, ib in np.asarray(edges, np.int64).reshape(-1, 2):
            if not (0 <= ia < stored[a] and 0 <= ib < stored[b]):
                continue
            if len(store["edges"]) < store["max_edges"]:
                store["edges"].append((a, int(ia), b, int(ib)))
            else:
                store["nb_dropped"] += 1
    store["nb_calls"] += 1
    for b in sorted(rows):
        if nb_buffers is not None and b >= nb_buffers:
            continue
        n = min(int(rows[b]), UNSET - 1)
        if b not in store["table"]:
            store["table"][b] = n
        elif store["table"][b] != n:
            store["nb_changed_buffers"] += 1
    return store


def stats(store):
    return dict(nb_edges=len(store["edges"]), nb_dropped=store["nb_dropped"], nb_calls=store["nb_calls"], nb_changed_buffers=store["nb_changed_buffers"])


def edge_records(store):
    return np.array(store["edges"], np.uint32).reshape(-1, 4).view(EDGE_DTYPE).reshape(-1)


def build_from_edges(rows, edges):
    """rows: {gpu_buffer_id: stored rows} of the participating buffers; edges: (n, 4) {A, idx_a, B, idx_b} -> what np_tracks.build returns"""
    e = np.asarray(edges, np.int64).reshape(-1, 4)
    known = np.array([a in rows and b in rows for a, _, b, _ in e], bool)
    e = e[known]
    groups = {}
    for a, ia, b, ib in e:
        groups.setdefault((int(a), int(b)), []).append((ia, ib))
    return NT.build(rows, [(a, b, np.array(v, np.int64)) for (a, b), v in groups.items()])


def build(store, max_rows):
    rows = {b: min(n, max_rows) for b, n in store["table"].items()}
    return build_from_edges(rows, np.array(store["edges"], np.int64).reshape(-1, 4))
