"""Restatement of the feature tracks of vksift_ext_buildTracks / vksift_hip_build_tracks (plain module, no GPU): a sequential union-find over the nodes
(gpu_buffer_id, row) plus the numbering rule of include/vksift_ext.h.

  * a node is (gpu_buffer_id, row), row in download order; `rows[b]` is the number of rows buffer b holds
  * an edge joins (A, idx_a) and (B, idx_b); an edge with both ends on one node joins nothing; a record that names a row its buffer does not hold
    is no edge at all (the library's own producers leave none)
  * a track is a connected component of at least two nodes; tracks are numbered from 0 in the order of their smallest member by (gpu_buffer_id, row)
  * record: (gpu_buffer_id, row) of the smallest member, length = members, nb_buffers = distinct buffers among them; conflicting iff length > nb_buffers
  * stats: nb_tracks, nb_conflicting, nb_features = sum of the lengths, nb_edges = edges taken (inside one buffer, on one node, duplicates: all counted)
"""
import numpy as np

NO_TRACK = 0xFFFFFFFF
TRACK_DTYPE = np.dtype([("gpu_buffer_id", "<u4"), ("row", "<u4"), ("length", "<u4"), ("nb_buffers", "<u4")])
SOURCES = ("filtered", "verified_h", "verified_f", "refined_h", "refined_f", "guided")


def pair_edges(records, mask=None, valid=True):
    """the (idx_a, idx_b) of one pair that a source takes: every record (FILTERED, GUIDED), or the records whose mask byte is 1 of a pair whose model is
    valid (the four mask sources)"""
    rec = np.asarray(records)
    if rec.dtype.names:
        rec = np.stack([rec["idx_a"], rec["idx_b"]], axis=1)
    rec = rec.reshape(-1, 2).astype(np.int64)
    if not valid:
        return rec[:0]
    if mask is not None:
        rec = rec[np.asarray(mask)[:len(rec)] == 1]
    return rec


def build(rows, pairs):
    """rows: {gpu_buffer_id: rows held} for every buffer of the pair list. pairs: [(A, B, edges)] with edges an (n, 2) array of (idx_a, idx_b).
    -> (records TRACK_DTYPE, {gpu_buffer_id: uint32 word per row}, stats dict)"""
    ids = sorted(rows)
    base, total = {}, 0
    for b in ids:
        base[b] = total
        total += int(rows[b])
    parent = list(range(total))

    def find(x):
        while parent[x] != x:
            parent[x] = parent[parent[x]]
            x = parent[x]
        return x

    nb_edges = 0
    for a, b, edges in pairs:
        for ia, ib in np.asarray(edges, np.int64).reshape(-1, 2):
            if not (0 <= ia < rows[a] and 0 <= ib < rows[b]):
                continue
            nb_edges += 1
            u, v = find(base[a] + int(ia)), find(base[b] + int(ib))
            if u != v:
                parent[max(u, v)] = min(u, v)
    node_buf = np.concatenate([np.full(int(rows[b]), b, np.int64) for b in ids] + [np.zeros(0, np.int64)])
    roots = np.array([find(x) for x in range(total)], np.int64)
    # the smallest member of a component is its root (links go to the smaller index); tracks in the order of their roots
    members = {}
    for x, r in enumerate(roots):
        members.setdefault(int(r), []).append(x)
    records, number = [], {}
    for r in sorted(members):
        m = members[r]
        if len(m) < 2:
            continue
        assert min(m) == r
        number[r] = len(records)
        b = int(node_buf[r])
        records.append((b, r - base[b], len(m), len({int(node_buf[x]) for x in m})))
    words = np.array([number.get(int(r), NO_TRACK) for r in roots], np.uint32)
    per_buf = {b: words[base[b]:base[b] + int(rows[b])] for b in ids}
    rec = np.array(records, TRACK_DTYPE) if records else np.zeros(0, TRACK_DTYPE)
    stats = dict(nb_tracks=len(rec), nb_conflicting=int((rec["length"] > rec["nb_buffers"]).sum()), nb_features=int(rec["length"].sum()), nb_edges=nb_edges)
    return rec, per_buf, stats
