"""Restatement of the observation table of vksift_ext_selectTrackObservations / vksift_hip_track_observations (plain module, no GPU), from the outputs of
tests/np_tracks.py's build() (or the downloads of a built instance):

  * track t is selected iff length >= min_length, and (max_length == 0 or length <= max_length), and (conflicts == KEEP or length == nb_buffers)
  * nb_rejected_length: the tracks that fail the length test; nb_rejected_conflicting: those that pass it and are dropped as conflicting
  * selected tracks keep their order; track_ids[m] is the old number of selected track m
  * offsets[m] .. offsets[m + 1] are the observations of selected track m, its members in increasing (gpu_buffer_id, row); offsets[0] == 0
  * an observation is (gpu_buffer_id, row, x, y), x and y the bits of xy[gpu_buffer_id][row]
"""
import numpy as np

KEEP_CONFLICTING, DROP_CONFLICTING = 0, 1
NO_TRACK = 0xFFFFFFFF
OBSERVATION_DTYPE = np.dtype([("gpu_buffer_id", "<u4"), ("row", "<u4"), ("x", "<f4"), ("y", "<f4")])
STATS = ("nb_tracks", "nb_observations", "nb_rejected_length", "nb_rejected_conflicting")


def args_valid(min_length, max_length, conflicts):
    return min_length >= 2 and (max_length == 0 or max_length >= min_length) and conflicts in (KEEP_CONFLICTING, DROP_CONFLICTING)


def select(records, words, xy, min_length, max_length, conflicts):
    """records: the track records (np_tracks.TRACK_DTYPE); words: {gpu_buffer_id: uint32 word per row}; xy: {gpu_buffer_id: float32 [rows, 2]}.
    -> (stats dict, offsets uint32 [M + 1], track_ids uint32 [M], observations OBSERVATION_DTYPE)"""
    assert args_valid(min_length, max_length, conflicts)
    length, nbuf = records["length"].astype(np.int64), records["nb_buffers"].astype(np.int64)
    length_ok = (length >= min_length) & ((length <= max_length) if max_length else np.ones(len(records), bool))
    selected = length_ok & ((length == nbuf) if conflicts == DROP_CONFLICTING else np.ones(len(records), bool))
    track_ids = np.flatnonzero(selected).astype(np.uint32)
    new_number = np.full(len(records), -1, np.int64)
    new_number[track_ids] = np.arange(len(track_ids))
    # every member, in the order (gpu_buffer_id, row); a stable sort by the new number groups them
    ids = sorted(words)
    buf = np.concatenate([np.full(len(words[b]), b, np.int64) for b in ids] + [np.zeros(0, np.int64)])
    row = np.concatenate([np.arange(len(words[b]), dtype=np.int64) for b in ids] + [np.zeros(0, np.int64)])
    word = np.concatenate([np.asarray(words[b], np.uint32) for b in ids] + [np.zeros(0, np.uint32)]).astype(np.int64)
    pos = np.concatenate([np.asarray(xy[b], np.float32).reshape(-1, 2)[:len(words[b])] for b in ids] + [np.zeros((0, 2), np.float32)])
    number = np.where(word != NO_TRACK, new_number[np.minimum(word, max(len(records) - 1, 0))] if len(records) else -1, -1)
    member = np.flatnonzero(number >= 0)
    member = member[np.argsort(number[member], kind="stable")]
    obs = np.zeros(len(member), OBSERVATION_DTYPE)
    obs["gpu_buffer_id"], obs["row"] = buf[member], row[member]
    obs["x"], obs["y"] = pos[member, 0], pos[member, 1]
    offsets = np.zeros(len(track_ids) + 1, np.uint32)
    offsets[1:] = np.cumsum(np.bincount(number[member], minlength=len(track_ids)))[:len(track_ids)] if len(track_ids) else []
    stats = dict(nb_tracks=len(track_ids), nb_observations=len(obs), nb_rejected_length=int((~length_ok).sum()), nb_rejected_conflicting=int((length_ok & ~selected).sum()))
    return stats, offsets, track_ids, obs
