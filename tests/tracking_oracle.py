"""Cell overlap and tracking restated in NumPy and plain Python for the tests of ``radar_processor_amd/tracking.py`` and
``csrc/rg_tracking.hip`` -- written from the contract of ``include/radargrid_hip.h`` ("Cell overlap and tracking") and the
identity rules of DESIGN.md K10, never from either implementation.

* :func:`overlap`: the contingency table of two label stacks with ``np.unique`` over int64 keys;
* :func:`relabel`: a label plane mapped through a per-cell table;
* :func:`advect_labels`: the motion restatement's nearest advection on the labels' bits;
* :func:`match` and :func:`identities`: successor / predecessor and the identity rules as loops over dictionaries;
* :func:`track`: the whole chain over a list of frames, with the motion of each step given.
"""
from __future__ import annotations

import numpy as np

import components_oracle as co
import motion_oracle as mo


def rows_of(labels, cell_ptr):
    """int64 ``[n, h, w]``: the table row of every pixel, ``-1`` for background and for labels above the plane's count."""
    labels = np.asarray(labels, dtype=np.int64)
    ptr = np.asarray(cell_ptr, dtype=np.int64)
    assert labels.ndim == 3 and ptr.shape == (labels.shape[0] + 1,)
    cells = (ptr[1:] - ptr[:-1])[:, None, None]
    return np.where((labels > 0) & (labels <= cells), ptr[:-1, None, None] + labels - 1, -1)


def overlap(labels_prev, ptr_prev, labels_next, ptr_next):
    """``(row_prev, row_next, count)`` int32 arrays sorted by ``(row_prev, row_next)``."""
    a, b = rows_of(labels_prev, ptr_prev), rows_of(labels_next, ptr_next)
    both = (a >= 0) & (b >= 0)
    keys, counts = np.unique((a[both] << 32) | b[both], return_counts=True)
    return (keys >> 32).astype(np.int32), (keys & 0xFFFFFFFF).astype(np.int32), counts.astype(np.int32)


def relabel(labels, cell_ptr, lut):
    """int32 of the labels' shape: ``lut[row]`` on the pixels of a cell whose row lies within ``lut``, else 0."""
    rows = rows_of(labels, cell_ptr)
    lut = np.asarray(lut, dtype=np.int32)
    ok = (rows >= 0) & (rows < len(lut))
    padded = np.concatenate((lut, np.zeros(1, np.int32)))
    return np.where(ok, padded[np.where(ok, rows, len(lut))], 0).astype(np.int32)


def advect_labels(labels, motion, lat, lead=1.0, substeps=1):
    """int32 ``[h, w]`` labels moved by ``lead`` intervals: the bits through ``motion_oracle.advect``, nearest, fill bits 0."""
    bits = np.ascontiguousarray(labels, dtype=np.int32).view(np.float32)
    return mo.advect(bits[None], motion, lat, (lead,), substeps, "nearest", 0.0)[0, 0].view(np.int32)


def match(pairs, area_prev, area_next, min_pixels=1, min_fraction=0.0):
    """``(succ, pred)`` as dicts row -> row from ``pairs = (row_prev, row_next, count)``; rows without a partner are absent."""
    best_next, best_prev = {}, {}
    for a, b, c in zip(*(np.asarray(v).tolist() for v in pairs)):
        if c < min_pixels or float(c) < min_fraction * float(min(int(area_prev[a]), int(area_next[b]))):
            continue
        if a not in best_next or (c, -b) > (best_next[a][0], -best_next[a][1]):
            best_next[a] = (c, b)
        if b not in best_prev or (c, -a) > (best_prev[b][0], -best_prev[b][1]):
            best_prev[b] = (c, a)
    return {a: b for a, (_, b) in best_next.items()}, {b: a for b, (_, a) in best_prev.items()}


def identities(succ, pred, n_next, prev_track, prev_parent, prev_age, next_id):
    """The identity rules.  Returns ``(track, parent, age, ended, next_id)`` as lists; ``ended`` holds ``(track, merged_into)``."""
    track, parent, age = [], [], []
    for b in range(n_next):
        a = pred.get(b)
        if a is None:
            track.append(next_id), parent.append(0), age.append(0)
            next_id += 1
        elif succ.get(a) == b:
            track.append(int(prev_track[a])), parent.append(int(prev_parent[a])), age.append(int(prev_age[a]) + 1)
        else:
            track.append(next_id), parent.append(int(prev_track[a])), age.append(0)
            next_id += 1
    ended = []
    for a in range(len(prev_track)):
        b = succ.get(a)
        if b is None:
            ended.append((int(prev_track[a]), 0))
        elif pred.get(b) != a:
            ended.append((int(prev_track[a]), track[b]))
    return track, parent, age, ended, next_id


def track(planes, threshold, motions, connectivity=8, min_pixels=1, min_fraction=0.0):
    """The tracker over ``planes`` (a list of float32 ``[h, w]``).  ``motions[k]`` moves the labels of frame ``k`` to frame
    ``k + 1``: ``None`` or ``(field float32 [ny, nx, 2], Lattice)``.  Returns one dict per frame: ``labels``, ``cell_ptr``,
    ``track_id``, ``parent_track``, ``age`` (int64), ``velocity`` (float64 ``[n, 2]``), ``ended`` (int64 ``[k, 2]``)."""
    frames, next_id, prev = [], 1, None
    for k, plane in enumerate(planes):
        labels, ptr = co.label(np.asarray(plane, np.float32)[None], threshold, connectivity=connectivity)
        table = co.stats(np.asarray(plane, np.float32)[None], labels, ptr)
        area = table["area"].astype(np.int64)
        centroid = table["sum_yx"].astype(np.float64) / area[:, None].astype(np.float64)
        n = len(area)
        velocity = np.full((n, 2), np.nan)
        if prev is None:
            ids, parent, age, ended = list(range(next_id, next_id + n)), [0] * n, [0] * n, []
            next_id += n
        else:
            moved = prev["labels"]
            if motions[k - 1] is not None:
                moved = advect_labels(moved[0], *motions[k - 1])[None]
            succ, pred = match(overlap(moved, prev["cell_ptr"], labels, ptr), prev["area"], area, min_pixels, min_fraction)
            ids, parent, age, ended, next_id = identities(succ, pred, n, prev["track_id"], prev["parent_track"], prev["age"],
                                                          next_id)
            for b in range(n):
                if age[b] > 0:
                    velocity[b] = centroid[b] - prev["centroid"][pred[b]]
        prev = dict(labels=labels, cell_ptr=ptr, area=area, centroid=centroid, track_id=np.array(ids, np.int64),
                    parent_track=np.array(parent, np.int64), age=np.array(age, np.int64), velocity=velocity,
                    ended=np.array(ended, np.int64).reshape(-1, 2))
        frames.append(prev)
    return frames
