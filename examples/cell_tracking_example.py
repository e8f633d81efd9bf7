#!/usr/bin/env python3
"""Follow storm cells over three synthetic frames, all on the device: cells at or above 35 dBZ keep their track id while they
move, one cell splits in two, one is born.

Every frame is labelled on the GPU; the motion between two frames is estimated by block matching, the earlier frame's labels
are moved along it, and a per-pixel pass counts the pixels every pair (old cell, new cell) shares.  Only that table of a few
pairs and the cell table come back to the host, where the identities are settled.  Needs an MI355X and the built library.

    python examples/cell_tracking_example.py
"""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from radar_processor_amd import CellTracker  # noqa: E402

SHAPE = (200, 300)
MOTION = (3, -5)                                  # pixels per frame: northwards and westwards


def disc(plane, cy, cx, r):
    yy, xx = np.mgrid[0:plane.shape[0], 0:plane.shape[1]]
    d2 = ((yy - cy) ** 2 + (xx - cx) ** 2) / float(r * r)
    np.maximum(plane, np.where(d2 <= 1.0, 36.0 + 16.0 * (1.0 - d2), 10.0), out=plane)


def frame(t):
    plane = np.full(SHAPE, 10.0)
    oy, ox = t * MOTION[0], t * MOTION[1]
    disc(plane, 60 + oy, 220 + ox, 14)                                    # a cell that only moves
    disc(plane, 130 + oy, 150 + ox, 12)                                   # a cell whose eastern part ...
    disc(plane, 130 + oy, 150 + ox + (14 if t < 2 else 30), 9)            # ... splits off in the third frame
    if t >= 1:
        disc(plane, 40 + oy, 80 + ox, 8)                                  # born in the second frame
    return plane.astype(np.float32)


def main():
    tracker = CellTracker(35.0, min_size=4)
    for t in range(3):
        f = tracker.update(frame(t))
        area = f.table.area.cpu().numpy()
        centroid = f.table.sum_yx.cpu().numpy() / area[:, None]
        moved = "" if f.motion is None else "  (mean motion %+.1f, %+.1f px)" % tuple(f.motion.motion.mean(dim=(0, 1)).tolist())
        print(f"frame {t}: {len(area)} cells{moved}")
        print("  track parent  age   area   centroid y, x     velocity dy, dx [px / frame]")
        for k in range(len(area)):
            v = "      new" if f.age[k] == 0 else f"{f.velocity[k, 0]:+6.2f} {f.velocity[k, 1]:+6.2f}"
            print(f"  {f.track_id[k]:5d} {f.parent_track[k]:6d} {f.age[k]:4d} {area[k]:6d}   {centroid[k, 0]:7.1f} {centroid[k, 1]:7.1f}"
                  f"     {v}")
        for track, into in f.ended:
            print(f"  track {track} ended" + (f", merged into track {into}" if into else ""))
        ids = f.track_plane_device()
        print(f"  track plane: {int((ids > 0).sum())} pixels carry a track id, the largest is {int(ids.max())}")


if __name__ == "__main__":
    main()
