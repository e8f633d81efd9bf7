#!/usr/bin/env python3
"""How much rain fell?  A sequence of COLMAX planes -> the rain rate of each scan -> the depth of every interval summed
along the echo's motion -> the total over the last half hour, all on the device.

The scans are made from one gridded plane by the advection kernel with a known drift of 9 pixels per scan, so a cell crosses
several pixels between two scans.  Adding up the rate planes scan by scan leaves one deposit per scan (the "fish bone");
the advection-corrected accumulation fills the swath between them, with the same total.  Needs an MI355X and the built library.

    python examples/rain_accumulation_example.py
"""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import torch  # noqa: E402

from radar_processor_amd import (RainAccumulator, RoiSearch, accumulate_device, advect_device, collapse_plane_device,  # noqa: E402
                                 get_field_data, get_gate_coordinates, rain_rate_device, roi_grid_fields_device, synthetic)

INTERVAL_S = 300.0                                          # five minutes between two scans
SCANS = 7
DRIFT = (4.0, -8.0)                                         # (dy, dx) pixels per scan


class Grid:
    grid_shape, grid_limits = (12, 400, 400), ((500.0, 12000.0), (-240e3, 240e3), (-240e3, 240e3))


def main():
    volume = synthetic.make_volume(n_elev=6, n_az=360, n_gates=480, seed=3, fields=("DBZH",))
    radar = volume.as_radar()
    search = RoiSearch(*get_gate_coordinates(radar), Grid.grid_shape, Grid.grid_limits)
    dbz = get_field_data(radar, "DBZH")
    field = torch.from_numpy(np.ascontiguousarray(dbz.filled(np.nan), dtype=np.float32).ravel()).to(search.dev)
    mask = torch.from_numpy(np.ma.getmaskarray(dbz).ravel().astype(np.uint8)).to(search.dev)
    first = collapse_plane_device(roi_grid_fields_device(search, [field], [mask])[0], "colmax").contiguous()
    h, w = (int(v) for v in first.shape)

    # 1. the scans: the first plane drifting by DRIFT per scan (one vector for the whole plane: a lattice of one node).  A
    #    pixel nothing moves into is dry ground here, not missing coverage: 0 dBZ
    drift = torch.tensor([[DRIFT]], dtype=torch.float32, device=first.device)
    scans = advect_device(first, drift, [float(t) for t in range(SCANS)], lattice=(0.0, 0.0, 1.0, 1.0, 1, 1), method="nearest")
    scans = torch.nan_to_num(scans, nan=0.0).contiguous()

    # 2. the rate of one scan: Marshall-Palmer, nothing below 5 dBZ, hail capped at 55 dBZ
    rate = rain_rate_device(scans[0])
    print(f"planes {h} x {w}: {float((rate > 0).float().mean()):.1%} of the first scan is rain, at most {float(rate.max()):.1f} mm/h")

    # 3. the accumulator: one update per scan.  "auto" estimates the motion between successive scans (block match, fill);
    #    steps=None takes the search radius, so a sub-instant moves the echo by at most about a pixel
    moving = RainAccumulator(motion="auto", block=32, stride=16, search=16, window_seconds=1800.0)
    still = RainAccumulator(motion=None, window_seconds=1800.0)
    for t in range(SCANS):
        frame = moving.update(scans[t], t * INTERVAL_S)
        plain = still.update(scans[t], t * INTERVAL_S)
        if frame.interval_mm is None:
            continue
        vectors = frame.motion.motion.reshape(-1, 2)
        print(f"scan {t}: motion {float(vectors[:, 0].median()):+.2f}, {float(vectors[:, 1].median()):+.2f} px per scan; interval "
              f"{float(torch.nan_to_num(frame.interval_mm).sum()):9.1f} mm over the plane along the motion, "
              f"{float(torch.nan_to_num(plain.interval_mm).sum()):9.1f} mm without")

    # 4. the half-hour totals.  Along the motion the swath of a cell is filled; without it the total is a row of deposits.
    #    The roughness ALONG the drift tells them apart: the mean difference between neighbours one scan's drift apart is what
    #    a smooth swath has little of
    total, plain = moving.total(skip_missing=True), still.total(skip_missing=True)
    hy, hx = int(DRIFT[0]) // 2, int(-DRIFT[1]) // 2          # half a drift: 2 rows up, 4 columns to the left

    def roughness(plane):
        return float((plane[hy:, :w - hx] - plane[:h - hy, hx:]).abs().mean())
    print(f"half an hour: {float(total.sum()):.1f} mm over the plane along the motion, {float(plain.sum()):.1f} mm without; "
          f"roughness half a drift apart {roughness(total):.4f} against {roughness(plain):.4f} mm")

    # 5. one interval by hand, with the count of sub-instants that contributed to every pixel
    grid = moving.update(scans[0], SCANS * INTERVAL_S + 7200.0).motion          # a gap: nothing is accumulated, the window empties
    assert grid is None and moving.total() is None
    r0, r1 = rain_rate_device(scans[0]), rain_rate_device(scans[1])
    depth, steps = accumulate_device(r0, r1, drift, INTERVAL_S / 3600.0, steps=9, lattice=(0.0, 0.0, 1.0, 1.0, 1, 1),
                                     min_steps=5, return_steps=True)
    print(f"one interval by hand: {float(torch.isfinite(depth).float().mean()):.1%} of the plane has at least 5 of 9 sub-instants, "
          f"{float((steps == 9).float().mean()):.1%} all 9")


if __name__ == "__main__":
    main()
