#!/usr/bin/env python3
"""Where is the echo going?  Two successive COLMAX planes -> the motion field between them -> the plane 5 to 30 minutes
ahead, all on the device.

The second plane is made from the first by the advection kernel itself with a known rotation about the radar plus a
drift, so the estimated vectors can be compared with the truth.  The usual way is to copy both planes to the host and run
an optical-flow package; here neither plane leaves the GPU.  Needs an MI355X and the built library.

    python examples/nowcast_example.py
"""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import torch  # noqa: E402

from radar_processor_amd import (RoiSearch, advect_device, collapse_plane_device, estimate_motion_device,  # noqa: E402
                                 fill_motion_device, get_field_data, get_gate_coordinates, motion_to_velocity, nowcast_device,
                                 roi_grid_fields_device, synthetic)

INTERVAL_S = 300.0                                          # five minutes between the two planes


class Grid:
    grid_shape, grid_limits = (12, 400, 400), ((500.0, 12000.0), (-240e3, 240e3), (-240e3, 240e3))


def main():
    volume = synthetic.make_volume(n_elev=6, n_az=360, n_gates=480, seed=3, fields=("DBZH",))
    radar = volume.as_radar()
    search = RoiSearch(*get_gate_coordinates(radar), Grid.grid_shape, Grid.grid_limits)
    dbz = get_field_data(radar, "DBZH")
    field = torch.from_numpy(np.ascontiguousarray(dbz.filled(np.nan), dtype=np.float32).ravel()).to(search.dev)
    mask = torch.from_numpy(np.ma.getmaskarray(dbz).ravel().astype(np.uint8)).to(search.dev)
    prev = collapse_plane_device(roi_grid_fields_device(search, [field], [mask])[0], "colmax").contiguous()
    h, w = (int(v) for v in prev.shape)

    # 1. a second plane with known motion: a slow rotation about the centre plus a drift to the north-east, one vector per
    #    pixel as (dy, dx) in pixels per interval -- the advection takes a dense field as it takes a block lattice
    yy, xx = torch.meshgrid(torch.arange(h, device=prev.device, dtype=torch.float32),
                            torch.arange(w, device=prev.device, dtype=torch.float32), indexing="ij")
    truth = torch.stack([0.02 * (xx - w / 2) + 2.0, -0.02 * (yy - h / 2) + 3.0], dim=-1).contiguous()
    nxt = advect_device(prev, truth, [1.0], method="bilinear", substeps=4)[0]

    # 2. the motion between the two planes: one vector per 32 x 32 block every 16 pixels, searched within +-16 pixels
    grid = estimate_motion_device(prev, nxt, block=32, stride=16, search=16)
    found = ~torch.isnan(grid.score)
    print(f"planes {h} x {w}: {tuple(grid.score.shape)} blocks, {int(found.sum())} with a vector, "
          f"median correlation {float(grid.score[found].median()):.3f}")
    filled = fill_motion_device(grid, min_score=0.5)
    lat = filled.lattice
    ny_, nx_ = torch.meshgrid(torch.arange(lat.ny, device=prev.device), torch.arange(lat.nx, device=prev.device), indexing="ij")
    at_nodes = truth[(lat.origin_y + ny_ * lat.step_y).round().long(), (lat.origin_x + nx_ * lat.step_x).round().long()]
    err = (grid.motion - at_nodes).abs().amax(dim=-1)[found]
    print(f"vectors against the truth at the block centres: median error {float(err.median()):.2f} px, "
          f"90 % below {float(err.quantile(0.9)):.2f} px")
    u, v = motion_to_velocity(filled, Grid, INTERVAL_S)
    print(f"mean motion {float(np.mean(u)):+.1f} m/s east, {float(np.mean(v)):+.1f} m/s north "
          f"(a pixel is {480e3 / (w - 1):.0f} m, the interval {INTERVAL_S:.0f} s)")

    # 3. the nowcast: the second plane 5, 10, 15 and 30 minutes ahead.  nowcast_device chains steps 2 and 3
    leads = [1.0, 2.0, 3.0, 6.0]
    forecast = advect_device(nxt, filled, leads, method="nearest", substeps=4)
    again, _ = nowcast_device(prev, nxt, leads, block=32, stride=16, search=16, substeps=4)
    assert torch.equal(forecast.isnan(), again.isnan()) and torch.equal(forecast.nan_to_num(), again.nan_to_num())
    for k, lead in enumerate(leads):
        target = advect_device(nxt, truth, [lead], method="nearest", substeps=8)[0]       # the same plane along the true field
        both = torch.isfinite(target) & torch.isfinite(forecast[k])
        mae = float((forecast[k][both] - target[both]).abs().mean())
        still = torch.isfinite(target) & torch.isfinite(nxt)
        persistence = float((nxt[still] - target[still]).abs().mean())
        print(f"+{lead * INTERVAL_S / 60:4.0f} min: mean |nowcast - truth| {mae:5.2f} dBZ, persistence {persistence:5.2f} dBZ, "
              f"{float(torch.isfinite(forecast[k]).float().mean()):.1%} of the plane filled")


if __name__ == "__main__":
    main()
