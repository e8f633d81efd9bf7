#!/usr/bin/env python3
"""Despeckle a COLMAX plane and list its storm cells, all on the device: COLMAX of a synthetic volume -> echo regions of
fewer than 10 pixels removed -> the connected regions at or above 35 dBZ with area, centroid and peak.

The usual way is a round trip to the host and ``scipy.ndimage.label``; here the plane never leaves the GPU until the table of
a few dozen rows is read.  The second part despeckles one sweep in gate space (the azimuth axis wraps) and feeds the mask to
the gridder.  Needs an MI355X and the built library.

    python examples/storm_cells_example.py
"""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import torch  # noqa: E402

from radar_processor_amd import (RoiSearch, collapse_plane_device, despeckle_device, get_field_data,  # noqa: E402
                                 get_gate_coordinates, identify_cells, roi_grid_fields_device, synthetic)


class Grid:
    grid_shape, grid_limits = (12, 400, 400), ((500.0, 12000.0), (-240e3, 240e3), (-240e3, 240e3))


def main():
    volume = synthetic.make_volume(n_elev=6, n_az=360, n_gates=480, seed=3, fields=("DBZH",))
    radar = volume.as_radar()
    gx, gy, gz = get_gate_coordinates(radar)
    search = RoiSearch(gx, gy, gz, Grid.grid_shape, Grid.grid_limits)
    dbz = get_field_data(radar, "DBZH")
    field = torch.from_numpy(np.ascontiguousarray(dbz.filled(np.nan), dtype=np.float32).ravel()).to(search.dev)
    mask = torch.from_numpy(np.ma.getmaskarray(dbz).ravel().astype(np.uint8)).to(search.dev)

    # 1. gates -> grid -> COLMAX -> despeckle: echo regions (>= 5 dBZ) of fewer than 10 pixels become NaN
    colmax = collapse_plane_device(roi_grid_fields_device(search, [field], [mask])[0], "colmax")
    clean, removed = despeckle_device(colmax, 5.0, 10, return_mask=True)
    print(f"COLMAX {tuple(colmax.shape)}: {float(torch.isfinite(colmax).float().mean()):.1%} echo, "
          f"{int(removed.sum())} pixels in regions below 10 pixels removed")

    # 2. the storm cells: regions at or above 35 dBZ of at least 4 pixels
    cells = identify_cells(clean.cpu().numpy(), Grid, 35.0, min_size=4)
    print(f"{len(cells['id'])} cells >= 35 dBZ")
    print("  id   area  km2      centroid x, y [km]      peak dBZ at x, y [km]")
    for i in np.argsort(-cells["area"])[:12]:
        print(f"{cells['id'][i]:4d} {cells['area'][i]:6d} {cells['area_km2'][i]:7.1f}   {cells['centroid_x'][i] / 1e3:8.1f} "
              f"{cells['centroid_y'][i] / 1e3:8.1f}      {cells['vmax'][i]:5.1f}  {cells['peak_x'][i] / 1e3:8.1f} "
              f"{cells['peak_y'][i] / 1e3:8.1f}")

    # 3. gate space: the lowest sweep [n_rays, n_gates], rows wrap in azimuth; the mask goes into the gridder
    sweep = field.view(volume.n_sweeps, volume.n_az, volume.n_gates)[0]
    sweep_mask = mask.view(volume.n_sweeps, volume.n_az, volume.n_gates)[0]
    _, speckle = despeckle_device(sweep, 5.0, 10, mask=sweep_mask, wrap_rows=True, return_mask=True)
    gate_mask = mask.clone()
    gate_mask.view(volume.n_sweeps, volume.n_az, volume.n_gates)[0] |= speckle
    regridded = roi_grid_fields_device(search, [field], [gate_mask])[0]
    print(f"lowest sweep: {int(speckle.sum())} gates in regions below 10 gates masked; the grid has "
          f"{int(torch.isfinite(regridded).sum())} filled voxels")


if __name__ == "__main__":
    main()
