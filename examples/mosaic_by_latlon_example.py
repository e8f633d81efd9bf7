#!/usr/bin/env python3
"""Two radars 200 km apart on one grid, placed by longitude and latitude.

Each radar's gate coordinates lie in the azimuthal-equidistant plane tangent at its own antenna; ``place_radars`` re-projects
them into the plane of the grid (on the device) and returns the tuples every mosaic function takes.  The example grids the
pair both ways -- placed, and merely translated as the mosaic functions alone would do -- and prints how far apart the two
put the second radar's gates.  Synthetic volumes stand in for ``pyart.io.read(...)``.  Needs an MI355X and the built library.

    python examples/mosaic_by_latlon_example.py
"""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import torch  # noqa: E402

from radar_processor_amd import (MosaicSearch, geographic_to_grid, get_field_data, get_gate_coordinates,  # noqa: E402
                                 grid_lonlat_device, grid_to_geographic, mosaic_fields_device,
                                 mosaic_section_fields_device, place_radars, section_path_lonlat, synthetic)


def main():
    origin = (-64.19, -31.44, 400.0)                                  # lon, lat, altitude of the grid's tangent point
    east = grid_to_geographic(2.0e5, 0.0, origin[0], origin[1])       # the point 200 km east of it
    radars = []
    for seed, (lon, lat, alt) in enumerate([origin, (float(east[0]), float(east[1]), 520.0)]):
        radar = synthetic.make_volume(n_elev=4, n_az=180, n_gates=240, seed=seed, fields=("DBZH",)).as_radar()
        radar.longitude["data"][0], radar.latitude["data"][0], radar.altitude["data"][0] = lon, lat, alt
        radars.append(radar)

    # 1. the tuples: (x', y', gate_z, (oz, oy, ox)) per radar; x', y' are device tensors
    placed = place_radars(radars, origin)
    for k, (x, y, _, o) in enumerate(placed):
        gx, gy, _ = get_gate_coordinates(radars[k])
        moved = np.hypot(x.cpu().numpy() - gx, y.cpu().numpy() - gy)
        print(f"radar {k}: antenna at x {o[2] / 1e3:8.3f} km, y {o[1] / 1e3:8.3f} km, {o[0]:5.1f} m above the origin; "
              f"re-projection moves its gates by up to {moved.max():7.1f} m")

    # 2. one grid over both radars, straight from the gates
    shape = (8, 200, 300)
    limits = ((1000.0, 8000.0), (-200e3, 200e3), (-200e3, 400e3))
    search = MosaicSearch(placed, shape, limits)
    fields = [[torch.from_numpy(get_field_data(r, "DBZH").filled(np.nan)).to(search.dev)] for r in radars]
    grid = mosaic_fields_device(search, fields)[0]
    print(f"mosaic: {tuple(grid.shape)}, {float(torch.isfinite(grid).float().mean()):.1%} filled")

    # ... against translation alone (what the tuples were before): where both grids hold a value, how different it is
    translated = [get_gate_coordinates(r) + (o,) for r, (_, _, _, o) in zip(radars, placed)]
    grid_t = mosaic_fields_device(MosaicSearch(translated, shape, limits), fields)[0]
    both = torch.isfinite(grid) & torch.isfinite(grid_t)
    print(f"translated instead: values differ by up to {float((grid - grid_t)[both].abs().max()):.1f} dBZ")

    # 3. georeferencing the product: longitude / latitude of every column
    lon, lat = grid_lonlat_device(shape, limits, origin)
    print(f"grid corners: ({float(lon[0, 0]):.3f}, {float(lat[0, 0]):.3f}) .. ({float(lon[-1, -1]):.3f}, {float(lat[-1, -1]):.3f})")

    # 4. a section between two geographic points (straight in the grid's plane, not a geodesic)
    xs, ys, s = section_path_lonlat([(-64.0, -31.0), (-62.3, -31.8)], 1000.0, origin)
    section = mosaic_section_fields_device(search, xs, ys, fields)[0]
    x_end, y_end = geographic_to_grid(-62.3, -31.8, origin[0], origin[1])
    print(f"section: {tuple(section.shape)} over {s[-1] / 1e3:.0f} km, ending near x {float(x_end) / 1e3:.1f} km, "
          f"y {float(y_end) / 1e3:.1f} km")


if __name__ == "__main__":
    main()
