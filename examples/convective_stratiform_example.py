#!/usr/bin/env python3
"""Which rain is convective?  A gridded volume -> the CAPPI of the work level -> the background reflectivity, the convective
centres and the convective / stratiform classes after Steiner, Houze and Yuter 1995 -> a rain rate with one Z-R relation per
class, all on the device.  Needs an MI355X and the built library.

    python examples/convective_stratiform_example.py
"""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import torch  # noqa: E402

from radar_processor_amd import (RainAccumulator, RoiSearch, classify_grid, convective_stratiform_device, disk_footprint,  # noqa: E402
                                 echo_background_device, get_field_data, get_gate_coordinates, rain_rate_by_class_device,
                                 rain_rate_device, roi_grid_fields_device, synthetic)


class Grid:
    grid_shape, grid_limits = (12, 400, 400), ((500.0, 12000.0), (-240e3, 240e3), (-240e3, 240e3))


def main():
    volume = synthetic.make_volume(n_elev=6, n_az=360, n_gates=480, seed=3, fields=("DBZH",))
    radar = volume.as_radar()
    search = RoiSearch(*get_gate_coordinates(radar), Grid.grid_shape, Grid.grid_limits)
    dbz = get_field_data(radar, "DBZH")
    field = torch.from_numpy(np.ascontiguousarray(dbz.filled(np.nan), dtype=np.float32).ravel()).to(search.dev)
    mask = torch.from_numpy(np.ma.getmaskarray(dbz).ravel().astype(np.uint8)).to(search.dev)
    grid = roi_grid_fields_device(search, [field], [mask])[0]
    spacing = 480e3 / 399                                    # metres per pixel of this grid: 1203 m

    # 1. the classification of the 3 km CAPPI in one call; the spacing comes from the geometry.  The background disk of
    #    11 km is a footprint of half-widths per row distance, made on the host
    hw = disk_footprint(11000.0, spacing, spacing)
    print(f"the 11 km disk at {spacing:.0f} m pixels: {2 * (len(hw) - 1) + 1} rows, half-widths {hw}")
    parts = classify_grid(grid, Grid, altitude=3000.0, return_parts=True)
    classes = parts.classes
    echo = float((classes > 0).float().mean())
    print(f"3 km CAPPI: {echo:.1%} echo, of which {float((classes == 2).sum()) / max(float((classes > 0).sum()), 1.0):.1%} convective; "
          f"{int((parts.centres > 0).sum())} centres in radius classes "
          f"{torch.bincount(parts.centres.flatten().long(), minlength=6)[1:].tolist()}")

    # 2. the background reflectivity as a product of its own: the mean LINEAR reflectivity within 11 km, in dBZ
    plane = torch.where(classes > 0, parts.background, torch.full_like(parts.background, float("nan")))
    print(f"background over the echo: {float(torch.nanmean(plane)):.1f} dBZ on average, at most {float(parts.background.nan_to_num(-99).max()):.1f}")
    from radar_processor_amd import constant_altitude_ppi
    cappi = constant_altitude_ppi(grid, Grid, 3000.0).contiguous()
    wide, count = echo_background_device(cappi, dx=spacing, radius=30000.0, return_counts=True)
    print(f"a 30 km background: defined on {float(torch.isfinite(wide).float().mean()):.1%} of the plane, up to {int(count.max())} echo pixels per disk")

    # 3. another relation: a lower intensity threshold and larger convective radii
    loose = convective_stratiform_device(cappi, dx=spacing, intense=35.0, area_relation="large")
    print(f"intense=35 dBZ with the 'large' radii: {int((loose == 2).sum())} convective pixels against {int((classes == 2).sum())}")

    # 4. one Z-R relation per class: Marshall-Palmer for the stratiform rain, Z = 300 R^1.4 for the cores
    one = rain_rate_device(cappi)
    two = rain_rate_by_class_device(cappi, classes)
    core = classes == 2
    if bool(core.any()):
        print(f"over the convective pixels: {float(one[core].mean()):.1f} mm/h under Marshall-Palmer, {float(two[core].mean()):.1f} mm/h by class")

    # 5. the accumulator classifies every scan when it is given a convective relation
    accumulator = RainAccumulator(motion=None, convective_zr=(300.0, 1.4), classify=dict(dx=spacing))
    accumulator.update(cappi, 0.0)
    frame = accumulator.update(cappi, 300.0)
    print(f"five minutes of this scan: {float(torch.nan_to_num(frame.interval_mm).sum()):.1f} mm over the plane")


if __name__ == "__main__":
    main()
