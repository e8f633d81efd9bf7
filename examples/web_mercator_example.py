#!/usr/bin/env python3
"""A gridded volume onto a web map: COLMAX of a synthetic volume, warped north-up into Web Mercator with its overview
pyramid, and into the pixels of one XYZ map tile -- all on the device.

The reference re-projects with ``gdalwarp`` and builds the overviews with rasterio after the image has left the GPU;
``web_mercator_rgba`` does both where the plane already lies.  What comes back is what a COG writer or a tile server needs:
the RGBA image, its overviews, and the raster's bounds / geotransform.  Needs an MI355X and the built library.

    python examples/web_mercator_example.py
"""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import torch  # noqa: E402

from radar_processor_amd import (RoiSearch, collapse_plane_device, colormap_lut, colormap_rgba_device,  # noqa: E402
                                 get_field_data, get_gate_coordinates, lonlat_to_mercator, mercator_raster_for,
                                 mercator_tile, mercator_to_lonlat, overview_pyramid_device, roi_grid_fields_device, synthetic,
                                 warp_to_mercator_device, web_mercator_rgba)


def main():
    origin = (-64.19, -31.44, 476.0)                                  # lon, lat, altitude of the radar = the grid's tangent point
    radar = synthetic.make_volume(n_elev=6, n_az=360, n_gates=480, seed=3, fields=("DBZH",)).as_radar()
    shape, limits = (12, 400, 400), ((500.0, 12000.0), (-240e3, 240e3), (-240e3, 240e3))

    # 1. gates -> grid -> COLMAX, on the device
    gx, gy, gz = get_gate_coordinates(radar)
    search = RoiSearch(gx, gy, gz, shape, limits)
    dbz = get_field_data(radar, "DBZH")
    field = torch.from_numpy(np.ascontiguousarray(dbz.filled(np.nan), dtype=np.float32).ravel()).to(search.dev)
    mask = torch.from_numpy(np.ma.getmaskarray(dbz).ravel().astype(np.uint8)).to(search.dev)
    grid = roi_grid_fields_device(search, [field], [mask])[0]
    colmax = collapse_plane_device(grid, "colmax")
    print(f"COLMAX: {tuple(colmax.shape)}, {float(torch.isfinite(colmax).float().mean()):.1%} echo")

    # 2. the raster that covers the grid, the warped image and its overviews
    lut = colormap_lut(np.stack([np.linspace(0.1, 1.0, 64), np.linspace(0.9, 0.1, 64), np.full(64, 0.3), np.ones(64)], axis=1))
    raster, rgba, overviews = web_mercator_rgba(colmax, limits, origin, lut, vmin=-10.0, vmax=60.0)
    west, south, east, north = raster.bounds
    (lon_w, lon_e), (lat_s, lat_n) = mercator_to_lonlat([west, east], [south, north])
    print(f"raster: {raster.width} x {raster.height} pixels of {raster.pixel:.1f} m; lon {lon_w:.3f} .. {lon_e:.3f}, "
          f"lat {lat_s:.3f} .. {lat_n:.3f}; geotransform {tuple(round(v, 1) for v in raster.transform)}")
    print(f"image: {tuple(rgba.shape)} uint8, {float((rgba[..., 3] > 0).float().mean()):.1%} opaque; overviews "
          f"{[tuple(t.shape[:2]) for t in overviews]}")

    # ... the same with bilinear sampling and averaged overviews (the float plane is averaged, each level coloured afterwards)
    _, smooth, smooth_levels = web_mercator_rgba(colmax, limits, origin, lut, vmin=-10.0, vmax=60.0, method="bilinear",
                                                 resampling="average")
    print(f"bilinear + average: {float((smooth[..., 3] > 0).float().mean()):.1%} opaque, smallest level "
          f"{tuple(smooth_levels[-1].shape[:2])}")

    # 3. the pieces on their own: float planes stay float until they are coloured
    same = mercator_raster_for(shape, limits, origin)
    assert same == raster
    warped = warp_to_mercator_device(colmax, limits, origin, raster)
    assert torch.equal(colormap_rgba_device(warped, lut, -10.0, 60.0), rgba)
    levels = overview_pyramid_device(warped, [2, 4], resampling="average")
    print(f"float overviews: {[tuple(t.shape) for t in levels]}, "
          f"mean of the finite pixels {float(warped[torch.isfinite(warped)].mean()):.2f} dBZ at full size, "
          f"{float(levels[1][torch.isfinite(levels[1])].mean()):.2f} dBZ at 1/4")

    # 4. straight into one XYZ tile: zoom 8, the tile over the radar
    x, y = (float(v) for v in lonlat_to_mercator(origin[0], origin[1]))
    world = 2.0 * np.pi * 6378137.0
    tile = mercator_tile(8, int((x / world + 0.5) * 256), int((0.5 - y / world) * 256))
    tile_rgba = colormap_rgba_device(warp_to_mercator_device(colmax, limits, origin, tile), lut, -10.0, 60.0)
    print(f"tile 8/{int((x / world + 0.5) * 256)}/{int((0.5 - y / world) * 256)}: {tuple(tile_rgba.shape)}, "
          f"{float((tile_rgba[..., 3] > 0).float().mean()):.1%} opaque, pixel {tile.pixel:.1f} m")


if __name__ == "__main__":
    main()
