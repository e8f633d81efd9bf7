#!/usr/bin/env python3
"""What a dealiased velocity is for: azimuthal shear and radial divergence by local linear least squares (LLSD) on the device,
gridded like any field and collapsed to a column maximum -- a rotation product and a divergence product.

A synthetic volume stands in for a file: a uniform wind, one Rankine vortex (a mesocyclone: solid rotation of 25 m/s at 2 km from
its centre, decaying outside) and one divergent outflow (a downburst), seen by every sweep as the component along the beam,
folded into a Nyquist interval of +-16 m/s, with noise, 2 % of the gates missing and a few wild outliers.  The chain is
dealias -> median filter -> LLSD -> gridder -> column maximum; the largest gridded shear must lie on the vortex and the largest
gridded divergence on the outflow.  Needs an MI355X and the built library.

    python examples/velocity_shear_example.py
"""
import os
import sys
import tempfile

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import radar_processor_amd as rg  # noqa: E402
from radar_processor_amd import _native, synthetic  # noqa: E402

N_ELEV, N_AZ, N_GATES = 4, 360, 600
GRID_SHAPE, GRID_LIMITS = (6, 300, 300), ((0.0, 6000.0), (-150e3, 150e3), (-150e3, 150e3))
NYQUIST = 16.0
VORTEX = dict(x=40e3, y=55e3, core=2000.0, speed=25.0)          # metres east and north of the radar
OUTFLOW = dict(x=-60e3, y=20e3, core=3000.0, speed=18.0)


def _rankine(d, core, speed):
    return np.where(d < core, speed * d / core, speed * core / np.maximum(d, 1e-9))


def volume(seed=0):
    """``(folded, truth, ranges, ray_spacing_deg, gate_spacing_m)``: float32 [n_sweeps, n_rays, n_gates] and the tables."""
    rng = np.random.default_rng(seed)
    elev, az_deg, ranges = synthetic.sweep_geometry(N_ELEV, N_AZ, N_GATES)
    az = np.deg2rad(az_deg)
    bx, by = np.sin(az)[:, None], np.cos(az)[:, None]            # the beam's unit vector (east, north)
    x, y = ranges[None, :] * bx, ranges[None, :] * by
    u, v = np.full_like(x, 6.0), np.full_like(x, -3.0)            # the environment's wind
    dx, dy = x - VORTEX["x"], y - VORTEX["y"]
    d = np.hypot(dx, dy)
    speed = _rankine(d, VORTEX["core"], VORTEX["speed"])
    u, v = u - speed * dy / np.maximum(d, 1e-9), v + speed * dx / np.maximum(d, 1e-9)      # counter-clockwise
    dx, dy = x - OUTFLOW["x"], y - OUTFLOW["y"]
    d = np.hypot(dx, dy)
    speed = _rankine(d, OUTFLOW["core"], OUTFLOW["speed"])
    u, v = u + speed * dx / np.maximum(d, 1e-9), v + speed * dy / np.maximum(d, 1e-9)      # outwards
    truth = np.broadcast_to((u * bx + v * by)[None], (N_ELEV, N_AZ, N_GATES))
    noisy = truth + rng.normal(0.0, 0.5, truth.shape)
    folded = (noisy - 2.0 * NYQUIST * np.floor((noisy + NYQUIST) / (2.0 * NYQUIST))).astype(np.float32)
    wild = rng.random(folded.shape) < 0.002
    folded[wild] = rng.uniform(-NYQUIST, NYQUIST, int(wild.sum())).astype(np.float32)
    folded[rng.random(folded.shape) < 0.02] = np.nan
    return folded, truth.astype(np.float32), ranges, 360.0 / N_AZ, float(ranges[1] - ranges[0]), (elev, az_deg)


def main():
    torch = _native.torch_mod()
    dev = _native.device()
    folded, truth, ranges, ray_deg, gate_m, (elev, az_deg) = volume()
    vel = torch.from_numpy(folded).to(dev)

    # 1. dealias (two host synchronisations by nature), then the window tables from the sweep's geometry (host, float64)
    d = rg.dealias_velocity_device(vel, NYQUIST, n_bands=3, wrap_rays=True)
    window = rg.llsd_window(ranges, ray_deg, gate_m)
    print(f"dealiased: {d.n_regions} regions, folds {int(d.folds.min())} .. {int(d.folds.max())}; window: {2 * window.half_gates + 1} gates "
          f"by {2 * int(window.half_rays.min()) + 1} .. {2 * int(window.half_rays.max()) + 1} rays")

    # 2. the chain: a 3 x 3 median takes the outliers out, the LLSD fits a plane per gate.  No host synchronisation.
    s = rg.azimuthal_shear_device(d.velocity, window, median=(1, 1), want=("azimuthal_shear", "radial_divergence", "velocity", "count"))
    fitted = ~torch.isnan(s.azimuthal_shear)
    print(f"LLSD: a fit at {int(fitted.sum())} of {fitted.numel()} gates, windows of up to {int(s.count.to(torch.int32).max())} gates; azimuthal shear "
          f"{float(s.azimuthal_shear[fitted].min()):+.4f} .. {float(s.azimuthal_shear[fitted].max()):+.4f} 1/s, divergence "
          f"{float(s.radial_divergence[fitted].min()):+.4f} .. {float(s.radial_divergence[fitted].max()):+.4f} 1/s")
    # the two calls by hand give the same bits
    filtered = rg.median_filter_device(d.velocity, half_rays=1, half_gates=1)
    again = rg.velocity_shear_device(filtered, window)
    assert torch.equal(again.azimuthal_shear.view(torch.int32), s.azimuthal_shear.view(torch.int32))

    # 3. shear.reshape(-1) is a gridder field like any other; the column maximum is the rotation product
    gate_x, gate_y, gate_z = synthetic.gate_coordinates(elev, az_deg, ranges)
    with tempfile.TemporaryDirectory() as tmp:
        geometry = rg.compute_grid_geometry(gate_x, gate_y, gate_z, GRID_SHAPE, GRID_LIMITS, temp_dir=tmp, toa=17000.0)
    # close to the radar a uniform wind V has an azimuthal derivative of its own, V / r: leave the first 15 km out
    far = torch.from_numpy(ranges >= 15e3).to(dev)[None, None, :]
    mask = (~(fitted & far)).reshape(-1).to(torch.uint8)
    grids = rg.grid_fields_device(geometry, [s.azimuthal_shear.reshape(-1), s.radial_divergence.reshape(-1)], shared_mask=mask)
    shear_grid, div_grid = (g.cpu().numpy() if hasattr(g, "cpu") else np.asarray(g) for g in grids)
    xs = np.linspace(GRID_LIMITS[2][0], GRID_LIMITS[2][1], GRID_SHAPE[2])
    ys = np.linspace(GRID_LIMITS[1][0], GRID_LIMITS[1][1], GRID_SHAPE[1])
    for name, grid, target in (("azimuthal shear", shear_grid, VORTEX), ("radial divergence", div_grid, OUTFLOW)):
        colmax = rg.column_max(grid.reshape(GRID_SHAPE))
        iy, ix = np.unravel_index(np.nanargmax(colmax), colmax.shape)
        off = float(np.hypot(xs[ix] - target["x"], ys[iy] - target["y"]))
        expected = target["speed"] / target["core"]             # solid rotation / uniform spreading inside the core
        print(f"column maximum of the gridded {name}: {np.nanmax(colmax):+.4f} 1/s at ({xs[ix] / 1e3:+.1f}, {ys[iy] / 1e3:+.1f}) km, "
              f"{off / 1e3:.1f} km from the centre put there ({target['x'] / 1e3:+.1f}, {target['y'] / 1e3:+.1f}); the core's own "
              f"{name} is {expected:+.4f} 1/s")
        assert off < 5000.0, f"the largest gridded {name} is not where the feature is"


if __name__ == "__main__":
    main()
