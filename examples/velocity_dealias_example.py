#!/usr/bin/env python3
"""Doppler velocity before the gridder: dealias a folded volume by regions on the device, then grid the dealiased velocity next
to the folded one and look at the fold line.

A synthetic volume stands in for a file: a wind of 24 m/s that every sweep sees as ``speed * cos(azimuth - direction)``, folded
into a Nyquist interval of +-10 m/s, with 3 % of the gates missing.  Across the fold line the gridder's weighted mean of the
folded field averages +10 with -10 m/s into a calm that is not there; the dealiased field has no such line.  Needs an MI355X and
the built library.

    python examples/velocity_dealias_example.py
"""
import os
import sys
import tempfile

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import radar_processor_amd as rg  # noqa: E402
from radar_processor_amd import _native, synthetic  # noqa: E402

N_ELEV, N_AZ, N_GATES = 4, 360, 500
GRID_SHAPE, GRID_LIMITS = (8, 250, 250), ((0.0, 7000.0), (-240e3, 240e3), (-240e3, 240e3))
NYQUIST, SPEED, DIRECTION = 10.0, 24.0, 0.7


def folded_volume(seed=0):
    """``(vel, truth)`` as float32 [n_sweeps, n_rays, n_gates]: the folded velocity and the wind it came from."""
    rng = np.random.default_rng(seed)
    az = 2.0 * np.pi * np.arange(N_AZ) / N_AZ
    truth = SPEED * np.cos(az - DIRECTION)[None, :, None] * np.linspace(0.6, 1.0, N_GATES)[None, None, :] * np.ones((N_ELEV, 1, 1))
    vel = (truth - 2.0 * NYQUIST * np.floor((truth + NYQUIST) / (2.0 * NYQUIST))).astype(np.float32)
    vel[rng.random(vel.shape) < 0.03] = np.nan
    return vel, truth.astype(np.float32)


def main():
    torch = _native.torch_mod()
    dev = _native.device()
    vel, truth = folded_volume()
    vel_d = torch.from_numpy(vel).to(dev)

    # 1. the chain: split into bands, label, edge table, host merge, apply.  Two host synchronisations by nature.
    d = rg.dealias_velocity_device(vel_d, NYQUIST, n_bands=3, wrap_rays=True)
    valid = ~torch.isnan(d.velocity)
    error = (d.velocity - torch.from_numpy(truth).to(dev))[valid].abs().max()
    print(f"{d.n_regions} regions, {d.n_edges} edges; folds {int(d.folds.min())} .. {int(d.folds.max())}; "
          f"largest error against the wind at {int(valid.sum())} valid gates: {float(error):.2e} m/s")

    # 2. the pieces, for a caller that wants to look inside
    regions = rg.velocity_regions_device(vel_d, NYQUIST, n_bands=3)
    edges = rg.region_edges_device(vel_d, regions.regions, wrap_rows=True)
    print(f"the strongest border joins regions {edges.pairs[edges.count.argmax()].tolist()} over {int(edges.count.max())} gate pairs")

    # 3. velocity.reshape(-1) is a gridder field like any other
    elev, az, ranges = synthetic.sweep_geometry(N_ELEV, N_AZ, N_GATES)
    gate_x, gate_y, gate_z = synthetic.gate_coordinates(elev, az, ranges)
    with tempfile.TemporaryDirectory() as tmp:
        geometry = rg.compute_grid_geometry(gate_x, gate_y, gate_z, GRID_SHAPE, GRID_LIMITS, temp_dir=tmp, toa=17000.0)
    mask = torch.isnan(vel_d).reshape(-1).to(torch.uint8)
    grids = rg.grid_fields_device(geometry, [d.velocity.reshape(-1), vel_d.reshape(-1)], shared_mask=mask)
    level = 1
    dealiased, folded = (g[level].cpu().numpy() if hasattr(g, "cpu") else np.asarray(g)[level] for g in grids)
    print(f"gridded level {level}: |v| reaches {np.nanmax(np.abs(dealiased)):.1f} m/s dealiased, {np.nanmax(np.abs(folded)):.1f} m/s folded "
          f"(Nyquist {NYQUIST}); the largest step between neighbouring voxels is {np.nanmax(np.abs(np.diff(dealiased, axis=1))):.1f} "
          f"against {np.nanmax(np.abs(np.diff(folded, axis=1))):.1f} m/s across the fold line")


if __name__ == "__main__":
    main()
