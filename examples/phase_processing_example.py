#!/usr/bin/env python3
"""Differential phase before the gridder: unfold PHIDP, estimate KDP, correct Z and ZDR for attenuation on the device, then
grid the corrected reflectivity next to the uncorrected one and look at the COLMAX behind a convective cell.

A synthetic C-band volume stands in for a file: along every ray of a sector a cell with KDP = 3 deg/km removes dB from
everything behind it (``A_H = alpha * KDP``); PHIDP starts at a system offset of 100 degrees, carries 3 degrees of noise and
folds at +-180.  The fields are built ray by ray like the test rays of tests/phase_scenes.py.  Needs an MI355X and the built
library.

    python examples/phase_processing_example.py
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
CELL_AZ, CELL_GATES, CELL_KDP = (40, 80), (120, 170), 3.0          # a sector of 40 rays, gates 120 .. 169


def dual_pol_volume(seed=0):
    """``(phidp, dbz, zdr, rhohv, dbz_true)`` as float32 [n_rays, n_gates], and the gate spacing in metres."""
    elev, az, ranges = synthetic.sweep_geometry(N_ELEV, N_AZ, N_GATES)
    spacing = float(ranges[1] - ranges[0])
    rng = np.random.default_rng(seed)
    n_rays = N_ELEV * N_AZ
    in_sector = np.tile((np.arange(N_AZ) >= CELL_AZ[0]) & (np.arange(N_AZ) < CELL_AZ[1]), N_ELEV)
    kdp = np.zeros((n_rays, N_GATES))
    kdp[in_sector, CELL_GATES[0]:CELL_GATES[1]] = CELL_KDP
    path = np.cumsum(2.0 * kdp * spacing / 1000.0, axis=1)                       # two-way degrees gained along the ray
    truth = 100.0 + path + rng.normal(0.0, 3.0, path.shape)
    phidp = (truth - 360.0 * np.floor((truth + 180.0) / 360.0)).astype(np.float32)
    dbz_true = 25.0 + 8.0 * kdp + rng.normal(0.0, 1.0, path.shape)
    alpha, beta = rg.ATTENUATION_COEFFICIENTS["C"]
    dbz = (dbz_true - alpha * path).astype(np.float32)
    zdr = (0.5 + 0.5 * kdp - beta * path + rng.normal(0.0, 0.1, path.shape)).astype(np.float32)
    rhohv = np.clip(0.985 - 0.25 * rng.beta(2.0, 8.0, path.shape), 0.0, 1.0).astype(np.float32)
    rhohv[rng.random(path.shape) < 0.03] = 0.5                                   # speckle the unfolding must not see
    phidp[rhohv < 0.8] += np.float32(170.0)                                      # ... because its phase means nothing
    return phidp, dbz, zdr, rhohv, dbz_true.astype(np.float32), spacing


def main():
    torch = _native.torch_mod()
    dev = _native.device()
    phidp, dbz, zdr, rhohv, dbz_true, spacing = dual_pol_volume()
    phidp_d, dbz_d, zdr_d, rhohv_d = (torch.from_numpy(a).to(dev) for a in (phidp, dbz, zdr, rhohv))

    # 1. QC in the polar domain: leave the gates of low RHOHV out of the unfolding (and, below, of the gridding)
    mask = rg.device_gate_mask(rhohv_d.reshape(-1), "below", 0.8).reshape(rhohv_d.shape)
    print(f"{int(mask.sum())} of {mask.numel()} gates masked for RHOHV < 0.8")

    # 2. the chain: three launches, nothing returns to the host
    products = rg.process_phase_device(phidp_d, dbz_d, spacing, zdr=zdr_d, mask=mask, band="C", half_window=12, min_valid=8)
    sector = slice(CELL_AZ[0], CELL_AZ[1])
    core = slice(CELL_GATES[0] + 12, CELL_GATES[1] - 12)
    print(f"KDP in the core: {float(products.kdp[sector, core].nanmean()):.2f} deg/km (true {CELL_KDP}); "
          f"PHIDP gained at the end of those rays: {float(products.dphi[sector, -1].mean()):.1f} degrees "
          f"(true {2.0 * CELL_KDP * (CELL_GATES[1] - CELL_GATES[0]) * spacing / 1000.0:.1f})")
    behind = slice(CELL_GATES[1] + 20, N_GATES)
    true_d = torch.from_numpy(dbz_true).to(dev)
    for name, field in (("uncorrected", dbz_d), ("corrected", products.dbz)):
        print(f"  {name:>11} Z behind the cell: {float((field - true_d)[sector, behind].mean()):+.2f} dB against the truth")

    # 3. the outputs, flattened, are what the gridders take
    elev, az, ranges = synthetic.sweep_geometry(N_ELEV, N_AZ, N_GATES)
    gate_x, gate_y, gate_z = synthetic.gate_coordinates(elev, az, ranges)
    with tempfile.TemporaryDirectory() as tmp:
        geometry = rg.compute_grid_geometry(gate_x, gate_y, gate_z, GRID_SHAPE, GRID_LIMITS, temp_dir=tmp, toa=17000.0)
    grids = rg.grid_fields_device(geometry, [products.dbz.reshape(-1), dbz_d.reshape(-1)], shared_mask=mask.reshape(-1))
    colmax_corrected, colmax_raw = rg.column_max(grids[0]), rg.column_max(grids[1])
    difference = (colmax_corrected - colmax_raw).cpu().numpy() if hasattr(colmax_raw, "cpu") else colmax_corrected - colmax_raw
    ny, nx = difference.shape
    y = np.linspace(GRID_LIMITS[1][0], GRID_LIMITS[1][1], ny)[:, None]
    x = np.linspace(GRID_LIMITS[2][0], GRID_LIMITS[2][1], nx)[None, :]
    azimuth = np.degrees(np.arctan2(x, y)) % 360.0
    shadow = (azimuth >= CELL_AZ[0] + 2) & (azimuth < CELL_AZ[1] - 2) & (np.hypot(x, y) > ranges[CELL_GATES[1] + 20])
    elsewhere = (azimuth >= 180.0) & (azimuth < 300.0)
    print(f"COLMAX corrected - uncorrected: {np.nanmean(difference[shadow]):+.2f} dB behind the cell, "
          f"{np.nanmean(difference[elsewhere]):+.2f} dB in the sector without one")


if __name__ == "__main__":
    main()
