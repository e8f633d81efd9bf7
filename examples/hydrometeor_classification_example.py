#!/usr/bin/env python3
"""Hydrometeor classes in the polar domain: phase processing, the temperature along the beam from a sounding, texture and fuzzy
logic on the device, then the classes as a mask for the gridder and as a gridded categorical field.

A synthetic S-band volume stands in for a file: a sector with a rain cell whose core holds hail-like signatures (62 dBZ, ZDR near
0), stratiform echo elsewhere that turns into snow where the beam climbs above the freezing level, and a ring of ground clutter
near the radar (low RHOHV, noisy Z and PHIDP).  Needs an MI355X and the built library.

    python examples/hydrometeor_classification_example.py
"""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import radar_processor_amd as rg  # noqa: E402
from radar_processor_amd import _native, synthetic  # noqa: E402

N_ELEV, N_AZ, N_GATES = 4, 360, 500
GRID_SHAPE, GRID_LIMITS = (8, 250, 250), ((0.0, 7000.0), (-120e3, 120e3), (-120e3, 120e3))
CELL_AZ, CELL_GATES, CORE_GATES, CLUTTER_GATES = (40, 80), (120, 200), (150, 170), 25
SOUNDING_H, SOUNDING_T = [0.0, 3500.0, 12000.0], [22.0, 0.0, -55.0]       # metres above sea level, degrees Celsius


def dual_pol_volume(seed=0):
    """``(phidp, dbz, zdr, rhohv)`` as float32 [n_rays, n_gates], the elevations, the ranges and the gate spacing."""
    elev, az, ranges = synthetic.sweep_geometry(N_ELEV, N_AZ, N_GATES)
    spacing = float(ranges[1] - ranges[0])
    rng = np.random.default_rng(seed)
    n_rays = N_ELEV * N_AZ
    shape = (n_rays, N_GATES)
    in_sector = np.tile((np.arange(N_AZ) >= CELL_AZ[0]) & (np.arange(N_AZ) < CELL_AZ[1]), N_ELEV)
    kdp = np.zeros(shape)
    kdp[in_sector, CELL_GATES[0]:CELL_GATES[1]] = 1.0
    dbz = 22.0 + 20.0 * kdp + rng.normal(0.0, 1.0, shape)
    zdr = 0.3 + 1.0 * kdp + rng.normal(0.0, 0.1, shape)
    dbz[in_sector, CORE_GATES[0]:CORE_GATES[1]] = 62.0 + rng.normal(0.0, 1.0, (int(in_sector.sum()), CORE_GATES[1] - CORE_GATES[0]))
    zdr[in_sector, CORE_GATES[0]:CORE_GATES[1]] = rng.normal(0.1, 0.1, (int(in_sector.sum()), CORE_GATES[1] - CORE_GATES[0]))
    rhohv = np.clip(0.99 - 0.02 * rng.beta(2.0, 8.0, shape), 0.0, 1.0)
    truth = 60.0 + np.cumsum(2.0 * kdp * spacing / 1000.0, axis=1) + rng.normal(0.0, 2.0, shape)
    # ground clutter: the nearest gates of the lowest sweep
    low = slice(0, N_AZ)
    dbz[low, :CLUTTER_GATES] = rng.normal(35.0, 8.0, (N_AZ, CLUTTER_GATES))
    zdr[low, :CLUTTER_GATES] = rng.normal(0.0, 1.5, (N_AZ, CLUTTER_GATES))
    rhohv[low, :CLUTTER_GATES] = rng.uniform(0.55, 0.9, (N_AZ, CLUTTER_GATES))
    truth[low, :CLUTTER_GATES] += rng.normal(0.0, 45.0, (N_AZ, CLUTTER_GATES))
    phidp = (truth - 360.0 * np.floor((truth + 180.0) / 360.0)).astype(np.float32)
    return phidp, dbz.astype(np.float32), zdr.astype(np.float32), rhohv.astype(np.float32), elev, az, ranges, spacing


def main():
    torch = _native.torch_mod()
    dev = _native.device()
    phidp, dbz, zdr, rhohv, elev, az, ranges, spacing = dual_pol_volume()
    phidp_d, dbz_d, zdr_d, rhohv_d = (torch.from_numpy(a).to(dev) for a in (phidp, dbz, zdr, rhohv))

    # 1. a first pass without a mask: textures and classes tell clutter from weather
    first = rg.process_phase_device(phidp_d, dbz_d, spacing, zdr=zdr_d, band="S", half_window=12, min_valid=8)
    temperature = rg.beam_temperature(elev, ranges, SOUNDING_H, SOUNDING_T)                 # float32 [n_sweeps, n_gates]
    hc = rg.classify_hydrometeors_device(first.dbz, first.zdr, first.kdp, rhohv_d, phidp=first.phidp_unfolded, temperature=temperature,
                                         rays_per_sweep=N_AZ)
    table = rg.HYDROMETEOR_TABLE_S_BAND
    counts = torch.bincount(hc.classes.reshape(-1).to(torch.int64), minlength=table.n_classes + 1).cpu().numpy()
    for name, n in zip(("unclassified",) + table.class_names, counts):
        print(f"  {name:>14}: {int(n):7d} gates")
    core = hc.classes[CELL_AZ[0]:CELL_AZ[1], CORE_GATES[0] + 2:CORE_GATES[1] - 2]
    print(f"the core of the cell is {100.0 * float((core == table.class_value('rain and hail')).float().mean()):.0f} % 'rain and hail'; "
          f"the nearest {CLUTTER_GATES} gates of the lowest sweep are "
          f"{100.0 * float((hc.classes[:N_AZ, 2:CLUTTER_GATES - 2] == table.class_value('ground clutter')).float().mean()):.0f} % 'ground clutter'")

    # 2. the classes as a mask: the second pass of the phase processing and the gridder leave clutter and insects out
    not_weather = rg.class_mask_device(hc.classes, table, ("ground clutter", "biological"))
    second = rg.process_phase_device(phidp_d, dbz_d, spacing, zdr=zdr_d, mask=not_weather, band="S", half_window=12, min_valid=8)

    # 3. gridded: reflectivity without clutter, and the classes themselves by the closest gate (a category has no mean)
    gx, gy, gz = synthetic.gate_coordinates(elev, az, ranges)
    search = rg.RoiSearch(gx, gy, gz, GRID_SHAPE, GRID_LIMITS)
    z_grid = rg.roi_grid_fields_device(search, [second.dbz.reshape(-1)], shared_mask=not_weather.reshape(-1))
    unclassified = (hc.classes == 0).to(torch.uint8)
    class_grid = rg.roi_grid_fields_device(search, [hc.classes.float().reshape(-1)], shared_mask=unclassified.reshape(-1), weighting="closest")
    hail = (class_grid[0] == float(table.class_value("rain and hail"))).any(dim=0)
    print(f"gridded: {int(torch.isfinite(z_grid[0]).sum())} voxels of clutter-free reflectivity, "
          f"{int(hail.sum())} columns with 'rain and hail' somewhere in them")


if __name__ == "__main__":
    main()
