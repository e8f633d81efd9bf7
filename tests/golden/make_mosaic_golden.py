#!/usr/bin/env python3
"""Generate the multi-radar mosaic fixtures tests/golden/g10_mosaic_{barnes2,cressman,nearest}.npz with the REFERENCE's own
modules (see make_golden.py, whose loader and meta blob this script reuses).

The reference grids one radar per geometry; the mosaic contract pins against it radar by radar: radar r's rows are the
reference's ``compute_grid_geometry`` on the shared limits shifted by the radar's origin (``mosaic_limits``) with
``toa - oz``, and the mosaic grid is the reference's ``apply_geometry`` on the row-wise concatenation of those CSRs (a
reference ``GridGeometry`` with the shared limits) applied to the concatenated masked fields.

    python tests/golden/make_mosaic_golden.py
"""
from __future__ import annotations

import os
import sys
import tempfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
from make_golden import REPO, load_reference, meta_blob  # noqa: E402

sys.path.insert(0, REPO)

FIELDS = ("DBZH", "RHOHV")
QC = ("RHOHV", 0.8)
QC_RADAR = 1
# three small radars about 80-90 km apart; (oz, oy, ox) in the grid frame, the second one on a hill
VOLUMES = [dict(n_elev=5, n_az=120, n_gates=160, seed=21, max_range_m=80e3),
           dict(n_elev=5, n_az=120, n_gates=160, seed=22, max_range_m=80e3),
           dict(n_elev=5, n_az=120, n_gates=160, seed=23, max_range_m=80e3)]
ORIGINS = [(0.0, 0.0, 0.0), (800.0, 10e3, 85e3), (250.0, 75e3, 35e3)]
GRID_SHAPE = (6, 28, 36)
GRID_LIMITS = ((0.0, 10000.0), (-25e3, 29e3), (10e3, 80e3))       # 2 km columns, 2 km levels
TOA = 9000.0
FILL = -9999.0


def mosaic_limits(grid_limits, origin):
    return tuple((lo - o, hi - o) for (lo, hi), o in zip(grid_limits, origin))


def concat_rows(csrs, offsets):
    """Row v of the result: radar 0's row v, then radar 1's, ... (gate numbers shifted by the radar's offset)."""
    counts = [np.diff(ip.astype(np.int64)) for ip, _, _ in csrs]
    total = np.sum(counts, axis=0)
    indptr = np.concatenate([[0], np.cumsum(total)]).astype(np.int64)
    n = int(indptr[-1])
    idx = np.empty(n, dtype=np.int32)
    w = np.empty(n, dtype=np.float32)
    base = indptr[:-1].copy()
    for r, (ip, gi, wt) in enumerate(csrs):
        ip = ip.astype(np.int64)
        rows = np.repeat(np.arange(len(ip) - 1), counts[r])
        dest = base[rows] + (np.arange(len(gi)) - ip[rows])
        idx[dest] = gi.astype(np.int64) + offsets[r]
        w[dest] = wt
        base += counts[r]
    return indptr.astype(np.int32), idx, w


def main():
    ref = load_reference()
    from radar_processor_amd import synthetic
    vols = [synthetic.make_volume(fields=FIELDS, **v) for v in VOLUMES]
    offsets = np.concatenate([[0], np.cumsum([v.n_total_gates for v in vols])]).astype(np.int64)
    radars = [v.as_radar() for v in vols]
    # concatenated masked fields; the QC filter folded into its radar's mask
    masked = {}
    for name in FIELDS:
        data, mask = [], []
        for r, radar in enumerate(radars):
            f = ref.utils.get_field_data(radar, name)
            m = np.ma.getmaskarray(f).ravel().copy()
            if r == QC_RADAR:
                gf = ref.filters.GateFilter(radar)
                gf.exclude_below(*QC)
                m |= gf.gate_excluded.ravel()
            data.append(np.ma.getdata(f).ravel())
            mask.append(m)
        masked[name] = np.ma.array(np.concatenate(data), mask=np.concatenate(mask))
    for weighting in ("barnes2", "cressman", "nearest"):
        out = {}
        csrs = []
        for r, (vol, origin) in enumerate(zip(vols, ORIGINS)):
            with tempfile.TemporaryDirectory() as tmp:
                g = ref.compute.compute_grid_geometry(
                    vol.gate_x, vol.gate_y, vol.gate_z, GRID_SHAPE, mosaic_limits(GRID_LIMITS, origin), tmp,
                    radar_altitude=0.0, min_radius=250.0, beam_factor=0.01746, weighting=weighting, toa=TOA - origin[0],
                    n_workers=1)
            csrs.append((g.indptr, g.gate_indices, g.weights))
            out[f"r{r}_indptr"], out[f"r{r}_gate_indices"], out[f"r{r}_weights"] = g.indptr, g.gate_indices, g.weights
        ip, idx, w = concat_rows(csrs, offsets)
        geom = ref.geometry.GridGeometry(GRID_SHAPE, GRID_LIMITS, ip, idx, w, TOA)
        for name in FIELDS:
            out[f"grid_{name}"] = ref.interpolate.apply_geometry(geom, masked[name])
            out[f"grid_{name}_fill"] = ref.interpolate.apply_geometry(geom, masked[name], fill_value=FILL)
        reached = np.sum([np.diff(c[0].astype(np.int64)) > 0 for c in csrs], axis=0)
        assert set(np.unique(reached)) == {0, 1, 2, 3}, np.unique(reached)
        out["meta"] = meta_blob(case="G10", volumes=VOLUMES, digests=[v.digest() for v in vols],
                                origins=[list(o) for o in ORIGINS], grid_shape=GRID_SHAPE, grid_limits=GRID_LIMITS,
                                toa=TOA, weighting=weighting, min_radius=250.0, beam_factor=0.01746, fields=list(FIELDS),
                                qc=[QC[0], QC[1]], qc_radar=QC_RADAR, fill_value=FILL)
        path = os.path.join(HERE, f"g10_mosaic_{weighting}.npz")
        np.savez_compressed(path, **out)
        print(weighting, int(ip[-1]), "pairs;", "voxels reached by 0/1/2/3 radars:",
              [int((reached == k).sum()) for k in range(4)], f"{os.path.getsize(path) / 1e3:.0f} kB")


if __name__ == "__main__":
    main()
