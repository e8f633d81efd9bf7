#!/usr/bin/env python3
"""Generate the mosaic-section fixtures tests/golden/g12_mosaic_section_{barnes2,cressman,nearest}.npz with the REFERENCE's
own modules (see make_golden.py and make_section_golden.py, whose loader and meta blob this script reuses).

The reference grids one radar per geometry and has no joint mean.  Its level worker ``compute._process_single_level`` is
run per radar and level at that radar's points -- ``float64(y_r)``, ``float64(x_r)``, ``zc_r[k]`` in the radar's frame, the
toa mask ``gate_z <= toa - oz`` -- the levels are stacked into that radar's CSR of ``nz * n_points`` rows, and the radars'
rows are concatenated (radar 0's row, then radar 1's, ..., gate numbers shifted by the radar's offset).  The section
values are the reference's ``apply_geometry`` on a reference ``GridGeometry((nz, 1, n_points), ...)`` with that joint CSR
over the concatenated fields.  The scene is tests/mosaic_section_scenes.py (mosaic_scenes.scene16 and its dog-leg).

    python tests/golden/make_mosaic_section_golden.py
"""
from __future__ import annotations

import os
import sys
import tempfile
import types

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
from make_golden import REPO, load_reference, meta_blob  # noqa: E402

sys.path.insert(0, REPO)
sys.path.insert(0, os.path.join(REPO, "tests"))
import mosaic_scenes as ms  # noqa: E402
import mosaic_section_scenes as mss  # noqa: E402


def radar_csr(ref, s, r, xs, ys, weighting):
    """The reference's rows of radar r's part of the section, level by level (its own in-row order)."""
    v = s.vols[r]
    n_rows = s.shape[0] * len(xs)
    if len(v.gate_x) == 0:
        return np.zeros(n_rows + 1, dtype=np.int64), np.zeros(0, dtype=np.int32), np.zeros(0, dtype=np.float32)
    z_rel = v.gate_z - 0.0                                          # compute.py:182 (radar_altitude = 0)
    valid = z_rel <= s.toa - s.origins[r][0]                        # compute.py:193 with the radar's toa - oz
    x_r, y_r = mss.radar_points(s, r, xs, ys)
    gy, gx = y_r.astype(np.float64), x_r.astype(np.float64)
    ips, idxs, ws = [], [], []
    with tempfile.TemporaryDirectory() as tmp:
        for k, z in enumerate(mss.levels(s, r)):
            _, _, path = ref.compute._process_single_level(
                (k, z, gy, gx, v.gate_x, v.gate_y, z_rel, valid, s.min_radius, s.beam_factor, weighting, tmp))
            with np.load(path) as lvl:
                ips.append(lvl["indptr"].astype(np.int64))
                idxs.append(lvl["gate_indices"])
                ws.append(lvl["weights"])
    offsets = np.concatenate([[0], np.cumsum([ip[-1] for ip in ips])])
    indptr = np.concatenate([[0]] + [ip[1:] + off for ip, off in zip(ips, offsets)]).astype(np.int64)
    return indptr, np.concatenate(idxs).astype(np.int32), np.concatenate(ws).astype(np.float32)


def main():
    ref = load_reference()
    s = ms.scene16()
    xs, ys, dist = mss.path()
    n, nz = len(xs), s.shape[0]
    n_total = int(s.offsets()[-1])
    # the concatenated radars as one duck-typed radar (what radar_grid/filters.py:40-52, 91-102 touch)
    fields = {}
    for name in ms.FIELDS:
        data, mask = mss.concat_field(s, name)
        fields[name] = np.ma.array(data, mask=mask)
    radar = types.SimpleNamespace(nrays=n_total, ngates=1, fields={k: {"data": f.reshape(n_total, 1)} for k, f in fields.items()})
    gf = ref.filters.GateFilter(radar)
    gf.exclude_below(*mss.QC)
    s_last = float(np.hypot(np.diff(xs.astype(np.float64)), np.diff(ys.astype(np.float64))).sum())
    shared_idx = None
    for weighting in mss.WEIGHTINGS:
        ip, idx, w = ms.concat_rows([radar_csr(ref, s, r, xs, ys, weighting) for r in range(s.n_radars)], s.offsets())
        lengths = np.diff(ip)
        out = dict(xs=xs, ys=ys, s=dist, indptr=ip.astype(np.int32), weights=w)
        if weighting == "barnes2":
            out["gate_indices"] = shared_idx = idx
        else:                                                  # the neighbour sets do not depend on the weighting
            assert np.array_equal(idx, shared_idx)
        geom = ref.geometry.GridGeometry((nz, 1, n), (s.limits[0], (0.0, 0.0), (0.0, s_last)), ip.astype(np.int32), idx, w,
                                         s.toa)
        A = ref.interpolate.apply_geometry
        for fname in mss.FIELDS:
            f = fields[fname]
            out[f"grid_{fname}"] = A(geom, f)
            out[f"grid_{fname}_qc"] = A(geom, f, additional_filters=[gf])
            out[f"grid_{fname}_qc_fill"] = A(geom, f, additional_filters=[gf], fill_value=mss.FILL)
        report = dict(points=n, pairs=int(ip[-1]), empty=round(float((lengths == 0).mean()), 4), longest=int(lengths.max()))
        out["meta"] = meta_blob(case="G12", scene="scene16", digests=[v.digest() for v in s.vols],
                                origins=[list(o) for o in s.origins], fields=list(mss.FIELDS), qc=list(mss.QC), nz=nz,
                                z_limits=list(s.limits[0]), toa=s.toa, weighting=weighting, min_radius=s.min_radius,
                                beam_factor=s.beam_factor, fill_value=mss.FILL,
                                vertices=[list(v) for v in mss.VERTICES], spacing=mss.SPACING, report=report)
        path = os.path.join(HERE, f"g12_mosaic_section_{weighting}.npz")
        np.savez_compressed(path, **out)
        print(weighting, report, f"{os.path.getsize(path) / 1e3:.0f} kB")
        assert os.path.getsize(path) < 1_000_000


if __name__ == "__main__":
    main()
