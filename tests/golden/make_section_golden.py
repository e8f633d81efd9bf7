#!/usr/bin/env python3
"""Generate the vertical-section fixtures tests/golden/g11_section_{barnes2,cressman,nearest}.npz with the REFERENCE's own
modules (see make_golden.py, whose loader and meta blob this script reuses).

The reference grids lattices; its level worker ``compute._process_single_level`` takes flat arrays of x and y for one z
and does not care whether they form one.  A section is pinned against it point by point: for every level k the worker is
called with the path's points (``float64(ys)``, ``float64(xs)``, ``zc[k]``, the toa mask ``gate_z - radar_altitude <= toa``)
and the levels are stacked into one CSR of ``nz * n_points`` rows; the section values are the reference's
``apply_geometry`` on a reference ``GridGeometry((nz, 1, n_points), ...)`` with that CSR.  The scene (volume, paths,
levels) is tests/section_scenes.py.

    python tests/golden/make_section_golden.py
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
sys.path.insert(0, os.path.join(REPO, "tests"))
import section_scenes as sc  # noqa: E402


def section_csr(ref, vol, xs, ys, zc, weighting):
    """The reference's rows of the section, level by level (its own in-row order: KD-tree traversal)."""
    z_rel = vol.gate_z - 0.0                                  # compute.py:182 (radar_altitude = 0)
    valid = z_rel <= sc.TOA                                   # compute.py:193
    gy, gx = ys.astype(np.float64), xs.astype(np.float64)
    ips, idxs, ws = [], [], []
    with tempfile.TemporaryDirectory() as tmp:
        for k, z in enumerate(zc):
            _, _, path = ref.compute._process_single_level(
                (k, z, gy, gx, vol.gate_x, vol.gate_y, z_rel, valid, sc.MIN_RADIUS, sc.BEAM_FACTOR, weighting, tmp))
            with np.load(path) as lvl:
                ips.append(lvl["indptr"].astype(np.int64))
                idxs.append(lvl["gate_indices"])
                ws.append(lvl["weights"])
    offsets = np.concatenate([[0], np.cumsum([ip[-1] for ip in ips])])
    indptr = np.concatenate([[0]] + [ip[1:] + off for ip, off in zip(ips, offsets)]).astype(np.int32)
    return indptr, np.concatenate(idxs).astype(np.int32), np.concatenate(ws).astype(np.float32)


def main():
    ref = load_reference()
    import radar_processor_amd as rg
    vol = sc.volume()
    radar = vol.as_radar()
    gf = ref.filters.GateFilter(radar)
    gf.exclude_below(*sc.QC)
    zc = sc.levels()
    shared_idx = {}
    for weighting in sc.WEIGHTINGS:
        out, report = {}, {}
        for name, (vertices, spacing) in sc.PATHS.items():
            xs, ys, s = rg.section_path(vertices, spacing)
            n = len(xs)
            ip, idx, w = section_csr(ref, vol, xs, ys, zc, weighting)
            lengths = np.diff(ip.astype(np.int64))
            empty = float((lengths == 0).mean())
            assert 1.0 - empty >= 0.5 and empty > 0.0 and (name != "dogleg" or lengths.max() > 1000), \
                (name, empty, int(lengths.max()))
            out[f"{name}_xs"], out[f"{name}_ys"], out[f"{name}_s"] = xs, ys, s
            out[f"{name}_indptr"], out[f"{name}_weights"] = ip, w
            if weighting == "barnes2":
                out[f"{name}_gate_indices"] = shared_idx[name] = idx
            else:                                              # the neighbour sets do not depend on the weighting
                assert np.array_equal(idx, shared_idx[name])
            s_last = float(np.hypot(np.diff(xs.astype(np.float64)), np.diff(ys.astype(np.float64))).sum())
            geom = ref.geometry.GridGeometry((sc.NZ, 1, n), (sc.Z_LIMITS, (0.0, 0.0), (0.0, s_last)), ip, idx, w, sc.TOA)
            for fname in sc.FIELDS:
                f = ref.utils.get_field_data(radar, fname)
                f = np.ma.array(np.ma.getdata(f), mask=np.ma.getmaskarray(f))     # a full-array mask
                A = ref.interpolate.apply_geometry
                out[f"{name}_grid_{fname}"] = A(geom, f)
                out[f"{name}_grid_{fname}_qc"] = A(geom, f, additional_filters=[gf])
                out[f"{name}_grid_{fname}_qc_fill"] = A(geom, f, additional_filters=[gf], fill_value=sc.FILL)
            report[name] = dict(points=n, pairs=int(ip[-1]), empty=round(empty, 4), longest=int(lengths.max()))
        assert max(r["longest"] for r in report.values()) > 1000
        out["meta"] = meta_blob(case="G11", volume=sc.VOLUME, digest=vol.digest(), fields=list(sc.FIELDS), qc=list(sc.QC),
                                nz=sc.NZ, z_limits=list(sc.Z_LIMITS), toa=sc.TOA, weighting=weighting,
                                min_radius=sc.MIN_RADIUS, beam_factor=sc.BEAM_FACTOR, fill_value=sc.FILL,
                                paths={k: dict(vertices=[list(v) for v in vs], spacing=sp)
                                       for k, (vs, sp) in sc.PATHS.items()}, report=report)
        path = os.path.join(HERE, f"g11_section_{weighting}.npz")
        np.savez_compressed(path, **out)
        print(weighting, report, f"{os.path.getsize(path) / 1e3:.0f} kB")
        assert os.path.getsize(path) < 1_000_000


if __name__ == "__main__":
    main()
