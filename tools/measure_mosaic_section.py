#!/usr/bin/env python3
"""A vertical section through a mosaic next to the single-radar sections it replaces, same process, same search structures,
alternating launches:

    python tools/measure_mosaic_section.py [--points 2000] [--launches 25] [--weighting barnes2] [--out profiles/mosaic_section_timing.json]

Three bench-size radars (12 x 360 x 1000 gates each, the origins of tools/profile_mosaic.py and INTEGRATION.md's mosaic
figures) on the 40 x 2000 x 2000 grid, one ``MosaicSearch``; ``--points`` points x 40 levels, one field, along

  ``through``   the diagonal x - y = -10 km, which passes through radar 0's antenna (rows of thousands of gates there) and
                through the reach of the other two;
  ``miss``      80 km of the grid's bottom edge (y = -239.5 km, x from 160 km on): 249 km and more from every antenna, beyond
                every gate and outside every radar's window rectangle: every point is dead for every radar, the one
                launch visits nobody, and the single-radar route has nothing to launch (its time is reported as null).

Per path and launch pair:

  (a) ``mosaic``   ONE rg_roi_section_mosaic_f32 launch over the three-entry table (the points NaN-marked per radar by
                   mosaic_section_points);
  (b) ``singles``  rg_roi_section_f32 once per radar that has a point of the path, on that radar's search at its points with
                   the NaN ones removed -- what a caller had before, short of joining the three results (which needs the
                   weight sums the single-radar entry point does not return).

Both are KERNEL times: the fields are packed once, outside the timed region, and stream events bracket the launches; (a)
and (b) alternate, the first ``--warmup`` pairs are dropped, the median of the rest is reported.  One JSON object on stdout
and in ``--out``."""
import argparse
import ctypes
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

ORIGINS = [(0.0, -80e3, -90e3), (300.0, 10e3, 110e3), (600.0, 130e3, -30e3)]
PATHS = {"through": ((-239e3, -229e3), (229e3, 239e3)), "miss": ((160e3, -239.5e3), (239.5e3, -239.5e3))}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--points", type=int, default=2000)
    ap.add_argument("--launches", type=int, default=25)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--weighting", default="barnes2")
    ap.add_argument("--out", default="")
    args = ap.parse_args()
    import torch
    import radar_processor_amd as rg
    from radar_processor_amd import _native, synthetic
    lib = rg.load_library()
    dev = torch.device("cuda", 0)
    cfg = synthetic.CONFIGS["METRIC"]
    shape, limits = cfg["grid_shape"], cfg["grid_limits"]
    vols = [synthetic.make_volume(cfg["n_elev"], cfg["n_az"], cfg["n_gates"], seed=60 + r, fields=("DBZH",)) for r in range(3)]
    radars = [(v.gate_x, v.gate_y, v.gate_z, o) for v, o in zip(vols, ORIGINS)]
    ms = rg.MosaicSearch(radars, shape, limits, device=dev)
    nz = shape[0]
    w = _native.WEIGHTINGS[args.weighting]
    stream = _native.stream_ptr()
    counts = ms.n_gates
    offsets = np.concatenate([[0], np.cumsum(counts)])
    n_total = int(offsets[-1])
    # the packed fields: all radars end to end for the mosaic (each radar's part is also what a single-radar call reads)
    f_t = torch.cat([torch.from_numpy(np.ascontiguousarray(np.ma.getdata(v.fields["DBZH"]))).to(dev) for v in vols])
    m_t = torch.cat([torch.from_numpy(np.ma.getmaskarray(v.fields["DBZH"]).astype(np.uint8)).to(dev) for v in vols])
    packed = torch.empty(n_total, dtype=torch.float32, device=dev)
    fptrs, mptrs = (ctypes.c_void_p * 1)(_native.ptr(f_t)), (ctypes.c_void_p * 1)(_native.ptr(m_t))
    _native.check(lib.rg_pack_fields_f32(1, fptrs, mptrs, None, n_total, 1, _native.ptr(packed), stream), "pack")
    rec = {"volume": [cfg["n_elev"], cfg["n_az"], cfg["n_gates"]], "radars": 3, "origins": ORIGINS, "grid_shape": list(shape),
           "windows": [list(wn) for wn in ms.windows], "levels": nz, "weighting": args.weighting, "launches": args.launches,
           "warmup": args.warmup, "device": torch.cuda.get_device_name(0),
           "unit": "ms; stream events around the kernel launch(es), median over the launches after the warm-up", "paths": {}}
    for name, (a, b) in PATHS.items():
        length = float(np.hypot(b[0] - a[0], b[1] - a[1]))
        xs, ys, s = rg.section_path([a, b], length / (args.points - 1) * (1 - 1e-12))
        n = len(xs)
        pts = rg.mosaic_section_points(ms, xs, ys)
        live = [~np.isnan(x) for x, _ in pts]
        dev_pts = [None if not live[r].any() else (torch.from_numpy(pts[r][0]).to(dev), torch.from_numpy(pts[r][1]).to(dev))
                   for r in range(3)]
        table = ms.section_table([0, 1, 2], offsets[:-1], dev_pts)
        out_m = torch.empty((1, nz, n), dtype=torch.float32, device=dev)
        # the single-radar calls: per radar its live points and an output of its own
        singles = []
        for r in range(3):
            if not live[r].any():
                continue
            sr = ms.searches[r]
            x_t = torch.from_numpy(np.ascontiguousarray(pts[r][0][live[r]])).to(dev)
            y_t = torch.from_numpy(np.ascontiguousarray(pts[r][1][live[r]])).to(dev)
            singles.append((r, sr, x_t, y_t, torch.empty((1, nz, int(live[r].sum())), dtype=torch.float32, device=dev)))

        def mosaic():
            _native.check(lib.rg_roi_section_mosaic_f32(table, 3, nz, n, ms.min_radius, ms.beam_factor, w, _native.ptr(packed),
                                                        1, 1, n_total, float("nan"), _native.ptr(out_m), stream),
                          "rg_roi_section_mosaic_f32")

        def single_radars():
            for r, sr, x_t, y_t, out in singles:
                _native.check(lib.rg_roi_section_f32(
                    _native.ptr(sr.sorted_gates), _native.ptr(sr.cell_start), sr.cells, _native.ptr(x_t), _native.ptr(y_t),
                    _native.ptr(sr.zc), nz, int(x_t.numel()), sr.min_radius, sr.beam_factor, w,
                    _native.ptr(packed) + 4 * int(offsets[r]), 1, 1, float("nan"), _native.ptr(out), stream), "rg_roi_section_f32")

        runs = {"mosaic": mosaic, "singles": single_radars}
        times = {k: [] for k in runs}
        for i in range(args.warmup + args.launches):
            for key in (("mosaic", "singles") if i % 2 == 0 else ("singles", "mosaic")):
                if key == "singles" and not singles:
                    continue
                torch.cuda.synchronize()
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                runs[key]()
                e1.record()
                e1.synchronize()
                if i >= args.warmup:
                    times[key].append(e0.elapsed_time(e1))
        # the timed launch against the public route
        public = rg.mosaic_section_fields_device(ms, xs, ys, [[f_t[offsets[r]:offsets[r + 1]]] for r in range(3)],
                                                 shared_masks=[m_t[offsets[r]:offsets[r + 1]] for r in range(3)],
                                                 weighting=args.weighting)
        same = bool(torch.equal(public.view(torch.int32), out_m.view(torch.int32)))
        times = {k: v for k, v in times.items() if v}
        med = {k: round(float(np.median(v)), 4) for k, v in times.items()}
        med.setdefault("singles", None)
        rec["paths"][name] = {
            "vertices": [list(a), list(b)], "points": n, "path_length_m": float(s[-1]),
            "live_points_per_radar": [int(l.sum()) for l in live], "single_radar_launches": len(singles),
            "median_ms": med, "min_ms": {k: round(float(np.min(v)), 4) for k, v in times.items()},
            "max_ms": {k: round(float(np.max(v)), 4) for k, v in times.items()},
            "mosaic_vs_singles": round(med["mosaic"] / med["singles"], 3) if singles else None,
            "filled_fraction": round(float(torch.isfinite(out_m).float().mean().item()), 4),
            "same_bits_as_mosaic_section_fields_device": same}
        assert same
    print(json.dumps(rec))
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as fh:
            json.dump(rec, fh, indent=1)
    return 0


if __name__ == "__main__":
    sys.exit(main())
