#!/usr/bin/env python3
"""The mosaic combine rules next to the joint mean and next to what they replace, one fresh process per call:

    python tools/measure_mosaic_combine.py [--label new] [--launches 7] [--points 2000] [--weighting barnes2]

Three bench-size radars (12 x 360 x 1000 gates each, the origins of tools/profile_mosaic.py and INTEGRATION.md's mosaic
figures) on the 40 x 2000 x 2000 grid, one ``MosaicSearch``, one field; then the ``through`` path of
tools/measure_mosaic_section.py (``--points`` points x 40 levels).  Per workload, KERNEL times (the fields are packed once,
outside the timed region; stream events bracket the launches; the variants alternate; the first ``--warmup`` rounds are
dropped; median, min and max of the rest):

  ``mean_old``        the joint mean through rg_roi_grid_mosaic_f32 / rg_roi_section_mosaic_f32
  ``mean_new``        the same through the combine entry point with RG_COMBINE_MEAN (the same kernel instantiation)
  ``max``, ``nearest_radar``, and ``max_with_radar``: the one-launch rules, the last with the provenance output
  ``per_radar_max`` / ``per_radar_nearest``: the alternative -- one mean launch per radar into a grid of its own, then a
                      torch fold over the stored grids (``torch.fmax``; for the nearest radar ``torch.where`` on precomputed
                      float32 D grids, which are not timed)

The script also runs on a checkout that has no combine entry points (the parent commit): it then times ``mean_old`` alone.
One JSON object on stdout: alternate processes of the two commits and collect the lines."""
import argparse
import ctypes
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

ORIGINS = [(0.0, -80e3, -90e3), (300.0, 10e3, 110e3), (600.0, 130e3, -30e3)]
THROUGH = ((-239e3, -229e3), (229e3, 239e3))


def alternate(runs, launches, warmup, torch):
    times = {k: [] for k in runs}
    keys = list(runs)
    for i in range(warmup + launches):
        for key in (keys if i % 2 == 0 else keys[::-1]):
            torch.cuda.synchronize()
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            runs[key]()
            e1.record()
            e1.synchronize()
            if i >= warmup:
                times[key].append(e0.elapsed_time(e1))
    return {k: {"median_ms": round(float(np.median(v)), 4), "min_ms": round(float(np.min(v)), 4),
                "max_ms": round(float(np.max(v)), 4)} for k, v in times.items()}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--label", default="new")
    ap.add_argument("--launches", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--points", type=int, default=2000)
    ap.add_argument("--weighting", default="barnes2")
    ap.add_argument("--small", action="store_true", help="a 6 x 120 x 120 grid and small volumes: a rehearsal, not a measurement")
    args = ap.parse_args()
    import torch
    import radar_processor_amd as rg
    from radar_processor_amd import _native, synthetic
    lib = rg.load_library()
    dev = torch.device("cuda", 0)
    cfg = dict(synthetic.CONFIGS["METRIC"])
    if args.small:
        cfg.update(n_elev=4, n_az=90, n_gates=200, grid_shape=(6, 120, 120))
    shape, limits = cfg["grid_shape"], cfg["grid_limits"]
    vols = [synthetic.make_volume(cfg["n_elev"], cfg["n_az"], cfg["n_gates"], seed=60 + r, fields=("DBZH",)) for r in range(3)]
    radars = [(v.gate_x, v.gate_y, v.gate_z, o) for v, o in zip(vols, ORIGINS)]
    ms = rg.MosaicSearch(radars, shape, limits, device=dev)
    nz, ny, nx = shape
    n_vox = nz * ny * nx
    w = _native.WEIGHTINGS[args.weighting]
    stream = _native.stream_ptr()
    counts = ms.n_gates
    offsets = np.concatenate([[0], np.cumsum(counts)])
    n_total = int(offsets[-1])
    f_t = torch.cat([torch.from_numpy(np.ascontiguousarray(np.ma.getdata(v.fields["DBZH"]))).to(dev) for v in vols])
    m_t = torch.cat([torch.from_numpy(np.ma.getmaskarray(v.fields["DBZH"]).astype(np.uint8)).to(dev) for v in vols])
    packed = torch.empty(n_total, dtype=torch.float32, device=dev)
    fptrs, mptrs = (ctypes.c_void_p * 1)(_native.ptr(f_t)), (ctypes.c_void_p * 1)(_native.ptr(m_t))
    _native.check(lib.rg_pack_fields_f32(1, fptrs, mptrs, None, n_total, 1, _native.ptr(packed), stream), "pack")
    combines = getattr(_native, "COMBINES", None)
    nan = float("nan")
    rec = {"label": args.label, "has_combine": combines is not None, "volume": [cfg["n_elev"], cfg["n_az"], cfg["n_gates"]],
           "radars": 3, "grid_shape": list(shape), "weighting": args.weighting, "launches": args.launches,
           "warmup": args.warmup, "device": torch.cuda.get_device_name(0), "fields": 1,
           "unit": "ms; stream events around the kernel launch(es) (and the torch fold of the per_radar_* variants)"}

    # ---- the lattice ------------------------------------------------------------------------------------------------------------
    table = ms.table([0, 1, 2], offsets[:-1])
    singles = [ms.table([r], [int(offsets[r])]) for r in range(3)]
    out = torch.empty((1, n_vox), dtype=torch.float32, device=dev)
    head = (table, 3, nz, ny, nx, ms.min_radius, ms.beam_factor, w, _native.ptr(packed), 1, 1, n_total, nan, _native.ptr(out))
    runs = {"mean_old": lambda: _native.check(lib.rg_roi_grid_mosaic_f32(*head, stream), "mean_old")}
    if combines:
        who = torch.empty((1, n_vox), dtype=torch.uint8, device=dev)
        grids = [torch.empty((1, n_vox), dtype=torch.float32, device=dev) for _ in range(3)]
        d32 = []
        for r in range(3):                       # D of every voxel in radar r's frame: static per geometry, not timed
            lim = rg.mosaic_limits(limits, ORIGINS[r])
            zc, yc, xc = (torch.from_numpy(np.linspace(lim[a][0], lim[a][1], shape[a], dtype="float32")).to(dev) for a in range(3))
            d32.append((zc[:, None, None] ** 2 + yc[None, :, None] ** 2 + xc[None, None, :] ** 2).reshape(1, n_vox))

        def combine(code, radar_map=None):
            return lambda: _native.check(lib.rg_roi_grid_mosaic_combine_f32(*head, code, _native.ptr(radar_map), stream), "combine")

        def per_radar():
            for r in range(3):
                _native.check(lib.rg_roi_grid_mosaic_f32(singles[r], 1, nz, ny, nx, ms.min_radius, ms.beam_factor, w,
                                                         _native.ptr(packed), 1, 1, n_total, nan, _native.ptr(grids[r]), stream),
                              "per radar")

        def per_radar_max():
            per_radar()
            torch.fmax(torch.fmax(grids[0], grids[1]), grids[2], out=out)

        def per_radar_nearest():
            per_radar()
            held, held_d = grids[0], torch.where(torch.isnan(grids[0]), float("inf"), d32[0])
            for r in (1, 2):
                take = ~torch.isnan(grids[r]) & (d32[r] < held_d)
                held, held_d = torch.where(take, grids[r], held), torch.where(take, d32[r], held_d)
            out.copy_(held)

        runs.update({"mean_new": combine(combines["mean"]), "max": combine(combines["max"]),
                     "nearest_radar": combine(combines["nearest_radar"]), "max_with_radar": combine(combines["max"], who),
                     "per_radar_max": per_radar_max, "per_radar_nearest": per_radar_nearest})
    rec["lattice"] = alternate(runs, args.launches, args.warmup, torch)
    if combines:       # the timed launches compute what the public route computes; the torch fold agrees where no NaN / tie decides
        for name in ("max", "nearest_radar"):
            runs[name]()
            public = rg.mosaic_fields_device(ms, [[f_t[offsets[r]:offsets[r + 1]]] for r in range(3)],
                                             shared_masks=[m_t[offsets[r]:offsets[r + 1]] for r in range(3)],
                                             weighting=args.weighting, combine=name)
            assert torch.equal(public.view(torch.int32).reshape(-1), out.view(torch.int32).reshape(-1)), name
        runs["max"]()
        one_launch = out.clone()
        per_radar_max()
        both = ~torch.isnan(one_launch) & ~torch.isnan(out)
        rec["lattice"]["filled_fraction"] = round(float((~torch.isnan(one_launch)).float().mean().item()), 4)
        rec["lattice"]["max_equals_per_radar_fmax"] = bool(torch.equal(one_launch[both], out[both]) and
                                                           torch.equal(torch.isnan(one_launch), torch.isnan(out)))
        del grids, d32, who, one_launch

    # ---- the section ------------------------------------------------------------------------------------------------------------
    a, b = THROUGH
    length = float(np.hypot(b[0] - a[0], b[1] - a[1]))
    xs, ys, _ = rg.section_path([a, b], length / (args.points - 1) * (1 - 1e-12))
    n = len(xs)
    pts = rg.mosaic_section_points(ms, xs, ys)
    dev_pts = [None if np.isnan(p[0]).all() else (torch.from_numpy(p[0]).to(dev), torch.from_numpy(p[1]).to(dev)) for p in pts]
    stable = ms.section_table([0, 1, 2], offsets[:-1], dev_pts)
    s_singles = [ms.section_table([r], [int(offsets[r])], [dev_pts[r]]) for r in range(3)]
    s_out = torch.empty((1, nz * n), dtype=torch.float32, device=dev)
    s_head = (stable, 3, nz, n, ms.min_radius, ms.beam_factor, w, _native.ptr(packed), 1, 1, n_total, nan, _native.ptr(s_out))
    runs = {"mean_old": lambda: _native.check(lib.rg_roi_section_mosaic_f32(*s_head, stream), "mean_old")}
    if combines:
        s_who = torch.empty((1, nz * n), dtype=torch.uint8, device=dev)
        s_grids = [torch.empty((1, nz * n), dtype=torch.float32, device=dev) for _ in range(3)]

        def s_combine(code, radar_map=None):
            return lambda: _native.check(lib.rg_roi_section_mosaic_combine_f32(*s_head, code, _native.ptr(radar_map), stream),
                                         "combine")

        def s_per_radar_max():
            for r in range(3):
                _native.check(lib.rg_roi_section_mosaic_f32(s_singles[r], 1, nz, n, ms.min_radius, ms.beam_factor, w,
                                                            _native.ptr(packed), 1, 1, n_total, nan, _native.ptr(s_grids[r]),
                                                            stream), "per radar")
            torch.fmax(torch.fmax(s_grids[0], s_grids[1]), s_grids[2], out=s_out)

        runs.update({"mean_new": s_combine(combines["mean"]), "max": s_combine(combines["max"]),
                     "nearest_radar": s_combine(combines["nearest_radar"]), "max_with_radar": s_combine(combines["max"], s_who),
                     "per_radar_max": s_per_radar_max})
    rec["section"] = alternate(runs, 4 * args.launches, args.warmup, torch)
    rec["section"]["points"] = n
    print(json.dumps(rec), flush=True)
    return 0


if __name__ == "__main__":
    sys.exit(main())
