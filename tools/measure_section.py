#!/usr/bin/env python3
"""A vertical section next to the full CSR-free pass, same process, same search structure, interleaved rounds:

    python tools/measure_section.py [--points 2000] [--offset 0] [--rounds 9] [--weighting barnes2] [--out profiles/section_timing.json]

The bench volume (12 x 360 x 1000 gates) and a RoiSearch for the 40 x 2000 x 2000 grid.  Per round, each of

  (a) ``section``   rg_roi_section_f32: a diagonal of ``--points`` points (corner to corner of the grid) x 40 levels, one field;
  (b) ``full``      rg_roi_grid_f32: the whole lattice, one field (the yardstick: README's 10.9 ms);
  (c) ``geometry``  compute_section_geometry of the same diagonal (count + scan + fill + the host's two reads)

is timed once, in an order that rotates per round.  (a) and (b) are KERNEL times -- the fields are packed once, outside the
timed region, and stream events bracket the one launch; (c) brackets the whole call.  The median over rounds is reported.
The section has 1 / 2000 of the full pass's samples: it has to come out below it.  One JSON object on stdout and in
``--out``."""
import argparse
import ctypes
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--points", type=int, default=2000)
    ap.add_argument("--rounds", type=int, default=9)
    ap.add_argument("--weighting", default="barnes2")
    ap.add_argument("--offset", type=float, default=0.0,
                    help="start the diagonal this many metres up the grid's left edge: it then misses the radar by offset / sqrt(2)")
    ap.add_argument("--out", default="")
    args = ap.parse_args()
    import torch
    import radar_processor_amd as rg
    from radar_processor_amd import _native, synthetic
    lib = rg.load_library()
    dev = torch.device("cuda", 0)
    cfg = synthetic.CONFIGS["METRIC"]
    vol = synthetic.make_volume(cfg["n_elev"], cfg["n_az"], cfg["n_gates"], seed=0, fields=("DBZH",))
    search = rg.RoiSearch(vol.gate_x, vol.gate_y, vol.gate_z, cfg["grid_shape"], cfg["grid_limits"], device=dev)
    nz, ny, nx = search.grid_shape
    (y0, y1), (x0, x1) = cfg["grid_limits"][1], cfg["grid_limits"][2]
    length = float(np.hypot(x1 - x0, y1 - y0))
    y0, x1 = y0 + args.offset, x1 - args.offset
    length = float(np.hypot(x1 - x0, y1 - y0))
    xs, ys, s = rg.section_path([(x0, y0), (x1, y1)], length / (args.points - 1) * (1 - 1e-12))
    n = len(xs)
    f_t = torch.from_numpy(np.ascontiguousarray(np.ma.getdata(vol.fields["DBZH"]))).to(dev)
    m_t = torch.from_numpy(np.ma.getmaskarray(vol.fields["DBZH"]).astype(np.uint8)).to(dev)
    w = _native.WEIGHTINGS[args.weighting]
    xs_t, ys_t = torch.from_numpy(xs).to(dev), torch.from_numpy(ys).to(dev)
    packed = torch.empty(search.n_gates, dtype=torch.float32, device=dev)
    out_s = torch.empty((1, nz, n), dtype=torch.float32, device=dev)
    out_f = torch.empty((1, nz, ny, nx), dtype=torch.float32, device=dev)
    stream = _native.stream_ptr()
    fptrs, mptrs = (ctypes.c_void_p * 1)(_native.ptr(f_t)), (ctypes.c_void_p * 1)(_native.ptr(m_t))
    _native.check(lib.rg_pack_fields_f32(1, fptrs, mptrs, None, search.n_gates, 1, _native.ptr(packed), stream), "pack")
    head = (_native.ptr(search.sorted_gates), _native.ptr(search.cell_start), search.cells)
    tail = (search.min_radius, search.beam_factor, w, _native.ptr(packed), 1, 1, float("nan"))

    def section():
        _native.check(lib.rg_roi_section_f32(*head, _native.ptr(xs_t), _native.ptr(ys_t), _native.ptr(search.zc), nz, n,
                                             *tail, _native.ptr(out_s), stream), "rg_roi_section_f32")

    def full():
        _native.check(lib.rg_roi_grid_f32(*head, _native.ptr(search.xc), _native.ptr(search.yc), _native.ptr(search.zc), nz,
                                          ny, nx, *tail, _native.ptr(out_f), stream), "rg_roi_grid_f32")

    def geometry():
        return rg.compute_section_geometry(search, xs, ys, args.weighting)

    runs = {"section": section, "full": full, "geometry": geometry}
    for fn in runs.values():                                        # warm-up
        fn()
    torch.cuda.synchronize()
    # the timed launch against the public route
    public = rg.section_fields_device(search, xs, ys, [f_t], [m_t], weighting=args.weighting)
    same_as_public = bool(torch.equal(public.view(torch.int32), out_s.view(torch.int32)))
    times = {k: [] for k in runs}
    keys = list(runs)
    for r in range(args.rounds):
        for key in keys[r % 3:] + keys[:r % 3]:
            torch.cuda.synchronize()
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            runs[key]()
            e1.record()
            e1.synchronize()
            times[key].append(e0.elapsed_time(e1))
    med = {k: round(float(np.median(v)), 4) for k, v in times.items()}
    filled = float(torch.isfinite(out_s).float().mean().item())
    rec = {"volume": [cfg["n_elev"], cfg["n_az"], cfg["n_gates"]], "grid_shape": list(cfg["grid_shape"]), "points": n,
           "levels": nz, "offset_m": args.offset, "weighting": args.weighting, "rounds": args.rounds, "path_length_m": float(s[-1]),
           "unit": "ms; section / full: events around the one kernel launch; geometry: around compute_section_geometry",
           "median_ms": med, "all_ms": {k: [round(t, 4) for t in v] for k, v in times.items()},
           "section_vs_full": round(med["section"] / med["full"], 5), "section_filled_fraction": round(filled, 4),
           "section_same_bits_as_section_fields_device": same_as_public,
           "device": torch.cuda.get_device_name(0)}
    print(json.dumps(rec))
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as fh:
            json.dump(rec, fh, indent=1)
    assert same_as_public
    return 0 if med["section"] < med["full"] else 1


if __name__ == "__main__":
    sys.exit(main())
