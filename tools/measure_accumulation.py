#!/usr/bin/env python3
"""Rain rate and advection-corrected accumulation on a 2000 x 2000 plane pair, three fresh processes:

    python tools/measure_accumulation.py [--launches 20] [--warmup 3] [--small] [--out profiles/accumulation_timing.json]

The pair: the COLMAX plane of the bench volume (synthetic ``METRIC`` configuration, gridded by ``roi_grid_fields_device``)
converted to a rain rate, and the same plane translated by (5, -7) pixels, NaN where nothing moves in.  The motion is the
block match at its defaults (``B=32, S=16, R=16``), filled.  ``K = 16`` sub-instants.  Times in ms by stream events around one
call, the variants alternating, the first ``--warmup`` rounds dropped:

  ``rain_rate``                      rg_rain_rate_f32 of one plane
  ``fused_<method>_sub<n>``          rg_accumulate_advected_f32, nearest and bilinear, substeps 1 and 3, into a buffer kept
  ``composed_<method>_sub<n>``       what it replaces: two rg_advect_f32 launches of 16 leads into buffers kept, then the blend
                                     and the sum over the leads in torch (float64, the header's rule)
  ``update``                         one RainAccumulator.update end to end: rate, block match, fill, accumulation, window sum

``ratio_composed_over_fused`` above 1 means the fused kernel is faster; the tool fails when it is slower on any of the four
settings.  ``bytes``: what each route must move at the least, computed from the shapes -- the fused kernel reads two planes and
writes one, the composition also writes 32 planes and reads them back.  In every process the two routes are compared once:
the same pixels filled, the largest difference reported (torch sums the leads in another order than the kernel).  The parent
process only starts the children (``--child``), collects their JSON lines and writes the summary."""
import argparse
import json
import os
import subprocess
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

B, S, R = 32, 16, 16
SHIFT = (5, -7)
K = 16
HOURS = 300.0 / 3600.0
SETTINGS = (("nearest", 1), ("nearest", 3), ("bilinear", 1), ("bilinear", 3))


def child(args):
    import torch
    import radar_processor_amd as rg
    from measure_components import alternate, colmax_plane
    from radar_processor_amd import _native, motion
    from radar_processor_amd.build import ensure_built
    ensure_built(verbose=False)
    lib = _native.load_library()
    dev = _native.device()
    P, s = _native.ptr, _native.stream_ptr()
    dbz_prev = colmax_plane(args.small, torch)
    h, w = (int(v) for v in dbz_prev.shape)
    dbz_next = torch.full_like(dbz_prev, float("nan"))
    dbz_next[SHIFT[0]:, :SHIFT[1]] = dbz_prev[:-SHIFT[0], -SHIFT[1]:]
    prev, nxt = rg.rain_rate_device(dbz_prev), rg.rain_rate_device(dbz_next)
    grid = rg.fill_motion_device(rg.estimate_motion_device(dbz_prev, dbz_next, block=B, stride=S, search=R))
    field, lat = grid.motion.contiguous(), grid.lattice
    c_lat = _native.MotionLattice(*lat)
    p_zr, q_zr = np.log(10.0) / 16.0, np.log(200.0) / 1.6
    rate_out = torch.empty_like(prev)
    fused_out = torch.empty_like(prev)
    legs = [torch.empty((K, 1, h, w), dtype=torch.float32, device=dev) for _ in range(2)]
    leads = [(k + 0.5) / K for k in range(K)]
    c_fwd, c_back = (_native.c_double * K)(*leads), (_native.c_double * K)(*[v - 1.0 for v in leads])
    weight = torch.tensor(leads, dtype=torch.float64, device=dev)[:, None, None]
    zero = torch.zeros((), dtype=torch.float64, device=dev)
    nan32 = torch.full((), float("nan"), dtype=torch.float32, device=dev)

    def rain_rate():
        _native.check(lib.rg_rain_rate_f32(P(dbz_prev), 0, 1, h, w, p_zr, q_zr, 5.0, 55.0, P(rate_out), s), "rg_rain_rate_f32")

    def fused(method, substeps):
        def run():
            _native.check(lib.rg_accumulate_advected_f32(P(prev), P(nxt), 1, h, w, P(field), c_lat, HOURS, K, substeps, method, K,
                                                         float("nan"), P(fused_out), 0, s), "rg_accumulate_advected_f32")
            return fused_out
        return run

    def composed(method, substeps):
        def run():
            for src, c_leads, out in ((prev, c_fwd, legs[0]), (nxt, c_back, legs[1])):
                _native.check(lib.rg_advect_f32(P(src), 1, h, w, P(field), c_lat, c_leads, K, substeps, method, float("nan"), P(out), s),
                              "rg_advect_f32")
            a, b = legs[0][:, 0].to(torch.float64), legs[1][:, 0].to(torch.float64)
            has_a, has_b = ~torch.isnan(a), ~torch.isnan(b)
            r = torch.where(has_a & has_b, (1.0 - weight) * a + weight * b, torch.where(has_a, a, b))
            present = has_a | has_b
            total = torch.where(present, r, zero).sum(dim=0)
            n = present.sum(dim=0)
            return torch.where(n >= K, (HOURS * (total / n.clamp(min=1))).to(torch.float32), nan32)
        return run

    acc = rg.RainAccumulator(block=B, stride=S, search=R)
    acc.update(dbz_prev, 0.0)
    clock = {"t": 0.0, "flip": False}

    def update():
        clock["t"] += 300.0
        clock["flip"] = not clock["flip"]
        acc.update(dbz_next if clock["flip"] else dbz_prev, clock["t"])

    runs = {"rain_rate": rain_rate}
    agreement = {}
    for name, substeps in SETTINGS:
        method = motion.ADVECT_METHODS[name]
        key = f"{name}_sub{substeps}"
        runs["fused_" + key], runs["composed_" + key] = fused(method, substeps), composed(method, substeps)
        one, two = runs["fused_" + key]().clone(), runs["composed_" + key]()
        same_fill = bool(torch.equal(torch.isnan(one), torch.isnan(two)))
        live = ~torch.isnan(one) & ~torch.isnan(two)
        agreement[key] = {"same_pixels_filled": same_fill, "filled_fraction": round(float(live.float().mean().item()), 4),
                          "largest_difference_mm": float((one[live] - two[live]).abs().max().item()) if bool(live.any()) else 0.0,
                          "largest_depth_mm": float(one[live].max().item()) if bool(live.any()) else 0.0}
    runs["update"] = update
    times = alternate(runs, args.launches, args.warmup, torch)
    plane_bytes = 4 * h * w
    line = {"plane_shape": [h, w], "settings": {"B": B, "S": S, "R": R, "shift": list(SHIFT), "K": K, "hours": HOURS},
            "launches": args.launches, "warmup": args.warmup, "device": torch.cuda.get_device_name(dev),
            "unit": "ms; stream events around one call", "lattice": [lat.ny, lat.nx],
            "rain_fraction": round(float((prev > 0).float().mean().item()), 4), "times": times, "agreement": agreement,
            "bytes": {"plane": plane_bytes, "fused_compulsory": 3 * plane_bytes,
                      "composed_compulsory": (2 + 2 * K) * plane_bytes + (2 * K + 1) * plane_bytes,
                      "composed_note": "two advections read a plane and write 16 each; the blend reads the 32 and writes one; torch's "
                                       "float64 intermediates come on top"}}
    print(json.dumps(line))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--launches", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--processes", type=int, default=3)
    ap.add_argument("--small", action="store_true", help="a 200 x 200 plane: a rehearsal, not a measurement")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "accumulation_timing.json"))
    ap.add_argument("--child", action="store_true", help=argparse.SUPPRESS)
    args = ap.parse_args()
    if args.child:
        return child(args)
    cmd = [sys.executable, os.path.abspath(__file__), "--child", "--launches", str(args.launches), "--warmup", str(args.warmup)]
    cmd += ["--small"] if args.small else []
    lines = []
    for _ in range(args.processes):                       # one after another: a fresh process each, never two on the GPU
        done = subprocess.run(cmd, check=True, capture_output=True, text=True, timeout=400)
        lines.append(json.loads(done.stdout.strip().splitlines()[-1]))
    summary = {}
    for key in lines[0]["times"]:
        medians = [ln["times"][key]["median_ms"] for ln in lines]
        summary[key] = {"median_ms_per_process": medians, "median_ms": round(float(np.median(medians)), 4),
                        "spread_ms": round(max(medians) - min(medians), 4)}
    ratios = {}
    for name, substeps in SETTINGS:
        key = f"{name}_sub{substeps}"
        ratios[key] = round(summary["composed_" + key]["median_ms"] / summary["fused_" + key]["median_ms"], 3)
    summary["ratio_composed_over_fused"] = ratios
    rec = {"what": "tools/measure_accumulation.py on one MI355X, %d fresh processes: the %d x %d COLMAX plane of the bench volume as "
                   "a rain rate, paired with itself translated by %s pixels; block-match motion at B=%d S=%d R=%d, filled; K=%d "
                   "sub-instants; times in ms by stream events around one call, variants alternating, %d launches after %d warm-up "
                   "rounds. rain_rate = rg_rain_rate_f32 of one plane; fused_<method>_sub<n> = rg_accumulate_advected_f32; "
                   "composed_<method>_sub<n> = two rg_advect_f32 launches of 16 leads plus the float64 blend and sum in torch; "
                   "update = one RainAccumulator.update end to end. ratio_composed_over_fused above 1: the fused kernel is faster."
                   % (len(lines), *lines[0]["plane_shape"], list(SHIFT), B, S, R, K, args.launches, args.warmup),
           "summary": summary, "lines": lines}
    with open(args.out, "w") as f:
        json.dump(rec, f, indent=1)
        f.write("\n")
    print(json.dumps(summary, indent=1))
    slower = [k for k, v in ratios.items() if v < 1.0]
    if slower:
        sys.exit(f"the fused kernel is slower than the composition on {slower}")


if __name__ == "__main__":
    main()
