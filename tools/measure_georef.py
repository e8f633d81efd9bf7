#!/usr/bin/env python3
"""The gate re-projection kernel (rg_gates_to_frame_f32) at the two gate counts the bench volumes have, next to the same
arithmetic in host NumPy float64 on the same machine:

    python tools/measure_georef.py [--launches 20] [--warmup 3] [--small] [--out PATH]

A radar 200 km east of the grid origin (lat -31.44); gates seeded uniformly within 480 km of the antenna (the kernel's work
per gate does not depend on where a finite gate lies, and every gate here is finite).  KERNEL times by stream events around
one launch each, out of place; the first ``--warmup`` launches are dropped; median, min and max of the rest.  The in-place
launch and the same-centre copy are timed the same way.  ``numpy_float64_ms`` is one evaluation of
``geographic_to_grid(grid_to_geographic(x, y))`` on the host (median of three), the route a user has without this kernel.

One JSON object on stdout (profiles/georef_timing.json)."""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

RADAR, ORIGIN = (-62.085, -31.44), (-64.19, -31.44)          # about 200 km apart on one parallel


def timed(run, launches, warmup, torch):
    times = []
    for i in range(warmup + launches):
        torch.cuda.synchronize()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        run()
        e1.record()
        e1.synchronize()
        if i >= warmup:
            times.append(e0.elapsed_time(e1))
    return {"median_ms": round(float(np.median(times)), 4), "min_ms": round(float(np.min(times)), 4),
            "max_ms": round(float(np.max(times)), 4)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--launches", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--small", action="store_true", help="40 000 gates: a rehearsal, not a measurement")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()

    import torch
    import radar_processor_amd as rg
    from radar_processor_amd import _native, georef
    from radar_processor_amd.build import ensure_built
    ensure_built(verbose=False)
    lib = _native.load_library()
    dev = _native.device()
    P, s = _native.ptr, _native.stream_ptr()
    sizes = (40_000,) if args.small else (4_320_000, 20_160_000)
    moved, same = georef.make_georef(RADAR, ORIGIN), georef.make_georef(ORIGIN, ORIGIN)
    ox, oy = rg.geographic_to_grid(*RADAR, *ORIGIN)
    results = []
    for n in sizes:
        rng = np.random.default_rng(n)
        r, az = 4.8e5 * np.sqrt(rng.random(n)), 2.0 * np.pi * rng.random(n)
        x, y = (r * np.sin(az)).astype(np.float32), (r * np.cos(az)).astype(np.float32)
        x_t, y_t = torch.from_numpy(x).to(dev), torch.from_numpy(y).to(dev)
        xo, yo = torch.empty_like(x_t), torch.empty_like(y_t)
        xi, yi = x_t.clone(), y_t.clone()

        def launch(g, a, b, c, d):
            def run():
                _native.check(lib.rg_gates_to_frame_f32(P(a), P(b), n, g, P(c), P(d), s), "rg_gates_to_frame_f32")
            return run
        kernel = timed(launch(moved, x_t, y_t, xo, yo), args.launches, args.warmup, torch)
        in_place = timed(launch(moved, xi, yi, xi, yi), args.launches, args.warmup, torch)      # its inputs drift: timing only
        copy = timed(launch(same, x_t, y_t, xi, yi), args.launches, args.warmup, torch)

        host = []
        for _ in range(3):
            t0 = time.perf_counter()
            lon, lat = rg.grid_to_geographic(x, y, *RADAR)
            hx, hy = rg.geographic_to_grid(lon, lat, *ORIGIN)
            hx, hy = (hx - ox).astype(np.float32), (hy - oy).astype(np.float32)
            host.append((time.perf_counter() - t0) * 1e3)
        got_x, got_y = xo.cpu().numpy(), yo.cpu().numpy()
        results.append({"gates": n, "kernel": kernel, "kernel_in_place": in_place, "same_centre_copy": copy,
                        "numpy_float64_ms": round(float(np.median(host)), 1),
                        "gates_per_us": round(n / kernel["median_ms"] / 1e3, 1),
                        "bytes_moved_gb_per_s": round(16.0 * n / kernel["median_ms"] / 1e6, 1),
                        "differs_from_numpy": int((got_x != hx).sum() + (got_y != hy).sum()),
                        "max_abs_diff_m": float(max(np.abs(got_x - hx).max(), np.abs(got_y - hy).max()))})
    line = {"what": "rg_gates_to_frame_f32: a radar 200 km from the grid origin, every gate finite", "radar": RADAR,
            "origin": ORIGIN, "launches": args.launches, "warmup": args.warmup, "device": torch.cuda.get_device_name(dev),
            "host_cpus_used_by_numpy": 1, "unit": "ms; stream events around one kernel launch", "results": results}
    text = json.dumps(line, indent=1)
    print(text)
    if args.out:
        with open(args.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
