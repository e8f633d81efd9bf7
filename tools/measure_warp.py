#!/usr/bin/env python3
"""The Web Mercator warp and the overview pyramid (csrc/rg_warp.hip) on a plane a user would put on a map:

    python tools/measure_warp.py [--rounds 20] [--warmup 3] [--calls 20] [--small] [--variant-lib PATH] [--out PATH]

A 2000 x 2000 plane (limits +-500 km about lat -31.44, 30 % NaN) into its ``mercator_raster_for`` raster, and into one 256 x 256
XYZ tile (zoom 8, over the origin): nearest and bilinear, 1 and 3 planes, the RGBA route, the [2, 4, 8, 16] pyramid with both
rules, ``colormap_rgba_device`` over the same raster as the yardstick, and ``web_mercator_rgba`` end to end.

``--variant-lib``: another build of the library whose ``rg_warp_mercator_f32`` is timed beside the shipped one under the labels
``per_pixel_trig_*`` -- the lines of profiles/warp_timing.json come from a build that evaluated tanh, cosh and sincos for every
pixel instead of once per row and column of a block's tile (EXPERIMENTS.md; not in the tree).  Its outputs must equal the
shipped kernel's bit for bit; the script checks that before it times either, and records the answer.

Every label is timed by stream events around ``--calls`` back-to-back calls (a single launch is tens of microseconds), the
labels interleaved round by round in ONE process; the first ``--warmup`` rounds are dropped; median, min and max of the rest,
per call.  One JSON object on stdout (profiles/warp_timing.json)."""
import argparse
import ctypes
import json
import os
import sys

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)

ORIGIN = (-64.19, -31.44)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--calls", type=int, default=20, help="back-to-back calls inside one pair of events")
    ap.add_argument("--small", action="store_true", help="a 200 x 200 plane: a rehearsal, not a measurement")
    ap.add_argument("--variant-lib", default=None, help="another build of the library to time beside the shipped one")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()

    import torch
    import radar_processor_amd as rg
    from radar_processor_amd import _native, georef
    from radar_processor_amd.build import ensure_built
    ensure_built(verbose=False)
    lib = _native.load_library()
    dev = _native.device()
    P, stream = _native.ptr, _native.stream_ptr()

    n = 200 if args.small else 2000
    limits = ((-500e3, 500e3), (-500e3, 500e3))
    rng = np.random.default_rng(2000)
    yy, xx = np.mgrid[0:n, 0:n].astype(np.float32) / np.float32(n)
    plane = (40.0 * np.sin(6.0 * xx) * np.cos(4.0 * yy) + rng.normal(0.0, 4.0, (n, n))).astype(np.float32)
    plane[rng.random((n, n)) < 0.3] = np.nan
    planes3 = np.stack([plane, plane + 1.0, -plane]).astype(np.float32)
    full = rg.mercator_raster_for((n, n), limits, ORIGIN)
    x0, y0 = (float(v) for v in rg.lonlat_to_mercator(*ORIGIN))
    world = 2.0 * np.pi * 6378137.0
    tile = rg.mercator_tile(8, int((x0 / world + 0.5) * 256), int((0.5 - y0 / world) * 256))
    lut = torch.from_numpy(rg.colormap_lut(np.stack([np.linspace(0, 1, 256)] * 3 + [np.ones(256)], axis=1))).to(dev)
    p1, p3 = torch.from_numpy(plane).to(dev), torch.from_numpy(planes3).to(dev)
    rgba_src = rg.colormap_rgba_device(p1, lut, -40.0, 40.0)
    g = georef.make_georef(ORIGIN, ORIGIN)
    source = _native.WarpSource(limits[1][0], limits[0][0], 1000e3 / (n - 1), 1000e3 / (n - 1), n, n)

    labels = {}

    def warp_call(library, src, n_planes, raster, method, out):
        c_raster = _native.MercatorRaster(*raster)

        def run():
            status = library.rg_warp_mercator_f32(P(src), n_planes, source, g, c_raster, method, float("nan"), P(out), stream)
            assert status == 0, status
        return run

    outs = {}
    for where, raster in (("full", full), ("tile", tile)):
        for method, mname in ((0, "nearest"), (1, "bilinear")):
            for n_planes, src in ((1, p1), (3, p3)):
                out = torch.empty((n_planes, raster.height, raster.width), dtype=torch.float32, device=dev)
                outs[(where, mname, n_planes)] = out
                labels[f"warp_{where}_{mname}_{n_planes}p"] = warp_call(lib, src, n_planes, raster, method, out)
        labels[f"warp_{where}_rgba"] = (lambda r=raster: rg.warp_to_mercator_device(rgba_src, limits, ORIGIN, r))
    warped = rg.warp_to_mercator_device(p1, limits, ORIGIN, full)
    rgba_full = rg.colormap_rgba_device(warped, lut, -40.0, 40.0)
    labels["colormap_rgba_device_full"] = lambda: rg.colormap_rgba_device(warped, lut, -40.0, 40.0)
    labels["pyramid_full_rgba_nearest"] = lambda: rg.overview_pyramid_device(rgba_full)
    labels["pyramid_full_f32_nearest"] = lambda: rg.overview_pyramid_device(warped)
    labels["pyramid_full_f32_average"] = lambda: rg.overview_pyramid_device(warped, None, "average")
    labels["web_mercator_rgba_nearest"] = lambda: rg.web_mercator_rgba(p1, limits, ORIGIN, lut, -40.0, 40.0)
    labels["web_mercator_rgba_bilinear_average"] = lambda: rg.web_mercator_rgba(p1, limits, ORIGIN, lut, -40.0, 40.0,
                                                                                method="bilinear", resampling="average")

    per_pixel_same = None
    if args.variant_lib:
        variant = ctypes.CDLL(args.variant_lib)
        variant.rg_warp_mercator_f32.restype, variant.rg_warp_mercator_f32.argtypes = _native.SIGNATURES["rg_warp_mercator_f32"]
        per_pixel_same = True
        for where, raster in (("full", full), ("tile", tile)):
            for method, mname in ((0, "nearest"), (1, "bilinear")):
                out = torch.empty((1, raster.height, raster.width), dtype=torch.float32, device=dev)
                run = warp_call(variant, p1, 1, raster, method, out)
                labels[f"per_pixel_trig_{where}_{mname}_1p"] = run
                run()
                labels[f"warp_{where}_{mname}_1p"]()
                torch.cuda.synchronize()
                per_pixel_same &= bool(torch.equal(out.view(torch.int32), outs[(where, mname, 1)].view(torch.int32)))

    times = {k: [] for k in labels}
    for i in range(args.warmup + args.rounds):
        for name, run in labels.items():
            torch.cuda.synchronize()
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(args.calls):
                run()
            e1.record()
            e1.synchronize()
            if i >= args.warmup:
                times[name].append(e0.elapsed_time(e1) / args.calls)
    results = {k: {"median_ms": round(float(np.median(v)), 4), "min_ms": round(float(np.min(v)), 4),
                   "max_ms": round(float(np.max(v)), 4)} for k, v in times.items()}
    line = {"what": "rg_warp_mercator_* / rg_overview_*: a %d x %d plane, 30 %% NaN, limits +-500 km at %r" % (n, n, ORIGIN),
            "full_raster": list(full), "tile_raster": list(tile), "rounds": args.rounds, "warmup": args.warmup,
            "device": torch.cuda.get_device_name(dev),
            "calls_per_sample": args.calls,
            "unit": "ms per call; stream events around calls_per_sample back-to-back calls, labels interleaved round by round in "
                    "one process; warp_* of the float "
                    "planes and per_pixel_trig_* are one kernel launch through the C entry point, the other labels go through "
                    "the Python surface (allocation of the result included)",
            "per_pixel_trig": "not measured" if per_pixel_same is None else
                              {"same_bits_as_shipped": per_pixel_same, "library": os.path.basename(args.variant_lib)},
            "full_raster_mpixels_per_ms": round(full.width * full.height / results["warp_full_nearest_1p"]["median_ms"] / 1e6, 3),
            "results": results}
    text = json.dumps(line, indent=1)
    print(text)
    if args.out:
        with open(args.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
