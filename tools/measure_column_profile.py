#!/usr/bin/env python3
"""The column profile kernel (rg_column_profile_f32) next to the column maximum that reads the same grid, one fresh
process per call:

    python tools/measure_column_profile.py [--launches 20] [--warmup 3] [--small]

The bench grid, 40 x 2000 x 2000 float32 (640 MB: larger than the Infinity Cache), filled on the device with seeded values
on a 0.5 dB lattice in -10 .. 70 with 30 % NaN.  KERNEL times by stream events around one launch each; the variants
alternate; the first ``--warmup`` rounds are dropped; median, min and max of the rest:

  ``colmax_arg``        rg_column_reduce_f32, RG_COL_MAX with the arg plane: the yardstick
  ``top1``              one threshold, echo top only
  ``top1_nearest``      the same without interpolation (no float64 division at the end of the walk)
  ``top4_base4``        four thresholds, echo top and base, no VIL
  ``vil``               VIL alone
  ``top4_base4_vil``    four thresholds, echo top, base and VIL: everything one launch can produce
  ``top4_base4_1col``   ``top4_base4`` on the one-column-per-lane path, reached as a caller reaches it: output planes that
                        start one float into their buffers (not 16-byte aligned)
  ``vil_unaligned`` / ``top4_base4_vil_unaligned``   the two VIL requests with such planes (a launch with VIL takes one column
                        per lane whatever the alignment: these should equal ``vil`` / ``top4_base4_vil``)

One JSON object on stdout: run three processes and collect the lines (profiles/column_profile_timing.json)."""
import argparse
import ctypes
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

THRESHOLDS = (18.0, 30.0, 45.0, 5.0)


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
    ap.add_argument("--launches", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--small", action="store_true", help="a 6 x 120 x 120 grid: a rehearsal, not a measurement")
    args = ap.parse_args()

    import torch
    from radar_processor_amd import _native
    from radar_processor_amd.build import ensure_built
    ensure_built(verbose=False)
    lib = _native.load_library()
    dev = _native.device()
    nz, ny, nx = (6, 120, 120) if args.small else (40, 2000, 2000)
    n_xy = ny * nx
    gen = torch.Generator(device=dev).manual_seed(5)
    grid = torch.randint(-20, 141, (nz, ny, nx), generator=gen, device=dev).to(torch.float32).mul_(0.5)
    grid[torch.rand((nz, ny, nx), generator=gen, device=dev) < 0.3] = float("nan")
    zl = torch.linspace(500.0, 20000.0, nz, dtype=torch.float64, device=dev)
    top = torch.empty((4, ny, nx), dtype=torch.float32, device=dev)
    base = torch.empty((4, ny, nx), dtype=torch.float32, device=dev)
    vil = torch.empty((ny, nx), dtype=torch.float32, device=dev)
    cmax = torch.empty((ny, nx), dtype=torch.float32, device=dev)
    carg = torch.empty((ny, nx), dtype=torch.int32, device=dev)
    thr = (ctypes.c_double * 4)(*THRESHOLDS)
    s = _native.stream_ptr()
    P = _native.ptr

    def profile(n, t, b, v, linear=1):
        def run():
            _native.check(lib.rg_column_profile_f32(P(grid), nz, n_xy, 0, nz - 1, P(zl), thr, n, linear, P(t), P(b), 56.0, P(v), s),
                          "rg_column_profile_f32")
        return run

    def colmax():
        _native.check(lib.rg_column_reduce_f32(P(grid), nz, n_xy, 0, nz - 1, _native.COLUMN_OPS["max"], P(cmax), P(carg), s),
                      "rg_column_reduce_f32")

    top_u = torch.empty(4 * n_xy + 4, dtype=torch.float32, device=dev)[1:]          # unaligned planes: the one-column path
    base_u = torch.empty(4 * n_xy + 4, dtype=torch.float32, device=dev)[1:]
    vil_u = torch.empty(n_xy + 4, dtype=torch.float32, device=dev)[1:]
    assert vil_u.data_ptr() % 16 == 4 and top.data_ptr() % 16 == 0
    runs = {"colmax_arg": colmax, "top1": profile(1, top, None, None),
            "top1_nearest": profile(1, top, None, None, linear=0), "top4_base4": profile(4, top, base, None),
            "vil": profile(0, None, None, vil), "top4_base4_vil": profile(4, top, base, vil),
            "top4_base4_1col": profile(4, top_u, base_u, None),
            "vil_unaligned": profile(0, None, None, vil_u), "top4_base4_vil_unaligned": profile(4, top_u, base_u, vil_u)}
    times = alternate(runs, args.launches, args.warmup, torch)
    read_gb = 4.0 * nz * n_xy / 1e9
    line = {"grid_shape": [nz, ny, nx], "grid_read_gb": round(read_gb, 4), "launches": args.launches, "warmup": args.warmup,
            "device": torch.cuda.get_device_name(dev), "thresholds": list(THRESHOLDS),
            "unit": "ms; stream events around one kernel launch", "times": times,
            "read_tb_per_s": {k: round(read_gb / v["median_ms"], 3) for k, v in times.items()},
            "finite_fraction": {"top18": round(float(torch.isfinite(top[0]).float().mean()), 4),
                                "vil": round(float(torch.isfinite(vil).float().mean()), 4)},
            "paths_agree": bool(torch.equal(vil.view(torch.int32).reshape(-1), vil_u[:n_xy].view(torch.int32))
                                and torch.equal(top.view(torch.int32).reshape(-1), top_u[:4 * n_xy].view(torch.int32)))}
    print(json.dumps(line))


if __name__ == "__main__":
    main()
