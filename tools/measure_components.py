#!/usr/bin/env python3
"""Connected-component labelling, the cell table and despeckling on 2000 x 2000 planes, three fresh processes:

    python tools/measure_components.py [--launches 20] [--warmup 3] [--small] [--planes a,b] [--out profiles/components_timing.json]

Planes: the COLMAX plane of the bench volume (synthetic ``METRIC`` configuration, gridded by ``roi_grid_fields_device``) at
18, 35 and 45 dBZ, and three constructed planes of the same size -- all foreground (one cell), a checkerboard under
4-connectivity (every foreground pixel its own cell) and a one-pixel serpentine (one cell that crosses every tile seam).
Per plane, times in ms by stream events, the variants alternating, the first ``--warmup`` rounds dropped:

  ``label``            rg_label_components_f32 (six launches), 8-connectivity (4 for the checkerboard)
  ``stats``            rg_component_stats_f32, every output
  ``select``           rg_despeckle_select_f32 with a mask output
  ``despeckle_device`` the whole public call (label + areas + select, allocations included), min_size 10

and ``scipy.ndimage.label`` on the same foreground on the host (one run, wall clock), for context.  The parent process only
starts the children (``--child``), collects their JSON lines and writes the summary.  For the time of each of the launches
of a call, run one child under a kernel trace: ``rocprofv3 --kernel-trace --stats -- python tools/measure_components.py --child
--planes all_foreground``."""
import argparse
import json
import os
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

COLMAX_THRESHOLDS = (18.0, 35.0, 45.0)


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


def colmax_plane(small, torch):
    """COLMAX of the bench volume on its grid (``--small``: a 6-sweep volume on a 200 x 200 grid, a rehearsal)."""
    from radar_processor_amd import (RoiSearch, collapse_plane_device, get_field_data, get_gate_coordinates,
                                     roi_grid_fields_device, synthetic)
    cfg = dict(synthetic.CONFIGS["METRIC"])
    if small:
        cfg.update(n_elev=6, n_az=360, n_gates=480, grid_shape=(8, 200, 200))
    radar = synthetic.make_volume(cfg["n_elev"], cfg["n_az"], cfg["n_gates"], seed=0, fields=("DBZH",)).as_radar()
    search = RoiSearch(*get_gate_coordinates(radar), cfg["grid_shape"], cfg["grid_limits"])
    dbz = get_field_data(radar, "DBZH")
    field = torch.from_numpy(np.ascontiguousarray(dbz.filled(np.nan), dtype=np.float32).ravel()).to(search.dev)
    mask = torch.from_numpy(np.ma.getmaskarray(dbz).ravel().astype(np.uint8)).to(search.dev)
    grid = roi_grid_fields_device(search, [field], [mask])[0]
    return collapse_plane_device(grid, "colmax").contiguous()


def constructed(h, w, torch, dev):
    yy = torch.arange(h, device=dev)[:, None]
    xx = torch.arange(w, device=dev)[None, :]
    serp = (yy % 2 == 0).expand(h, w).clone()
    odd = torch.arange(1, h, 2, device=dev)
    serp[odd, torch.where((odd // 2) % 2 == 0, w - 1, 0)] = True
    value = lambda fg: torch.where(fg, 40.0, float("nan")).to(torch.float32).contiguous()
    return {"all_foreground": (value(torch.ones((h, w), dtype=torch.bool, device=dev)), 35.0, 8),
            "checkerboard_4": (value((yy + xx) % 2 == 0), 35.0, 4), "serpentine": (value(serp), 35.0, 8)}


def child(args):
    import torch
    import radar_processor_amd as rg
    from radar_processor_amd import _native
    from radar_processor_amd.build import ensure_built
    ensure_built(verbose=False)
    lib = _native.load_library()
    dev = _native.device()
    P, s = _native.ptr, _native.stream_ptr()
    colmax = colmax_plane(args.small, torch)
    h, w = (int(v) for v in colmax.shape)
    planes = {f"colmax_{int(t)}dbz": (colmax, t, 8) for t in COLMAX_THRESHOLDS}
    planes.update(constructed(h, w, torch, dev))
    if args.planes:
        planes = {k: planes[k] for k in args.planes.split(",")}
    need = int(lib.rg_components_workspace_bytes(1, h, w))
    workspace = torch.empty(need, dtype=torch.uint8, device=dev)
    labels = torch.empty((h, w), dtype=torch.int32, device=dev)
    cell_ptr = torch.empty(2, dtype=torch.int32, device=dev)
    out = torch.empty((h, w), dtype=torch.float32, device=dev)
    removed = torch.empty((h, w), dtype=torch.uint8, device=dev)
    line = {"plane_shape": [h, w], "launches": args.launches, "warmup": args.warmup, "device": torch.cuda.get_device_name(dev),
            "unit": "ms; stream events around one call", "planes": {}}
    for name, (plane, lo, conn) in planes.items():
        def label():
            _native.check(lib.rg_label_components_f32(P(plane), 0, 1, h, w, lo, float("inf"), conn, 0, P(labels), P(cell_ptr),
                                                      P(workspace), need, s), "rg_label_components_f32")
        label()
        cells = int(cell_ptr[-1].item())
        t = {k: torch.empty(shape, dtype=dt, device=dev) for k, shape, dt in (
            ("area", (cells,), torch.int32), ("bbox", (cells, 4), torch.int32), ("sum_yx", (cells, 2), torch.int64),
            ("vmax", (cells,), torch.float32), ("argmax", (cells,), torch.int32), ("vsum", (cells,), torch.float64))}

        def stats():
            _native.check(lib.rg_component_stats_f32(P(plane), P(labels), P(cell_ptr), 1, h, w, cells, P(t["area"]), P(t["bbox"]),
                                                     P(t["sum_yx"]), P(t["vmax"]), P(t["argmax"]), P(t["vsum"]), s),
                          "rg_component_stats_f32")

        def select():
            _native.check(lib.rg_despeckle_select_f32(P(plane), P(labels), P(cell_ptr), P(t["area"]), 1, h, w, 10, float("nan"),
                                                      P(out), P(removed), s), "rg_despeckle_select_f32")
        stats()
        runs = {"label": label, "stats": stats, "select": select,
                "despeckle_device": lambda: rg.despeckle_device(plane, lo, 10, connectivity=conn)}
        times = alternate(runs, args.launches, args.warmup, torch)
        fg = (plane >= lo).cpu().numpy()
        rec = {"threshold": lo, "connectivity": conn, "foreground_fraction": round(float(fg.mean()), 4), "cells": cells,
               "largest_cell": int(t["area"].max().item()) if cells else 0, "removed_below_10": int(removed.sum().item()),
               "times": times}
        try:
            from scipy import ndimage
            t0 = time.perf_counter()
            _, count = ndimage.label(fg, structure=np.ones((3, 3)) if conn == 8 else None)
            rec["scipy_label_ms"] = round(1e3 * (time.perf_counter() - t0), 2)
            rec["scipy_cells_agree"] = bool(count == cells)
        except ImportError:
            rec["scipy_label_ms"] = None
        line["planes"][name] = rec
    print(json.dumps(line))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--launches", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--processes", type=int, default=3)
    ap.add_argument("--small", action="store_true", help="a 200 x 200 plane: a rehearsal, not a measurement")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "components_timing.json"))
    ap.add_argument("--planes", default="", help="comma-separated plane names to measure (default: all six)")
    ap.add_argument("--child", action="store_true", help=argparse.SUPPRESS)
    args = ap.parse_args()
    if args.child:
        return child(args)
    cmd = [sys.executable, os.path.abspath(__file__), "--child", "--launches", str(args.launches), "--warmup", str(args.warmup)]
    cmd += ["--small"] if args.small else []
    cmd += ["--planes", args.planes] if args.planes else []
    lines = []
    for _ in range(args.processes):                       # one after another: a fresh process each, never two on the GPU
        done = subprocess.run(cmd, check=True, capture_output=True, text=True, timeout=600)
        lines.append(json.loads(done.stdout.strip().splitlines()[-1]))
    summary = {}
    for name in lines[0]["planes"]:
        summary[name] = {k: lines[0]["planes"][name][k] for k in ("threshold", "connectivity", "foreground_fraction", "cells",
                                                                  "largest_cell")}
        for key in lines[0]["planes"][name]["times"]:
            medians = [ln["planes"][name]["times"][key]["median_ms"] for ln in lines]
            summary[name][key] = {"median_ms_per_process": medians, "spread_ms": round(max(medians) - min(medians), 4)}
        summary[name]["scipy_label_ms_per_process"] = [ln["planes"][name]["scipy_label_ms"] for ln in lines]
    rec = {"what": "tools/measure_components.py on one MI355X, %d fresh processes: one %d x %d float32 plane, times in ms by stream "
                   "events around one call, variants alternating, %d launches after %d warm-up rounds. label = "
                   "rg_label_components_f32 (tile, seam, flatten, scan, rank, write), stats = rg_component_stats_f32 with every "
                   "output, select = rg_despeckle_select_f32 with its mask, despeckle_device = the whole public call, allocations "
                   "included. scipy_label_ms: scipy.ndimage.label on the same foreground on the host, wall clock, one run. "
                   "`summary` gives, per plane and variant, the median of each process and the spread between processes."
                   % (len(lines), *lines[0]["plane_shape"], args.launches, args.warmup),
           "summary": summary, "lines": lines}
    with open(args.out, "w") as f:
        json.dump(rec, f, indent=1)
        f.write("\n")
    print(json.dumps(summary, indent=1))


if __name__ == "__main__":
    main()
