#!/usr/bin/env python3
"""Convective / stratiform classification on the bench volume's 2000 x 2000 planes, three fresh processes:

    python tools/measure_convection.py [--launches 20] [--warmup 3] [--small] [--out profiles/convection_timing.json]

The planes: the 3 km CAPPI and the COLMAX of the bench volume (synthetic ``METRIC`` configuration, gridded by
``roi_grid_fields_device``; 240 m pixels, so the 11 km background disk is 46 pixels in radius: 91 rows of up to 91 pixels).
Steiner's relations at the defaults (``intense=40``, the "medium" radii).  Times in ms by stream events around one call, the
variants alternating, the first ``--warmup`` rounds dropped, per plane:

  ``echo_table``   rg_echo_table_f32
  ``background``   rg_disk_background writing the background only (the classification's call)
  ``centres``      rg_convective_centres_f32
  ``area``         rg_convective_area_u8 (the per-class row prefixes and the footprint counts)
  ``whole_call``   convective_stratiform_device end to end, with its allocations

``oracle_seconds``: the NumPy restatement (tests/convection_oracle.py) of the same chain on the same plane in the same
process, once; ``differing_pixels`` counts where its classes are not the device's (a decision closer than one float32 step of
the background can differ; the tests pin the chain stage by stage instead).  ``background_loads``: the bytes the background
kernel loads from the table -- two entries per covered row and pixel, 12 bytes of each (the generated code loads the prefix
of q and the count, ``global_load_dwordx3``, not the reserved word) -- and the rate that makes at the measured time, to be
read against two bounds: the rate at which 16-byte loads are served from L2 on this part (about 17-19 TB/s chip-wide, a
measured figure) and the peak of the vector L1, 64 bytes per clock and CU x 256 CUs x 2.4 GHz = 39.3 TB/s (from the
datasheet, not measured here).  A rate above the first says the loads hit L1: neighbouring rows of a workgroup's tile read
the same table rows.  Its compulsory traffic is the table read once plus one plane written.  No time here is a pass
criterion: nothing in the package did this before.  The parent process only starts the children (``--child``), collects their
JSON lines and writes the summary."""
import argparse
import json
import os
import subprocess
import sys
import time
import types

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))

ALTITUDE = 3000.0
RADIUS = 11000.0
RELATION = "medium"
L2_GATHER_TBS = (16.8, 18.8)
ENTRY_LOAD_BYTES = 12                                   # of a 16-byte entry: global_load_dwordx3
L1_PEAK_TBS = 64 * 256 * 2.4e9 / 1e12                     # bytes per clock and CU x CUs x clock: 39.3


def bench_planes(small, torch):
    """``({"cappi_3km": plane, "colmax": plane}, dy, dx)`` of the bench volume on its grid."""
    import radar_processor_amd as rg
    from radar_processor_amd import synthetic
    cfg = dict(synthetic.CONFIGS["METRIC"])
    if small:
        cfg.update(n_elev=6, n_az=360, n_gates=480, grid_shape=(8, 200, 200))
    radar = synthetic.make_volume(cfg["n_elev"], cfg["n_az"], cfg["n_gates"], seed=0, fields=("DBZH",)).as_radar()
    search = rg.RoiSearch(*rg.get_gate_coordinates(radar), cfg["grid_shape"], cfg["grid_limits"])
    dbz = rg.get_field_data(radar, "DBZH")
    field = torch.from_numpy(np.ascontiguousarray(dbz.filled(np.nan), dtype=np.float32).ravel()).to(search.dev)
    mask = torch.from_numpy(np.ma.getmaskarray(dbz).ravel().astype(np.uint8)).to(search.dev)
    grid = rg.roi_grid_fields_device(search, [field], [mask])[0]
    geometry = types.SimpleNamespace(grid_shape=tuple(cfg["grid_shape"]), grid_limits=tuple(cfg["grid_limits"]))
    (y_lo, y_hi), (x_lo, x_hi) = cfg["grid_limits"][1:]
    dy, dx = (y_hi - y_lo) / (cfg["grid_shape"][1] - 1), (x_hi - x_lo) / (cfg["grid_shape"][2] - 1)
    planes = {"cappi_3km": rg.constant_altitude_ppi(grid, geometry, ALTITUDE).contiguous(),
              "colmax": rg.collapse_plane_device(grid, "colmax").contiguous()}
    return planes, dy, dx


def child(args):
    import torch
    import convection_oracle as co
    import radar_processor_amd as rg
    from measure_components import alternate
    from radar_processor_amd import _native, convection
    from radar_processor_amd.build import ensure_built
    ensure_built(verbose=False)
    lib = _native.load_library()
    dev = _native.device()
    P, s = _native.ptr, _native.stream_ptr()
    planes, dy, dx = bench_planes(args.small, torch)
    edges, radii = convection.AREA_RELATIONS[RELATION]
    hw = rg.disk_footprint(RADIUS, dy, dx)
    footprints = [rg.disk_footprint(r, dy, dx) for r in radii]
    K = len(footprints)
    c_hw = (_native.c_int32 * len(hw))(*hw)
    c_edges = (_native.c_double * len(edges))(*edges)
    rows = (_native.c_int32 * (K * 128))()
    for k, f in enumerate(footprints):
        rows[k * 128:k * 128 + len(f)] = f
    ry = (_native.c_int32 * K)(*[len(f) - 1 for f in footprints])
    results = {}
    for name, plane in planes.items():
        h, w = (int(v) for v in plane.shape)
        table = torch.empty(int(lib.rg_echo_table_bytes(1, h, w)), dtype=torch.uint8, device=dev)
        ws_bytes = int(lib.rg_convective_area_workspace_bytes(1, h, w, K))
        workspace = torch.empty(ws_bytes, dtype=torch.uint8, device=dev)
        bkg = torch.empty((h, w), dtype=torch.float32, device=dev)
        centres = torch.empty((h, w), dtype=torch.uint8, device=dev)
        classes = torch.empty((h, w), dtype=torch.uint8, device=dev)

        def echo_table():
            _native.check(lib.rg_echo_table_f32(P(plane), 0, 1, h, w, 5.0, P(table), table.numel(), s), "rg_echo_table_f32")

        def background():
            _native.check(lib.rg_disk_background(P(table), 1, h, w, c_hw, len(hw) - 1, 0, 0, P(bkg), s), "rg_disk_background")

        def centre_pass():
            _native.check(lib.rg_convective_centres_f32(P(plane), 0, P(bkg), 1, h, w, 5.0, 40.0, 10.0, 180.0, c_edges, K, P(centres), s),
                          "rg_convective_centres_f32")

        def area():
            _native.check(lib.rg_convective_area_u8(P(centres), P(plane), 0, 1, h, w, 5.0, K, rows, ry, P(workspace), ws_bytes,
                                                    P(classes), s), "rg_convective_area_u8")

        def whole_call():
            return rg.convective_stratiform_device(plane, dx=dx, dy=dy, area_relation=RELATION, background_radius=RADIUS)

        for run in (echo_table, background, centre_pass, area):
            run()
        public = whole_call()
        same_public = bool(torch.equal(public, classes))
        host = plane.cpu().numpy()
        t0 = time.perf_counter()
        want, _, _ = co.classify(host, hw, footprints, edges)
        oracle_seconds = time.perf_counter() - t0
        got = classes.cpu().numpy()
        times = alternate({"echo_table": echo_table, "background": background, "centres": centre_pass, "area": area,
                           "whole_call": whole_call}, args.launches, args.warmup, torch)
        span = np.minimum(np.arange(h) + (len(hw) - 1), h - 1) - np.maximum(np.arange(h) - (len(hw) - 1), 0) + 1
        loaded = int(span.sum()) * w * 2 * ENTRY_LOAD_BYTES
        seconds = times["background"]["median_ms"] / 1e3
        results[name] = {"times": times, "public_equals_raw": same_public, "oracle_seconds": round(oracle_seconds, 3),
                         "differing_pixels": int((got != want[0]).sum()),
                         "pixels": {"no_echo": int((got == 0).sum()), "stratiform": int((got == 1).sum()),
                                    "convective": int((got == 2).sum()), "centres": int((centres != 0).sum().item())},
                         "background_loads": {"bytes": loaded, "tb_per_s": round(loaded / seconds / 1e12, 2),
                                              "share_of_l2_gather_rate": [round(loaded / seconds / 1e12 / v, 3) for v in L2_GATHER_TBS[::-1]],
                                              "share_of_l1_peak": round(loaded / seconds / 1e12 / L1_PEAK_TBS, 3),
                                              "compulsory_bytes": int(table.numel()) + 4 * h * w,
                                              "compulsory_tb_per_s": round((int(table.numel()) + 4 * h * w) / seconds / 1e12, 3)}}
    line = {"plane_shape": [h, w], "spacing_m": [dy, dx],
            "settings": {"altitude": ALTITUDE, "background_radius": RADIUS, "relation": RELATION, "ry": len(hw) - 1, "hw_max": max(hw),
                         "class_ry": [len(f) - 1 for f in footprints]},
            "launches": args.launches, "warmup": args.warmup, "device": torch.cuda.get_device_name(dev),
            "unit": "ms; stream events around one call", "planes": results}
    print(json.dumps(line))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--launches", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--processes", type=int, default=3)
    ap.add_argument("--small", action="store_true", help="a 200 x 200 plane: a rehearsal, not a measurement")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "convection_timing.json"))
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
        print(f"[measure_convection] process {len(lines)} of {args.processes} done", file=sys.stderr, flush=True)
    summary = {}
    for name in lines[0]["planes"]:
        per = {}
        for key in lines[0]["planes"][name]["times"]:
            medians = [ln["planes"][name]["times"][key]["median_ms"] for ln in lines]
            per[key] = {"median_ms_per_process": medians, "median_ms": round(float(np.median(medians)), 4),
                        "spread_ms": round(max(medians) - min(medians), 4)}
        per["kernels_ms"] = round(sum(per[k]["median_ms"] for k in ("echo_table", "background", "centres", "area")), 4)
        oracle = [ln["planes"][name]["oracle_seconds"] for ln in lines]
        per["oracle_seconds"] = {"per_process": oracle, "median": round(float(np.median(oracle)), 3)}
        per["ratio_oracle_over_whole_call"] = round(1000.0 * float(np.median(oracle)) / per["whole_call"]["median_ms"], 1)
        per["public_equals_raw"] = [ln["planes"][name]["public_equals_raw"] for ln in lines]
        per["differing_pixels"] = [ln["planes"][name]["differing_pixels"] for ln in lines]
        per["pixels"] = lines[0]["planes"][name]["pixels"]
        per["background_loads"] = [ln["planes"][name]["background_loads"] for ln in lines]
        summary[name] = per
    rec = {"what": "tools/measure_convection.py on one MI355X, %d fresh processes: the %d x %d planes of the bench volume (3 km CAPPI "
                   "and COLMAX, %.1f m pixels), Steiner's relations at the defaults, background radius %.0f m (ry = %d); times in ms "
                   "by stream events around one call, variants alternating, %d launches after %d warm-up rounds. kernels_ms = the "
                   "sum of the four passes; whole_call = convective_stratiform_device with its allocations; oracle_seconds = the "
                   "NumPy restatement of the same chain in the same process, once. background_loads: bytes loaded from the table "
                   "at two entries of 12 loaded bytes per covered row and pixel, read against the %.1f-%.1f TB/s at which 16-byte loads "
                   "are served from L2 chip-wide (measured elsewhere) and against the vector L1's peak of 64 B per clock and CU, "
                   "%.1f TB/s (datasheet, not measured here); the kernel is bound by those loads, not by its compulsory traffic. "
                   "No time is a pass criterion." % (len(lines), *lines[0]["plane_shape"], lines[0]["spacing_m"][1], RADIUS,
                                                      lines[0]["settings"]["ry"], args.launches, args.warmup, *L2_GATHER_TBS,
                                                      L1_PEAK_TBS),
           "summary": summary, "lines": lines}
    with open(args.out, "w") as f:
        json.dump(rec, f, indent=1)
        f.write("\n")
    print(json.dumps(summary, indent=1))
    if any(False in summary[name]["public_equals_raw"] for name in summary):
        sys.exit("the public call and the staged entry points disagree")


if __name__ == "__main__":
    main()
