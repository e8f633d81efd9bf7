#!/usr/bin/env python3
"""Echo motion and nowcasts on a 2000 x 2000 plane pair, three fresh processes:

    python tools/measure_motion.py [--launches 20] [--warmup 3] [--small] [--out profiles/motion_timing.json]

The pair: the COLMAX plane of the bench volume (synthetic ``METRIC`` configuration, gridded by ``roi_grid_fields_device``) and
the same plane translated by (5, -7) pixels, NaN where nothing moves in.  Settings ``B=32, S=16, R=16``.  Times in ms by stream
events around one call, the variants alternating, the first ``--warmup`` rounds dropped:

  ``quantize``             rg_motion_quantize_f32, both planes in one call
  ``block_match``          rg_block_match_u8 on the levels
  ``fill``                 fill_motion_device (torch elementwise operations on the 124 x 124 lattice)
  ``advect_<method>_<L>``  rg_advect_f32 of one plane, nearest and bilinear, 1 and 6 leads, substeps 1
  ``nowcast_device``       the whole public chain for 6 leads, allocations included

``dot4``: the packed 8-bit dot products the block match needs -- three per dword of every in-plane candidate of every valid
block -- over its time, beside the integer-issue bound of DESIGN.md ("Echo motion and nowcasts": one wave instruction per
SIMD every four cycles, every slot a dot product).  Reported, not asserted.  ``warp_full_*`` of profiles/warp_timing.json,
the warp of a raster of the same size, is copied in as a yardstick for the advection.  The parent process only starts the
children (``--child``), collects their JSON lines and writes the summary."""
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
LEADS6 = (1.0, 2.0, 3.0, 4.0, 5.0, 6.0)


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
    prev = colmax_plane(args.small, torch)
    h, w = (int(v) for v in prev.shape)
    nxt = torch.full_like(prev, float("nan"))
    nxt[SHIFT[0]:, :SHIFT[1]] = prev[:-SHIFT[0], -SHIFT[1]:]
    pair = torch.stack([prev, nxt]).contiguous()
    lat = motion.block_lattice((h, w), B, S)
    levels = torch.empty((2, h, w), dtype=torch.uint8, device=dev)
    disp = torch.empty((1, lat.ny, lat.nx, 2), dtype=torch.int16, device=dev)
    vectors = torch.empty((1, lat.ny, lat.nx, 2), dtype=torch.float32, device=dev)
    score = torch.empty((1, lat.ny, lat.nx), dtype=torch.float32, device=dev)
    inv = float(np.float32(254.0 / 63.5))

    def quantize():
        _native.check(lib.rg_motion_quantize_f32(P(pair), 0, 2, h, w, 0.0, inv, P(levels), s), "rg_motion_quantize_f32")

    def block_match():
        _native.check(lib.rg_block_match_u8(P(levels[0]), P(levels[1]), 1, h, w, B, S, R, B * B // 8, P(disp), P(vectors), P(score),
                                            s), "rg_block_match_u8")
    quantize()
    block_match()
    grid = motion.MotionGrid(vectors[0], score[0], disp[0], B, S, R, (h, w), lat.origin_y, lat.step_y)
    filled = rg.fill_motion_device(grid)
    field = filled.motion
    outs = {n: torch.empty((n, 1, h, w), dtype=torch.float32, device=dev) for n in (1, 6)}
    c_leads = (_native.c_double * 6)(*LEADS6)
    c_lat = _native.MotionLattice(*lat)

    def advect(method, n):
        def run():
            _native.check(lib.rg_advect_f32(P(nxt), 1, h, w, P(field), c_lat, c_leads, n, 1, method, float("nan"), P(outs[n]), s),
                          "rg_advect_f32")
        return run
    runs = {"quantize": quantize, "block_match": block_match, "fill": lambda: rg.fill_motion_device(grid),
            "advect_nearest_1": advect(0, 1), "advect_nearest_6": advect(0, 6), "advect_bilinear_1": advect(1, 1),
            "advect_bilinear_6": advect(1, 6),
            "nowcast_device": lambda: rg.nowcast_device(prev, nxt, LEADS6, block=B, stride=S, search=R)}
    times = alternate(runs, args.launches, args.warmup, torch)
    # the work of the block match: three dot products per dword of every in-plane candidate of every block with a vector
    live = ~torch.isnan(score[0]).cpu().numpy()
    ys, xs = np.arange(lat.ny) * S, np.arange(lat.nx) * S
    inside_y = np.minimum(ys + R, h - B) - np.maximum(ys - R, 0) + 1
    inside_x = np.minimum(xs + R, w - B) - np.maximum(xs - R, 0) + 1
    candidates = int((inside_y[:, None] * inside_x[None, :])[live].sum())
    dot4 = 3 * (B * B // 4) * candidates
    props = torch.cuda.get_device_properties(dev)
    cus = int(props.multi_processor_count)
    mhz = float(getattr(props, "clock_rate", 2400000)) / 1e3
    bound = cus * 4 * 16 * mhz * 1e6                      # lane-level dot4 per second: 4 SIMDs x 16 lanes per CU and cycle
    rate = dot4 / (times["block_match"]["median_ms"] * 1e-3)
    good = live & (np.abs(vectors[0].cpu().numpy() - np.array(SHIFT, dtype=np.float32)).max(axis=-1) <= 0.5)
    line = {"plane_shape": [h, w], "settings": {"B": B, "S": S, "R": R, "shift": list(SHIFT)}, "launches": args.launches,
            "warmup": args.warmup, "device": torch.cuda.get_device_name(dev), "unit": "ms; stream events around one call",
            "lattice": [lat.ny, lat.nx], "blocks_with_a_vector": int(live.sum()), "vectors_within_half_a_pixel_of_the_shift": int(good.sum()),
            "echo_fraction": round(float((levels[0] != 0).float().mean().item()), 4), "times": times,
            "dot4": {"candidates": candidates, "lane_dot4": dot4, "multiply_adds": 4 * dot4, "compute_units": cus, "clock_mhz": mhz,
                     "lane_dot4_per_s": rate, "issue_bound_lane_dot4_per_s": bound, "fraction_of_issue_bound": round(rate / bound, 4)}}
    print(json.dumps(line))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--launches", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--processes", type=int, default=3)
    ap.add_argument("--small", action="store_true", help="a 200 x 200 plane: a rehearsal, not a measurement")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "motion_timing.json"))
    ap.add_argument("--child", action="store_true", help=argparse.SUPPRESS)
    args = ap.parse_args()
    if args.child:
        return child(args)
    cmd = [sys.executable, os.path.abspath(__file__), "--child", "--launches", str(args.launches), "--warmup", str(args.warmup)]
    cmd += ["--small"] if args.small else []
    lines = []
    for _ in range(args.processes):                       # one after another: a fresh process each, never two on the GPU
        done = subprocess.run(cmd, check=True, capture_output=True, text=True, timeout=300)
        lines.append(json.loads(done.stdout.strip().splitlines()[-1]))
    summary = {}
    for key in lines[0]["times"]:
        medians = [ln["times"][key]["median_ms"] for ln in lines]
        summary[key] = {"median_ms_per_process": medians, "spread_ms": round(max(medians) - min(medians), 4)}
    summary["dot4_fraction_of_issue_bound_per_process"] = [ln["dot4"]["fraction_of_issue_bound"] for ln in lines]
    yardstick = {}
    try:
        with open(os.path.join(ROOT, "profiles", "warp_timing.json")) as f:
            warp = json.load(f)
        yardstick = {"raster": warp["full_raster"][3:], "median_ms": {k: v["median_ms"] for k, v in warp["results"].items()
                                                                      if k in ("warp_full_nearest_1p", "warp_full_bilinear_1p")}}
    except (OSError, KeyError, ValueError):
        pass
    rec = {"what": "tools/measure_motion.py on one MI355X, %d fresh processes: the %d x %d COLMAX plane of the bench volume paired "
                   "with itself translated by %s pixels, B=%d S=%d R=%d; times in ms by stream events around one call, variants "
                   "alternating, %d launches after %d warm-up rounds. quantize = both planes in one rg_motion_quantize_f32, "
                   "block_match = rg_block_match_u8, fill = fill_motion_device, advect_<method>_<leads> = rg_advect_f32 of one "
                   "plane, nowcast_device = the public chain for 6 leads with its allocations. dot4: the packed dot products of "
                   "the block match over its time against the integer-issue bound of DESIGN.md (reported, not asserted). "
                   "warp_yardstick: profiles/warp_timing.json's warp of a raster of about this size (not a gate)."
                   % (len(lines), *lines[0]["plane_shape"], list(SHIFT), B, S, R, args.launches, args.warmup),
           "summary": summary, "warp_yardstick": yardstick, "lines": lines}
    with open(args.out, "w") as f:
        json.dump(rec, f, indent=1)
        f.write("\n")
    print(json.dumps(summary, indent=1))


if __name__ == "__main__":
    main()
