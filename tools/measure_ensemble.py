#!/usr/bin/env python3
"""Ensemble exceedance probabilities and their verification counts on a 2000 x 2000 plane pair, three fresh processes:

    python tools/measure_ensemble.py [--launches 20] [--warmup 3] [--small] [--out profiles/ensemble_timing.json]

The pair: the COLMAX plane of the bench volume (synthetic ``METRIC`` configuration, gridded by ``roi_grid_fields_device``) and
the same plane translated by (5, -7) pixels, NaN where nothing moves in.  The motion is the block match at its defaults
(``B=32, S=16, R=16``), filled.  20 members perturbed along the mean motion, 6 leads, thresholds 18 / 35 / 45 dBZ.  Times in ms
by stream events around one call, the variants alternating, the first ``--warmup`` rounds dropped:

  ``fused_<method>``        rg_ensemble_exceedance_f32, nearest and bilinear, writing prob, counts and members into buffers kept
  ``fused_<method>_prob``   the same writing prob only
  ``histogram``             rg_ensemble_histogram_u8 of the six leads against six observation planes
  ``composed_<method>``     what the fused call replaces: 20 ``advect_device`` calls of the six leads into ONE reused buffer (so the
                            120 member planes are never all resident: the composition at its cheapest), each followed by a torch
                            ``>=`` per threshold and a sum into the counts, then the division.  The members' motion fields are
                            identical -- this leg is for cost only.

``ratio_composed_over_fused`` above 1 means the fused kernel is faster.  No ratio is required: the numbers are reported as
measured.  ``bytes``: what each route must move at the least, computed from the shapes.  With all shifts zero the two routes
are compared once per process (equal counts).  The parent process only starts the children (``--child``), collects their JSON
lines and writes the summary."""
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
MEMBERS = 20
LEADS = (1.0, 2.0, 3.0, 4.0, 5.0, 6.0)
THRESHOLDS = (18.0, 35.0, 45.0)
PAR, PERP = (0.6, 0.5, 0.2), (0.3, 0.5, 0.1)          # pixels per interval: a spread of a few pixels at the last lead
METHODS = ("nearest", "bilinear")


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
    grid = rg.fill_motion_device(rg.estimate_motion_device(prev, nxt, block=B, stride=S, search=R))
    field, lat = grid.motion.contiguous(), grid.lattice
    c_lat = _native.MotionLattice(*lat)
    direction = field.to(torch.float64).mean(dim=(0, 1)).cpu().numpy()
    shifts_host = rg.motion_perturbations(MEMBERS, LEADS, direction=direction, par=PAR, perp=PERP, seed=1)
    shifts = torch.from_numpy(shifts_host).to(dev)
    zero_shifts = torch.zeros_like(shifts)
    L, T = len(LEADS), len(THRESHOLDS)
    c_leads, c_thr = (_native.c_double * L)(*LEADS), (_native.c_float * T)(*THRESHOLDS)
    prob = torch.empty((L, T, h, w), dtype=torch.float32, device=dev)
    counts = torch.empty((L, T, h, w), dtype=torch.uint8, device=dev)
    members = torch.empty((L, h, w), dtype=torch.uint8, device=dev)
    hist = torch.empty((L, T, MEMBERS + 1, 2), dtype=torch.int64, device=dev)
    valid = torch.empty((L,), dtype=torch.int64, device=dev)
    obs = torch.stack([torch.roll(nxt, (SHIFT[0] * (k + 1), SHIFT[1] * (k + 1)), dims=(0, 1)) for k in range(L)]).contiguous()
    member_planes = torch.empty((L, h, w), dtype=torch.float32, device=dev)
    thr_t = torch.tensor(THRESHOLDS, dtype=torch.float32, device=dev)[None, :, None, None]

    def fused(method, sh=shifts, everything=True):
        def run():
            _native.check(lib.rg_ensemble_exceedance_f32(P(nxt), h, w, P(field), c_lat, c_leads, L, 1, motion.ADVECT_METHODS[method],
                                                         P(sh), MEMBERS, c_thr, T, 1, P(prob), P(counts) if everything else None,
                                                         P(members) if everything else None, None, s), "rg_ensemble_exceedance_f32")
        return run

    def histogram():
        _native.check(lib.rg_ensemble_histogram_u8(P(counts), P(members), P(obs), None, L, h, w, MEMBERS, c_thr, T, P(hist), P(valid), s),
                      "rg_ensemble_histogram_u8")

    def composed(method):
        def run():
            cnt = torch.zeros((L, T, h, w), dtype=torch.uint8, device=dev)
            n = torch.zeros((L, h, w), dtype=torch.uint8, device=dev)
            for _ in range(MEMBERS):
                rg.advect_device(nxt, field, LEADS, lattice=tuple(lat), method=method, out=member_planes)
                cnt += member_planes[:, None] >= thr_t
                n += ~torch.isnan(member_planes)
            p = torch.where(n[:, None] >= 1, cnt.to(torch.float32) / n[:, None].clamp(min=1).to(torch.float32), float("nan"))
            return p, cnt, n
        return run

    agreement = {}
    for method in METHODS:                                  # zero shifts: the composition's identical members ARE the ensemble
        fused(method, zero_shifts)()
        _, cnt, n = composed(method)()
        agreement[method] = {"equal_counts": bool(torch.equal(cnt, counts)), "equal_members": bool(torch.equal(n, members))}
    runs = {}
    for method in METHODS:
        runs["fused_" + method] = fused(method)
        runs["fused_" + method + "_prob"] = fused(method, everything=False)
        runs["composed_" + method] = composed(method)
    fused("nearest")()                                      # the histogram's inputs: the perturbed ensemble
    runs["histogram"] = histogram
    times = alternate(runs, args.launches, args.warmup, torch)
    histogram()
    torch.cuda.synchronize()
    plane_bytes = 4 * h * w
    line = {"plane_shape": [h, w], "settings": {"B": B, "S": S, "R": R, "shift": list(SHIFT), "members": MEMBERS, "leads": list(LEADS),
                                                "thresholds": list(THRESHOLDS), "par": list(PAR), "perp": list(PERP), "substeps": 1,
                                                "largest_shift_px": round(float(np.abs(shifts_host).max()), 2)},
            "launches": args.launches, "warmup": args.warmup, "device": torch.cuda.get_device_name(dev),
            "unit": "ms; stream events around one call", "lattice": [lat.ny, lat.nx], "times": times, "agreement": agreement,
            "complete_fraction": round(float((members == MEMBERS).float().mean().item()), 4),
            "histogram_valid": [int(v) for v in valid.cpu()],
            "bytes": {"plane": plane_bytes,
                      "fused_compulsory": plane_bytes + L * T * h * w * 5 + L * h * w,
                      "composed_compulsory": MEMBERS * (plane_bytes + L * plane_bytes) + MEMBERS * L * plane_bytes + L * T * h * w * 5,
                      "note": "fused: one plane in, prob (4 bytes), counts (1) and members (1) out; composed: every member writes "
                              "its six planes and reads them back once; torch's intermediates come on top"}}
    print(json.dumps(line))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--launches", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--processes", type=int, default=3)
    ap.add_argument("--small", action="store_true", help="a 200 x 200 plane: a rehearsal, not a measurement")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "ensemble_timing.json"))
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
    summary["ratio_composed_over_fused"] = {m: round(summary["composed_" + m]["median_ms"] / summary["fused_" + m]["median_ms"], 3)
                                            for m in METHODS}
    rec = {"what": "tools/measure_ensemble.py on one MI355X, %d fresh processes: the %d x %d COLMAX plane of the bench volume paired "
                   "with itself translated by %s pixels; block-match motion at B=%d S=%d R=%d, filled; %d members, %d leads, "
                   "thresholds %s dBZ, substeps 1; times in ms by stream events around one call, variants alternating, %d launches "
                   "after %d warm-up rounds. fused_<method> = rg_ensemble_exceedance_f32 writing prob, counts and members; "
                   "fused_<method>_prob = prob only; histogram = rg_ensemble_histogram_u8 of the six leads; composed_<method> = %d "
                   "advect_device calls of the six leads into one reused buffer, each with a torch >= and sum. "
                   "ratio_composed_over_fused above 1: the fused kernel is faster."
                   % (len(lines), *lines[0]["plane_shape"], list(SHIFT), B, S, R, MEMBERS, len(LEADS), list(THRESHOLDS), args.launches,
                      args.warmup, MEMBERS),
           "summary": summary, "lines": lines}
    with open(args.out, "w") as f:
        json.dump(rec, f, indent=1)
        f.write("\n")
    print(json.dumps(summary, indent=1))


if __name__ == "__main__":
    main()
