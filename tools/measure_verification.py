#!/usr/bin/env python3
"""Nowcast verification on a 2000 x 2000 plane, six leads, three fresh processes:

    python tools/measure_verification.py [--launches 20] [--warmup 3] [--small] [--out profiles/verification_timing.json]

The observation: the COLMAX plane of the bench volume (synthetic ``METRIC`` configuration, gridded by
``roi_grid_fields_device``).  The forecast of every one of the 6 leads: the same plane moved by (5, -7) pixels, NaN where
nothing moves in -- the kernels' work does not depend on what the planes hold, only on their number.  Thresholds 18 / 35 /
45 dBZ, window sizes 1, 2, 4, 8, 16, 32, 64.  Times in ms by stream events around one call, the variants alternating, the first
``--warmup`` rounds dropped:

  ``contingency``      rg_contingency_f32 of the 6 pairs
  ``sat``              ONE rg_exceedance_sat_i32 (6 planes x 3 thresholds; a verification takes two)
  ``fss_sums``         rg_fss_sums_i32 over the 18 layers and 7 window sizes
  ``box_fraction``     rg_box_fraction_f32 of the 18 layers at window size 16
  ``verify_nowcast``   the public call end to end: contingency, two tables, the sums, with its allocations
  ``verifier_update``  one NowcastVerifier.update in its steady state: 6 nowcasts and 6 persistence forecasts verified, then
                       the block match, the fill and the 6-lead advection

``host_route_seconds``: the same sums on the host in the same process, once -- one ``scipy.ndimage.uniform_filter`` per (lead,
threshold, window size, field) on the exceedance as float64 plus NumPy for the rest -- and ``host_equals_device`` says whether
its integers are the device's.  No time here is a pass criterion: nothing in the package did this before, the host route is
the yardstick.  The parent process only starts the children (``--child``), collects their JSON lines and writes the summary."""
import argparse
import json
import os
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

SHIFT = (5, -7)
LEADS = 6
THRESHOLDS = (18.0, 35.0, 45.0)
SCALES = (1, 2, 4, 8, 16, 32, 64)
FRACTION_SCALE = 16
B, S, R = 32, 16, 16


def host_route(forecast, observed):
    """int64 ``[L, T, S, 3]`` by scipy's box filter, and the seconds it took; ``(None, None)`` without scipy."""
    try:
        from scipy import ndimage
    except ImportError:
        return None, None
    t0 = time.perf_counter()
    valid = ~np.isnan(forecast) & ~np.isnan(observed)
    sums = np.zeros((len(forecast), len(THRESHOLDS), len(SCALES), 3), dtype=np.int64)
    with np.errstate(invalid="ignore"):
        for lead in range(len(forecast)):
            for t, thr in enumerate(THRESHOLDS):
                fe = (valid[lead] & (forecast[lead] >= np.float32(thr))).astype(np.float64)
                oe = (valid[lead] & (observed[lead] >= np.float32(thr))).astype(np.float64)
                for k, n in enumerate(SCALES):
                    cf = np.rint(ndimage.uniform_filter(fe, size=n, mode="constant", cval=0.0) * (n * n)).astype(np.int64)
                    co = np.rint(ndimage.uniform_filter(oe, size=n, mode="constant", cval=0.0) * (n * n)).astype(np.int64)
                    sums[lead, t, k] = (((cf - co) ** 2).sum(), (cf * cf).sum(), (co * co).sum())
    return sums, time.perf_counter() - t0


def child(args):
    import torch
    import radar_processor_amd as rg
    from measure_components import alternate, colmax_plane
    from radar_processor_amd import _native
    from radar_processor_amd.build import ensure_built
    ensure_built(verbose=False)
    lib = _native.load_library()
    dev = _native.device()
    P, s = _native.ptr, _native.stream_ptr()
    plane = colmax_plane(args.small, torch)
    h, w = (int(v) for v in plane.shape)
    moved = torch.full_like(plane, float("nan"))
    moved[SHIFT[0]:, :SHIFT[1]] = plane[:-SHIFT[0], -SHIFT[1]:]
    forecast = moved.unsqueeze(0).repeat(LEADS, 1, 1).contiguous()
    observed = plane.unsqueeze(0).repeat(LEADS, 1, 1).contiguous()
    T, n_scales, layers = len(THRESHOLDS), len(SCALES), LEADS * len(THRESHOLDS)
    thr = (_native.c_float * T)(*THRESHOLDS)
    scales = (_native.c_int32 * n_scales)(*SCALES)
    counts = torch.empty((LEADS, T, 3), dtype=torch.int64, device=dev)
    valid = torch.empty((LEADS,), dtype=torch.int64, device=dev)
    sat_f = torch.empty((LEADS, T, h, w), dtype=torch.int32, device=dev)
    sat_o = torch.empty_like(sat_f)
    sums = torch.empty((LEADS, T, n_scales, 3), dtype=torch.int64, device=dev)
    fraction = torch.empty((LEADS, T, h, w), dtype=torch.float32, device=dev)

    def contingency():
        _native.check(lib.rg_contingency_f32(P(forecast), P(observed), 0, LEADS, h, w, thr, T, P(counts), P(valid), s),
                      "rg_contingency_f32")

    def sat(src=forecast, partner=observed, out=sat_f):
        _native.check(lib.rg_exceedance_sat_i32(P(src), P(partner), 0, LEADS, h, w, thr, T, P(out), s), "rg_exceedance_sat_i32")

    def fss_sums():
        _native.check(lib.rg_fss_sums_i32(P(sat_f), P(sat_o), layers, h, w, scales, n_scales, P(sums), s), "rg_fss_sums_i32")

    def box_fraction():
        _native.check(lib.rg_box_fraction_f32(P(sat_f), layers, h, w, FRACTION_SCALE, P(fraction), s), "rg_box_fraction_f32")

    def verify_nowcast():
        return rg.verify_nowcast(forecast, observed, THRESHOLDS, SCALES)

    verifier = rg.NowcastVerifier(tuple(range(1, LEADS + 1)), THRESHOLDS, SCALES, block=B, stride=S, search=R)
    flip = {"on": False}

    def verifier_update():
        flip["on"] = not flip["on"]
        verifier.update(moved if flip["on"] else plane)

    for _ in range(LEADS + 1):                            # into the steady state: every lead has a forecast pending
        verifier_update()
    sat(observed, forecast, sat_o)
    sat()
    fss_sums()
    host_sums, host_seconds = host_route(forecast.cpu().numpy(), observed.cpu().numpy())
    same = None if host_sums is None else bool(np.array_equal(host_sums, sums.cpu().numpy()))
    public = verify_nowcast()
    same_public = bool(torch.equal(public.fss.sums, sums))
    runs = {"contingency": contingency, "sat": sat, "fss_sums": fss_sums, "box_fraction": box_fraction,
            "verify_nowcast": verify_nowcast, "verifier_update": verifier_update}
    times = alternate(runs, args.launches, args.warmup, torch)
    score = public.fss.fss()
    line = {"plane_shape": [h, w], "settings": {"leads": LEADS, "thresholds": list(THRESHOLDS), "scales": list(SCALES),
                                                 "shift": list(SHIFT), "fraction_scale": FRACTION_SCALE, "B": B, "S": S, "R": R},
            "launches": args.launches, "warmup": args.warmup, "device": torch.cuda.get_device_name(dev),
            "unit": "ms; stream events around one call", "times": times,
            "host_route_seconds": None if host_seconds is None else round(host_seconds, 3), "host_equals_device": same,
            "public_equals_raw": same_public, "fss_lead0": [[round(float(v), 6) for v in row] for row in score[0]],
            "bytes": {"plane": 4 * h * w, "one_table": 4 * layers * h * w,
                      "sat_compulsory": (2 * LEADS + 2 * layers) * 4 * h * w,
                      "sat_note": "the row pass reads two planes per lead and writes the layers; the column pass reads and "
                                  "writes them once more"}}
    print(json.dumps(line))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--launches", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--processes", type=int, default=3)
    ap.add_argument("--small", action="store_true", help="a 200 x 200 plane: a rehearsal, not a measurement")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "verification_timing.json"))
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
        print(f"[measure_verification] process {len(lines)} of {args.processes} done", file=sys.stderr, flush=True)
    summary = {}
    for key in lines[0]["times"]:
        medians = [ln["times"][key]["median_ms"] for ln in lines]
        summary[key] = {"median_ms_per_process": medians, "median_ms": round(float(np.median(medians)), 4),
                        "spread_ms": round(max(medians) - min(medians), 4)}
    summary["device_sums_ms"] = round(2.0 * summary["sat"]["median_ms"] + summary["fss_sums"]["median_ms"], 4)
    host = [ln["host_route_seconds"] for ln in lines if ln["host_route_seconds"] is not None]
    if host:
        summary["host_route_seconds"] = {"per_process": host, "median": round(float(np.median(host)), 3)}
        summary["ratio_host_over_device_sums"] = round(1000.0 * float(np.median(host)) / summary["device_sums_ms"], 1)
    summary["host_equals_device"] = [ln["host_equals_device"] for ln in lines]
    summary["public_equals_raw"] = [ln["public_equals_raw"] for ln in lines]
    rec = {"what": "tools/measure_verification.py on one MI355X, %d fresh processes: the %d x %d COLMAX plane of the bench volume as "
                   "the observation of %d leads, the forecast of each the same plane moved by %s pixels; thresholds %s dBZ, window "
                   "sizes %s; times in ms by stream events around one call, variants alternating, %d launches after %d warm-up "
                   "rounds. sat = ONE rg_exceedance_sat_i32 of 6 planes x 3 thresholds (a verification takes two); device_sums_ms = "
                   "2 x sat + fss_sums, what the host route computes; host_route_seconds = scipy.ndimage.uniform_filter per (lead, "
                   "threshold, size, field) plus NumPy in the same process, once; verifier_update = one steady-state "
                   "NowcastVerifier.update (12 forecasts verified, then the 6-lead nowcast). No time is a pass criterion."
                   % (len(lines), *lines[0]["plane_shape"], LEADS, list(SHIFT), list(THRESHOLDS), list(SCALES), args.launches,
                      args.warmup),
           "summary": summary, "lines": lines}
    with open(args.out, "w") as f:
        json.dump(rec, f, indent=1)
        f.write("\n")
    print(json.dumps(summary, indent=1))
    if False in summary["host_equals_device"] or False in summary["public_equals_raw"]:
        sys.exit("the host route and the device disagree")


if __name__ == "__main__":
    main()
