#!/usr/bin/env python3
"""Cell overlap, relabelling and one tracker step on 2000 x 2000 planes, three fresh processes:

    python tools/measure_tracking.py [--launches 20] [--warmup 3] [--small] [--planes a,b] [--out profiles/tracking_timing.json]

Frames: the COLMAX plane of the bench volume (``tools/measure_components.py`` builds it) against itself moved by (5, -7)
pixels, labelled at 18, 35 and 45 dBZ, and ``one_cell``: both frames all foreground, ONE pair of 4 M pixels -- every wavefront
adds to the same slot, the same-address stress case of the cell table.  Per pair of frames, times in ms by stream events, the
variants alternating, the first ``--warmup`` rounds dropped:

  ``overlap``             rg_cell_overlap_i32 alone (the memsets, the pixel pass, the compaction) with the table sized as
                          ``cell_overlap_device`` sizes it by default: max_pairs = min(pixels, cells_prev * cells_next)
  ``overlap_tight``       the same call with max_pairs = twice the pairs that exist: what the pixel pass costs when the table is
                          small, and so what the default's larger table adds in memset and compaction
  ``cell_overlap_device`` the whole public call: the read of the two cell counts, allocations, the launch, the read of totals,
                          the sort
  ``relabel``             rg_relabel_cells_i32 over the later frame
  ``tracker_update``      one ``CellTracker.update`` of the later frame end to end (label, table, motion estimate and fill,
                          label advection, overlap, match, identities), the earlier frame's update not timed

and ``np.unique`` over the same int64 keys on the host (one run, wall clock), for context.  The parent process only starts the
children (``--child``), collects their JSON lines and writes the summary."""
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

from measure_components import COLMAX_THRESHOLDS, alternate, colmax_plane          # noqa: E402

SHIFT = (5, -7)


def moved(plane, torch):
    """``plane`` moved by ``SHIFT``, NaN moving in."""
    dy, dx = SHIFT
    out = torch.full_like(plane, float("nan"))
    out[dy:, :dx] = plane[:-dy, -dx:]
    return out.contiguous()


def time_tracker(rg, prev, nxt, lo, launches, warmup, torch):
    times = []
    for i in range(warmup + launches):
        tracker = rg.CellTracker(lo)
        tracker.update(prev)
        torch.cuda.synchronize()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        frame = tracker.update(nxt)
        e1.record()
        e1.synchronize()
        if i >= warmup:
            times.append(e0.elapsed_time(e1))
    stats = {"median_ms": round(float(np.median(times)), 4), "min_ms": round(float(np.min(times)), 4),
             "max_ms": round(float(np.max(times)), 4)}
    return stats, frame


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
    shifted = moved(colmax, torch)
    ones = torch.full((h, w), 40.0, dtype=torch.float32, device=dev)
    pairs_of = {f"colmax_{int(t)}dbz": (colmax, shifted, t) for t in COLMAX_THRESHOLDS}
    pairs_of["one_cell"] = (ones, ones.clone(), 35.0)
    if args.planes:
        pairs_of = {k: pairs_of[k] for k in args.planes.split(",")}
    line = {"plane_shape": [h, w], "shift": list(SHIFT), "launches": args.launches, "warmup": args.warmup,
            "device": torch.cuda.get_device_name(dev), "unit": "ms; stream events around one call", "planes": {}}
    for name, (prev, nxt, lo) in pairs_of.items():
        lp, pp = rg.label_components_device(prev, lo)
        ln, pn = rg.label_components_device(nxt, lo)
        cells_prev, cells_next = int(pp[-1].item()), int(pn[-1].item())
        found = rg.cell_overlap_device(lp, pp, ln, pn)
        n_pairs = int(found.count.numel())
        totals = torch.empty(2, dtype=torch.int32, device=dev)

        def raw(max_pairs):
            need = int(lib.rg_cell_overlap_workspace_bytes(max_pairs))
            rows = torch.empty((max_pairs, 2), dtype=torch.int32, device=dev)
            count = torch.empty(max_pairs, dtype=torch.int32, device=dev)
            workspace = torch.empty(need // 8, dtype=torch.int64, device=dev)

            def run():
                _native.check(lib.rg_cell_overlap_i32(P(lp), P(pp), P(ln), P(pn), 1, h, w, max_pairs, P(rows), P(count), P(totals),
                                                      P(workspace), need, s), "rg_cell_overlap_i32")
            run()
            assert totals.cpu().tolist() == [n_pairs, 0], (name, max_pairs, totals.cpu().tolist())
            return run

        default_pairs = max(1, min(h * w, cells_prev * cells_next))
        tight_pairs = max(1, 2 * n_pairs)
        lut = torch.arange(1, cells_next + 1, dtype=torch.int32, device=dev)
        plane_out = torch.empty((h, w), dtype=torch.int32, device=dev)

        def relabel():
            _native.check(lib.rg_relabel_cells_i32(P(ln), P(pn), 1, h, w, P(lut), cells_next, P(plane_out), s), "rg_relabel_cells_i32")

        runs = {"overlap": raw(default_pairs), "overlap_tight": raw(tight_pairs),
                "cell_overlap_device": lambda: rg.cell_overlap_device(lp, pp, ln, pn), "relabel": relabel}
        times = alternate(runs, args.launches, args.warmup, torch)
        times["tracker_update"], frame = time_tracker(rg, prev, nxt, lo, args.launches, args.warmup, torch)
        a, b = lp.cpu().numpy().astype(np.int64).ravel(), ln.cpu().numpy().astype(np.int64).ravel()
        t0 = time.perf_counter()
        both = (a > 0) & (b > 0)
        keys, counts = np.unique(((a[both] - 1) << 32) | (b[both] - 1), return_counts=True)
        unique_ms = round(1e3 * (time.perf_counter() - t0), 2)
        order = np.argsort((found.row_prev.cpu().numpy().astype(np.int64) << 32) | found.row_next.cpu().numpy())
        agree = bool(len(keys) == n_pairs and np.array_equal(counts, found.count.cpu().numpy()[order]))
        line["planes"][name] = {
            "threshold": lo, "cells_prev": cells_prev, "cells_next": cells_next, "pairs": n_pairs,
            "paired_pixels": int(found.count.sum().item()), "largest_pair": int(found.count.max().item()) if n_pairs else 0,
            "max_pairs_default": default_pairs, "max_pairs_tight": tight_pairs,
            "table_bytes_default": int(lib.rg_cell_overlap_workspace_bytes(default_pairs)),
            "table_bytes_tight": int(lib.rg_cell_overlap_workspace_bytes(tight_pairs)),
            "continued_tracks": int((frame.age > 0).sum()), "new_tracks": int((frame.age == 0).sum()),
            "numpy_unique_ms": unique_ms, "numpy_unique_agrees": agree, "times": times}
    print(json.dumps(line))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--launches", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--processes", type=int, default=3)
    ap.add_argument("--small", action="store_true", help="a 200 x 200 plane: a rehearsal, not a measurement")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "tracking_timing.json"))
    ap.add_argument("--planes", default="", help="comma-separated frame pairs to measure (default: all four)")
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
        print(f"[measure_tracking] process {len(lines)} of {args.processes} done", flush=True)
    summary = {}
    for name, first in lines[0]["planes"].items():
        summary[name] = {k: v for k, v in first.items() if k not in ("times", "numpy_unique_ms")}
        for key in first["times"]:
            medians = [ln["planes"][name]["times"][key]["median_ms"] for ln in lines]
            summary[name][key] = {"median_ms_per_process": medians, "median_ms": round(float(np.median(medians)), 4),
                                  "spread_ms": round(max(medians) - min(medians), 4)}
        summary[name]["numpy_unique_ms_per_process"] = [ln["planes"][name]["numpy_unique_ms"] for ln in lines]
    rec = {"what": "tools/measure_tracking.py on one MI355X, %d fresh processes: one %d x %d int32 label plane against the labels of "
                   "the same float32 plane moved by (%d, %d) pixels, times in ms by stream events around one call, variants "
                   "alternating, %d launches after %d warm-up rounds. overlap = rg_cell_overlap_i32 with max_pairs = min(pixels, "
                   "cells_prev * cells_next), overlap_tight = the same with max_pairs = 2 * pairs, cell_overlap_device = the whole "
                   "public call (two host reads, allocations, sort), relabel = rg_relabel_cells_i32, tracker_update = one "
                   "CellTracker.update end to end. numpy_unique_ms: np.unique over the same int64 keys on the host, wall clock, "
                   "one run. `summary` gives, per pair of frames and variant, the median of each process, their median and the "
                   "spread between processes." % (len(lines), *lines[0]["plane_shape"], *SHIFT, args.launches, args.warmup),
           "summary": summary, "lines": lines}
    with open(args.out, "w") as f:
        json.dump(rec, f, indent=1)
        f.write("\n")
    print(json.dumps(summary, indent=1))


if __name__ == "__main__":
    main()
