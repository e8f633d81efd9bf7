"""Times the velocity dealiasing (include/radargrid_velocity.h) on one GPU and writes profiles/velocity_timing.json.

    python tools/measure_velocity.py [--out profiles/velocity_timing.json] [--launches 20] [--warmup 3] [--repeat 20] [--skip-oracle]

A synthetic volume of 12 sweeps x 360 rays x 1000 gates (the bench volume's shape): a wind that veers and strengthens with
height, folded into each sweep's Nyquist interval, 2 % of the gates missing at random and one sector without echo per sweep.
``smooth`` has no noise; ``noisy`` adds sigma = 0.7 m/s, which breaks every band border into thousands of small regions -- the
load the host merge has to carry.  For each call of the chain through the raw C ABI (split, the labeller and the stats call of
radargrid_hip.h as the chain uses them, regions, edges, apply): the median of ``launches`` samples after ``warmup`` rounds, a
sample being ``repeat`` back-to-back calls between two stream events, divided by ``repeat``, the kinds of sample alternating.
``merge_ms``: ``merge_regions`` on the host, on the table the device produced.  ``chain_ms``: ``dealias_velocity_device`` end to
end by the host clock around a device synchronise, allocations, both host synchronisations and the merge included.  For the edge
call also the share of its bytes-moved bound: 8 bytes per gate (a value and a region id) at the 8 TB/s HBM peak.
``numpy_seconds``: the restatement (tests/velocity_oracle.py) of the same work in the same process, once, on ``smooth`` only (its
merge is a scan per step), and whether every output of the device equals it.  No time is a pass criterion."""
import argparse
import ctypes
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

HBM_PEAK = 8.0e12
S, R, G, BANDS = 12, 360, 1000, 3
FLT_MAX = float(np.finfo(np.float32).max)


def volume(noise, seed=12):
    rng = np.random.default_rng(seed)
    az = 2.0 * np.pi * np.arange(R) / R
    nyq = np.linspace(9.0, 16.0, S)
    vel = np.empty((S, R, G), np.float32)
    for s in range(S):
        speed, direction = 18.0 + 2.0 * s, 0.7 + 0.1 * s
        truth = speed * np.cos(az - direction)[:, None] * np.linspace(0.5, 1.0, G)[None, :]
        if noise:
            truth = truth + rng.normal(0.0, noise, (R, G))
        vn = nyq[s]
        vel[s] = (truth - 2.0 * vn * np.floor((truth + vn) / (2.0 * vn))).astype(np.float32)
        vel[s, (40 + 25 * s) % R:(40 + 25 * s) % R + 12, 300 + 40 * s:] = np.nan             # a sector without echo
    vel[rng.random((S, R, G)) < 0.02] = np.nan
    return vel, nyq


def measure(name, noise, args, with_oracle):
    import torch
    import radar_processor_amd as rg
    from radar_processor_amd import _native, velocity
    lib = rg.load_library()
    dev = torch.device("cuda", 0)
    host_vel, nyq = volume(noise)
    vel = torch.from_numpy(host_vel).to(dev)
    c_nyq = (ctypes.c_double * S)(*nyq.tolist())
    P, n = _native.ptr, S * R * G
    stack = (S * BANDS, R, G)

    def check(status):
        if status != 0:
            raise RuntimeError(lib.rg_last_error().decode())

    # one eager chain gives the sizes every standing buffer needs
    first = rg.dealias_velocity_device(vel, nyq, n_bands=BANDS)
    n_regions, n_edges = first.n_regions, first.n_edges
    max_edges = velocity.default_max_edges(n_regions)
    split = torch.empty((S, BANDS, R, G), dtype=torch.float32, device=dev)
    labels = torch.empty(stack, dtype=torch.int32, device=dev)
    cell_ptr = torch.empty(S * BANDS + 1, dtype=torch.int32, device=dev)
    label_bytes = int(lib.rg_components_workspace_bytes(*stack))
    label_ws = torch.empty(max(label_bytes, 16), dtype=torch.uint8, device=dev)
    sizes = torch.empty(n_regions, dtype=torch.int32, device=dev)
    regions = torch.empty((S, R, G), dtype=torch.int32, device=dev)
    edge_bytes = int(lib.rg_region_edges_workspace_bytes(max_edges))
    pair_ids = torch.empty((max_edges, 2), dtype=torch.int32, device=dev)
    pair_count = torch.empty(max_edges, dtype=torch.int32, device=dev)
    pair_sum = torch.empty(max_edges, dtype=torch.int64, device=dev)
    totals = torch.empty(2, dtype=torch.int32, device=dev)
    edge_ws = torch.empty(edge_bytes // 8, dtype=torch.int64, device=dev)
    lut = torch.zeros(n_regions, dtype=torch.int32, device=dev)
    out = torch.empty((S, R, G), dtype=torch.float32, device=dev)
    folds = torch.empty((S, R, G), dtype=torch.int32, device=dev)
    stream = _native.stream_ptr
    calls = {
        "split": lambda: check(lib.rg_velocity_split_f32(P(vel), None, S, R, G, c_nyq, BANDS, P(split), stream())),
        "label": lambda: check(lib.rg_label_components_f32(P(split), None, *stack, -FLT_MAX, float("inf"), 4, 1, P(labels), P(cell_ptr),
                                                           P(label_ws), label_bytes, stream())),
        "stats": lambda: check(lib.rg_component_stats_f32(P(split), P(labels), P(cell_ptr), *stack, n_regions, P(sizes), None, None, None,
                                                          None, None, stream())),
        "regions": lambda: check(lib.rg_velocity_regions_i32(P(labels), P(cell_ptr), S, R, G, BANDS, P(regions), stream())),
        "edges": lambda: check(lib.rg_region_edges_f32(P(vel), P(regions), S, R, G, 1, max_edges, P(pair_ids), P(pair_count), P(pair_sum),
                                                       P(totals), P(edge_ws), edge_bytes, stream())),
        "apply": lambda: check(lib.rg_velocity_apply_folds_f32(P(vel), P(regions), P(lut), n_regions, S, R, G, c_nyq, P(out), P(folds),
                                                               stream())),
    }
    bytes_per_gate = {"split": 4 + 4 * BANDS, "label": None, "stats": None, "regions": 4 * BANDS + 4, "edges": 8, "apply": 4 + 4 + 4 + 4}
    for call in calls.values():                                  # in the order of the chain: each finds its inputs written
        call()
    torch.cuda.synchronize()
    assert totals.cpu().tolist() == [n_edges, 0]
    times = {key: [] for key in calls}
    for round_ in range(args.warmup + args.launches):
        for key, call in calls.items():
            start, stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            start.record()
            for _ in range(args.repeat):
                call()
            stop.record()
            stop.synchronize()
            if round_ >= args.warmup:
                times[key].append(start.elapsed_time(stop) / args.repeat)
    result = {"sweeps": S, "rays": R, "gates": G, "n_bands": BANDS, "noise_sigma": noise, "valid_gates": int(np.isfinite(host_vel).sum()),
              "n_regions": n_regions, "n_edges": n_edges, "max_edges": max_edges, "calls": {}}
    for key, ms in times.items():
        median = float(np.median(ms))
        entry = {"median_ms": round(median, 4), "min_ms": round(min(ms), 4), "max_ms": round(max(ms), 4)}
        if bytes_per_gate[key]:
            moved = bytes_per_gate[key] * n
            entry.update(bytes_moved=moved, share_of_bytes_bound=round(moved / HBM_PEAK / (median * 1e-3), 4))
        result["calls"][key] = entry
    # the host merge on the table the device produced
    rows = torch.cat((pair_ids[:n_edges].long(), pair_count[:n_edges].long()[:, None], pair_sum[:n_edges, None]), dim=1).cpu().numpy()
    intervals = velocity.region_intervals(cell_ptr.cpu().numpy(), nyq.tolist(), BANDS)
    host_sizes = sizes.cpu().numpy()
    merge_ms = []
    for _ in range(3):
        t0 = time.perf_counter()
        velocity.merge_regions(rows, host_sizes, intervals)
        merge_ms.append((time.perf_counter() - t0) * 1e3)
    result["merge_ms"] = round(float(np.median(merge_ms)), 3)
    chain_ms = []
    for round_ in range(1 + args.chains):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        got = rg.dealias_velocity_device(vel, nyq, n_bands=BANDS)
        torch.cuda.synchronize()
        if round_ >= 1:
            chain_ms.append((time.perf_counter() - t0) * 1e3)
    result["chain_ms"] = {"median_ms": round(float(np.median(chain_ms)), 3), "min_ms": round(min(chain_ms), 3), "max_ms": round(max(chain_ms), 3)}
    result["gates_with_a_fold"] = int((got.folds != 0).sum().item())
    if with_oracle:
        import velocity_oracle as vo
        seconds = {}
        t0 = time.perf_counter()
        reg = vo.regions(host_vel, nyq, BANDS, None, True)
        seconds["regions"] = time.perf_counter() - t0
        t0 = time.perf_counter()
        e = vo.edges(host_vel, reg.regions, True)
        seconds["edges"] = time.perf_counter() - t0
        t0 = time.perf_counter()
        table = vo.merge(e, reg.sizes, vo.region_intervals(reg.cell_ptr, nyq, BANDS))
        seconds["merge"] = time.perf_counter() - t0
        t0 = time.perf_counter()
        want, want_folds = vo.apply(host_vel, reg.regions, table, nyq)
        seconds["apply"] = time.perf_counter() - t0
        seconds["chain"] = sum(seconds.values())
        result["numpy_seconds"] = {key: round(value, 3) for key, value in seconds.items()}
        result["differing_gates"] = {"regions": int((got.regions.cpu().numpy() != reg.regions).sum()),
                                     "folds": int((got.folds.cpu().numpy() != want_folds).sum()),
                                     "velocity": int((vo.bits(got.velocity.cpu().numpy()) != vo.bits(want)).sum())}
        result["edge_rows_equal"] = bool(np.array_equal(rows[np.lexsort((rows[:, 1], rows[:, 0]))], e))
        result["ratio_numpy_over_device_chain"] = round(1000.0 * seconds["chain"] / result["chain_ms"]["median_ms"], 1)
    print(json.dumps({name: result}), flush=True)
    return result


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "velocity_timing.json"))
    ap.add_argument("--launches", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--repeat", type=int, default=20, help="back-to-back calls between the two events of one sample")
    ap.add_argument("--chains", type=int, default=7, help="end-to-end chains timed after one warm-up")
    ap.add_argument("--skip-oracle", action="store_true")
    args = ap.parse_args()
    import torch
    record = {"what": "tools/measure_velocity.py on one MI355X, one process: a synthetic volume of 12 sweeps x 360 rays x 1000 gates (a wind that "
                      "veers and strengthens with height, Nyquist velocities 9 .. 16 m/s, 2 % of the gates missing at random, one sector "
                      "without echo per sweep), three bands, rays wrapping; `smooth` without noise, `noisy` with sigma = 0.7 m/s.  "
                      f"calls.*.median_ms: per call through the raw C ABI into standing buffers, from {args.repeat} back-to-back calls "
                      f"between two stream events, the kinds of sample alternating, {args.launches} samples after {args.warmup} warm-up "
                      "rounds (the whole working set fits the 256 MiB Infinity Cache, so a call finds its inputs cache-warm); label "
                      "and stats are the calls of radargrid_hip.h as the chain makes them; edges is the clear, the pass and the "
                      "compaction together.  share_of_bytes_bound: the bytes the call has to move (edges: 8 per gate, a value and a "
                      "region id, although the kernel reads values only where regions meet) at the 8 TB/s HBM peak, over the time.  "
                      "merge_ms: merge_regions on the host over the device's table, median of 3.  chain_ms: dealias_velocity_device by "
                      f"the host clock around a device synchronise, {args.chains} chains after one warm-up, allocations, both host "
                      "synchronisations and the merge included.  "
                      "numpy_seconds: tests/velocity_oracle.py on the same arrays in the same process, once (smooth only); "
                      "differing_gates: gates at which an output of the device differs from it.  No time is a pass criterion.",
              "device": torch.cuda.get_device_name(0), "volumes": {}}
    record["volumes"]["smooth"] = measure("smooth", 0.0, args, not args.skip_oracle)
    record["volumes"]["noisy"] = measure("noisy", 0.7, args, False)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(record, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
