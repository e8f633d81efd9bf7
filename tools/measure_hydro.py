"""Times the hydrometeor classification (include/radargrid_hydro.h) on one GPU and writes profiles/hydro_timing.json.

    python tools/measure_hydro.py [--out profiles/hydro_timing.json] [--launches 20] [--warmup 3] [--repeat 50] [--skip-oracle]

The two volumes of tools/measure_phase.py -- the bench volume's 4320 rays x 1000 gates and C4's 10080 x 2000 -- as synthetic
dual-polarisation rays: rain cells along every ray, a stretch of clutter near the radar, a melting layer in the per-sweep
temperature, 5 % NaN, 3 % masked.  The preset table (980 cells).  For the two textures and the classifier through the raw C ABI and
for the chain (``classify_hydrometeors_device``, allocations included): the median of ``launches`` samples after ``warmup`` rounds,
a sample being ``repeat`` back-to-back calls between two stream events, divided by ``repeat``, the four kinds of sample
alternating; the bytes the call has to move (texture: 4 in and 4 per output; classifier: 4 per variable read per gate plus 1 to 6
out; the mask is 1 more where there is one); those bytes over the time, as a share of the 8 TB/s HBM peak.  ``numpy_seconds``:
the NumPy restatement (tests/hydro_oracle.py) of the same work in the same process, once, and whether every output of the device
equals it bit for bit.  No time is a pass criterion."""
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
HALF_Z, HALF_P, SWEEPS = 2, 4, 12
VOLUMES = {"bench_4320x1000": (4320, 1000), "c4_10080x2000": (10080, 2000)}
# texture: x and the mask in, sd out.  classifier: six per-gate variables and the mask in (T is one row per sweep: nothing per
# gate), cls, score and second out.  chain: both textures, then the classifier.
BYTES_PER_GATE = {"texture_z": 4 + 1 + 4, "texture_phidp": 4 + 1 + 4, "classify": 6 * 4 + 1 + 1 + 4 + 1}
BYTES_PER_GATE["chain"] = sum(BYTES_PER_GATE.values())


def volume(R, G, seed):
    rng = np.random.default_rng(seed)
    x = np.arange(G)[None, :]
    rain = np.zeros((R, G), np.float32)
    for level, width in ((1.0, G // 8), (2.0, G // 20), (3.0, G // 40)):
        start = rng.integers(G // 10, G - G // 5, size=(R, 1))
        rain[(x >= start) & (x < start + width)] = level
    dbz = (12.0 + 14.0 * rain + rng.normal(0.0, 1.5, (R, G))).astype(np.float32)
    zdr = (0.2 + 0.6 * rain + rng.normal(0.0, 0.15, (R, G))).astype(np.float32)
    kdp = (0.05 + 0.6 * rain * rain / 3.0 + rng.normal(0.0, 0.05, (R, G))).astype(np.float32)
    rhohv = np.clip(0.985 + rng.normal(0.0, 0.008, (R, G)), 0.0, 1.0).astype(np.float32)
    phidp = (60.0 + np.cumsum(2.0 * np.maximum(kdp, 0.0) * 0.24, axis=1) + rng.normal(0.0, 3.0, (R, G))).astype(np.float32)
    clutter = x < G // 25                                                 # near the radar: noisy, decorrelated
    dbz[:, :G // 25] += rng.normal(10.0, 8.0, (R, G // 25)).astype(np.float32)
    rhohv[:, :G // 25] = rng.uniform(0.4, 0.9, (R, G // 25)).astype(np.float32)
    phidp[:, :G // 25] += rng.normal(0.0, 40.0, (R, G // 25)).astype(np.float32)
    assert clutter.any()
    for a in (dbz, zdr, kdp, rhohv, phidp):
        a[rng.random((R, G)) < 0.05] = np.nan
    mask = (rng.random((R, G)) < 0.03).astype(np.uint8)
    return dict(dbz=dbz, zdr=zdr, kdp=kdp, rhohv=rhohv, phidp=phidp, mask=mask)


def measure(name, R, G, args):
    import torch
    import radar_processor_amd as rg
    from radar_processor_amd import _native
    import hydro_oracle as ho
    lib = rg.load_library()
    dev = torch.device("cuda", 0)
    table = rg.HYDROMETEOR_TABLE_S_BAND
    host = volume(R, G, seed=R + G)
    elevations = np.linspace(0.5, 19.5, SWEEPS)
    temperature = rg.beam_temperature(elevations, 240.0 * (0.5 + np.arange(G)), [0.0, 4000.0, 12000.0], [24.0, 0.0, -52.0])
    t = {key: torch.from_numpy(a).to(dev) for key, a in host.items()}
    t["temperature"] = torch.from_numpy(temperature).to(dev)
    new = lambda dtype: torch.empty((R, G), dtype=dtype, device=dev)                      # noqa: E731
    sd_z, sd_p, cls, score, second = new(torch.float32), new(torch.float32), new(torch.uint8), new(torch.float32), new(torch.uint8)
    cells = table.device_cells(dev)
    P, V = _native.ptr, table.n_vars
    c_vars = (ctypes.c_void_p * V)(P(t["dbz"]), P(t["zdr"]), P(t["kdp"]), P(t["rhohv"]), P(sd_z), P(sd_p), P(t["temperature"]))
    c_kinds = (ctypes.c_int32 * V)(*table.kinds)
    c_edges = (ctypes.c_double * len(table.edges))(*table.edges)
    c_weights = (ctypes.c_double * (table.n_classes * V))(*table.weights.reshape(-1).tolist())

    def check(status):
        if status != 0:
            raise RuntimeError(lib.rg_last_error().decode())

    calls = {
        "texture_z": lambda: check(lib.rg_polar_texture_f32(P(t["dbz"]), P(t["mask"]), R, G, HALF_Z, HALF_Z + 1, 0, P(sd_z), None, None,
                                                            _native.stream_ptr())),
        "texture_phidp": lambda: check(lib.rg_polar_texture_f32(P(t["phidp"]), P(t["mask"]), R, G, HALF_P, HALF_P + 1, 0, P(sd_p), None, None,
                                                                _native.stream_ptr())),
        "classify": lambda: check(lib.rg_fuzzy_classify_f32(c_vars, c_kinds, V, 1 << 6, table.required_bits, R // SWEEPS, P(t["mask"]), R, G,
                                                            table.cond_var, c_edges, table.n_bins, P(cells), table.n_classes, c_weights, 0.0,
                                                            P(cls), P(score), P(second), _native.stream_ptr())),
        "chain": lambda: rg.classify_hydrometeors_device(t["dbz"], t["zdr"], t["kdp"], t["rhohv"], phidp=t["phidp"],
                                                         temperature=t["temperature"], mask=t["mask"],
                                                         texture_half_gates=(HALF_Z, HALF_P)),
    }
    times = {key: [] for key in calls}
    for round_ in range(args.warmup + args.launches):
        for key, call in calls.items():
            start, stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            start.record()
            for _ in range(args.repeat):             # back to back: one call is tens of microseconds, an event pair resolves less
                call()
            stop.record()
            stop.synchronize()
            if round_ >= args.warmup:
                times[key].append(start.elapsed_time(stop) / args.repeat)
    result = {"rays": R, "gates": G, "sweeps": SWEEPS, "cells": int(table.cells.size // 6), "calls": {}}
    for key, ms in times.items():
        median = float(np.median(ms))
        moved = BYTES_PER_GATE[key] * R * G
        result["calls"][key] = {"median_ms": round(median, 4), "min_ms": round(min(ms), 4), "max_ms": round(max(ms), 4),
                                "bytes_moved": moved, "tb_per_s": round(moved / (median * 1e-3) / 1e12, 3),
                                "share_of_hbm_peak": round(moved / (median * 1e-3) / HBM_PEAK, 3)}
    if not args.skip_oracle:
        got = rg.classify_hydrometeors_device(t["dbz"], t["zdr"], t["kdp"], t["rhohv"], phidp=t["phidp"], temperature=t["temperature"],
                                              mask=t["mask"], texture_half_gates=(HALF_Z, HALF_P))
        got = {field: getattr(got, field).cpu().numpy() for field in got._fields}
        spec, seconds = ho.spec_of(table), {}
        t0 = time.perf_counter()
        want_z = ho.texture(host["dbz"], host["mask"], HALF_Z, HALF_Z + 1, 0).sd
        seconds["texture_z"] = time.perf_counter() - t0
        t0 = time.perf_counter()
        want_p = ho.texture(host["phidp"], host["mask"], HALF_P, HALF_P + 1, 0).sd
        seconds["texture_phidp"] = time.perf_counter() - t0
        t0 = time.perf_counter()
        ref = ho.classify([host["dbz"], host["zdr"], host["kdp"], host["rhohv"], want_z, want_p, temperature], 1 << 6, R // SWEEPS,
                          host["mask"], spec, 0.0)
        seconds["classify"] = time.perf_counter() - t0
        seconds["chain"] = sum(seconds.values())
        result["numpy_seconds"] = {key: round(value, 3) for key, value in seconds.items()}
        result["differing_gates"] = {"sd_dbz": int((ho.bits(got["sd_dbz"]) != ho.bits(want_z)).sum()),
                                     "sd_phidp": int((ho.bits(got["sd_phidp"]) != ho.bits(want_p)).sum()),
                                     "classes": int((got["classes"] != ref.cls).sum()), "second": int((got["second"] != ref.second).sum()),
                                     "score": int((ho.bits(got["score"]) != ho.bits(ref.score)).sum())}
        result["class_shares"] = {"unclassified": round(float((ref.cls == 0).mean()), 4),
                                  **{cname: round(float((ref.cls == k + 1).mean()), 4) for k, cname in enumerate(table.class_names)}}
        result["ratio_numpy_over_device"] = {key: round(1000.0 * seconds[key] / result["calls"][key]["median_ms"], 1) for key in seconds}
    print(json.dumps({name: result}), flush=True)
    return result


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "hydro_timing.json"))
    ap.add_argument("--launches", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--repeat", type=int, default=50, help="back-to-back calls between the two events of one sample")
    ap.add_argument("--skip-oracle", action="store_true")
    args = ap.parse_args()
    import torch
    record = {"what": "tools/measure_hydro.py on one MI355X, one process: synthetic dual-polarisation volumes (three rain cells per ray, "
                      "clutter over the nearest 4 % of the gates, 5 % NaN per field, 3 % masked, 12 sweeps with a sounding that crosses "
                      "0 C at 4 km) at the bench volume's 4320 x 1000 and at C4's 10080 x 2000; SD(Z) over 5 gates, SD(PHIDP) over 9, "
                      f"the preset S-band table (980 cells, 47040 bytes of LDS).  median_ms: per call, from {args.repeat} back-to-back "
                      f"calls between two stream events, the four kinds of sample alternating, {args.launches} samples after "
                      f"{args.warmup} warm-up rounds (so a call finds its inputs where the same call left them: cache-warm at the "
                      "smaller size); the textures and the classifier through the raw C ABI into standing outputs, chain = "
                      "classify_hydrometeors_device with its five allocations.  bytes_moved: every input read once and every output "
                      "written once (a texture 9 bytes per gate with its mask, the classifier 31: six variables, the mask, cls, score "
                      "and second; the chain is their sum, 49; without the mask 8 + 8 + 30 = 46); share_of_hbm_peak: those bytes over "
                      "the time against 8 TB/s (at 4320 x 1000 the whole working set fits the 256 MiB Infinity Cache, so that share is "
                      "a rate, not an HBM measurement).  No counters were collected: where the classifier's time goes is not established "
                      "by this record.  numpy_seconds: "
                      "tests/hydro_oracle.py on the same arrays in the same process, once; differing_gates: gates at which an output "
                      "of the device differs from it in any bit.  No time is a pass criterion.",
              "device": torch.cuda.get_device_name(0), "volumes": {}}
    for name, (R, G) in VOLUMES.items():
        record["volumes"][name] = measure(name, R, G, args)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(record, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
