"""Times the median filter and the LLSD (include/radargrid_shear.h) on one GPU and writes profiles/shear_timing.json.

    python tools/measure_shear.py [--out profiles/shear_timing.json] [--launches 20] [--warmup 3] [--repeat 20]
                                  [--oracle-sweeps 12 12] [--skip-oracle]

Two synthetic volumes: 12 sweeps x 360 rays x 1000 gates (the bench volume's shape: 1 degree rays, 250 m gates) and 12 x 720 x
2000 (0.5 degree, 125 m): a wind that veers with height plus Rankine vortices and noise of sigma = 1 m/s, 2 % of the gates
missing at random and one sector without echo per sweep.  The window is ``llsd_window`` with its defaults (2500 m across the
beam, 750 m along it, at most 16 rays on either side).  For the median (3 x 3), the LLSD (azimuthal shear and divergence) and the
two back to back (``chain``) through the raw C ABI into standing buffers: the median of ``launches`` samples after ``warmup``
rounds, a sample being ``repeat`` back-to-back calls between two stream events, divided by ``repeat``, the kinds of sample
alternating.  ``share_of_bytes_bound``: the bytes a call has to move (4 in, 4 per output asked for, per gate) at the 8 TB/s HBM
peak, over the time.  ``llsd_by_max_half_rays``: the LLSD with the window's half-widths clipped to 2, 8 and 16 rays -- what the
azimuthal halo costs.  ``numpy_seconds``: the restatement (tests/shear_oracle.py) of the median and the LLSD on the first
``oracle_sweeps`` sweeps in the same process, once, and the gates at which an output of the device differs from it.  No time is
a pass criterion."""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

HBM_PEAK = 8.0e12
VOLUMES = {"bench_shape": (12, 360, 1000, 1.0, 250.0), "half_degree": (12, 720, 2000, 0.5, 125.0)}
MIN_VALID, MIN_FRACTION_Q16 = 6, 32768


def volume(S, R, G, ray_deg, gate_m, seed=17):
    rng = np.random.default_rng(seed)
    az = np.deg2rad(ray_deg) * np.arange(R)
    r = gate_m * (0.5 + np.arange(G))
    x, y = r[None, :] * np.sin(az)[:, None], r[None, :] * np.cos(az)[:, None]
    vel = np.empty((S, R, G), np.float32)
    for s in range(S):
        field = (12.0 + s) * np.cos(az - 0.5 - 0.1 * s)[:, None] * np.linspace(0.5, 1.0, G)[None, :]
        for k in range(6):                                       # Rankine vortices: solid rotation inside rc, 1 / d outside
            d0 = (0.15 + 0.12 * k) * r[-1]
            cx, cy, rc, vmax = d0 * np.sin(1.0 * k + 0.3 * s), d0 * np.cos(1.0 * k + 0.3 * s), 1500.0 + 300.0 * k, 20.0
            dx, dy = x - cx, y - cy
            d = np.hypot(dx, dy) + 1e-9
            speed = np.where(d < rc, vmax * d / rc, vmax * rc / d)
            # tangential wind projected on the beam
            field += speed * ((-dy / d) * np.sin(az)[:, None] + (dx / d) * np.cos(az)[:, None])
        vel[s] = (field + rng.normal(0.0, 1.0, (R, G))).astype(np.float32)
        a0 = (40 + 25 * s) % (R - 12)
        vel[s, a0:a0 + 12, 3 * G // 10 + 4 * s:] = np.nan        # a sector without echo
    vel[rng.random((S, R, G)) < 0.02] = np.nan
    return vel, r


def measure(name, shape, args):
    import torch
    import radar_processor_amd as rg
    from radar_processor_amd import _native
    lib = rg.load_library()
    dev = torch.device("cuda", 0)
    S, R, G, ray_deg, gate_m = shape
    host_vel, ranges = volume(*shape)
    window = rg.llsd_window(ranges, ray_deg, gate_m)
    vel = torch.from_numpy(host_vel).to(dev)
    P, n = _native.ptr, S * R * G
    filtered, shear, div = (torch.empty((S, R, G), dtype=torch.float32, device=dev) for _ in range(3))
    az_scale = torch.from_numpy(window.az_scale).to(dev)
    tables = {k: torch.from_numpy(np.minimum(window.half_rays, k)).to(dev) for k in (2, 8, 16)}
    stream = _native.stream_ptr

    def check(status):
        if status != 0:
            raise RuntimeError(lib.rg_last_error().decode())

    def median():
        check(lib.rg_polar_median_f32(P(vel), None, S, R, G, 1, 1, 1, 1, 1, P(filtered), stream()))

    def llsd(k=16, src=None):
        check(lib.rg_velocity_llsd_f32(P(filtered if src is None else src), None, S, R, G, P(tables[k]), P(az_scale), k, window.half_gates,
                                       window.range_scale, 1, MIN_VALID, MIN_FRACTION_Q16, 0, P(shear), P(div), None, None, stream()))

    def chain():
        median()
        llsd()

    calls = {"median": median, "llsd": llsd, "chain": chain, "llsd_max_half_rays_2": lambda: llsd(2), "llsd_max_half_rays_8": lambda: llsd(8),
             "llsd_max_half_rays_16": lambda: llsd(16)}
    bytes_per_gate = {"median": 8, "llsd": 12, "chain": 20, "llsd_max_half_rays_2": 12, "llsd_max_half_rays_8": 12, "llsd_max_half_rays_16": 12}
    for call in calls.values():
        call()
    torch.cuda.synchronize()
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
    ka = np.minimum(window.half_rays, 16)
    result = {"sweeps": S, "rays": R, "gates": G, "ray_spacing_deg": ray_deg, "gate_spacing_m": gate_m,
              "valid_gates": int(np.isfinite(host_vel).sum()), "half_gates": window.half_gates,
              "half_rays": {"min": int(ka.min()), "max": int(ka.max()), "mean": round(float(ka.mean()), 2),
                            "gates_at_16": int((ka == 16).sum()), "gates_at_most_2": int((ka <= 2).sum())},
              "min_valid": MIN_VALID, "min_fraction_q16": MIN_FRACTION_Q16, "calls": {}, "llsd_by_max_half_rays": {}}
    for key, ms in times.items():
        med = float(np.median(ms))
        moved = bytes_per_gate[key] * n
        entry = {"median_ms": round(med, 4), "min_ms": round(min(ms), 4), "max_ms": round(max(ms), 4), "bytes_moved": moved,
                 "share_of_bytes_bound": round(moved / HBM_PEAK / (med * 1e-3), 4)}
        if key.startswith("llsd_max_half_rays_"):
            k = int(key.rsplit("_", 1)[1])
            entry["mean_half_rays"] = round(float(np.minimum(window.half_rays, k).mean()), 2)
            result["llsd_by_max_half_rays"][str(k)] = entry
        else:
            result["calls"][key] = entry
    chain()
    torch.cuda.synchronize()
    result["gates_with_a_fit"] = int((~torch.isnan(shear)).sum().item())
    if args.skip_oracle:
        print(json.dumps({name: result}), flush=True)
        return result
    import shear_oracle as so
    sweeps = min(S, args.oracle_sweeps[0 if name == "bench_shape" else 1])
    got = {"median": filtered[:sweeps].cpu().numpy(), "az_shear": shear[:sweeps].cpu().numpy(), "divergence": div[:sweeps].cpu().numpy()}
    seconds = {"median": 0.0, "llsd": 0.0}
    differing = {key: 0 for key in got}
    for s in range(sweeps):                                      # sweeps never interact: one at a time keeps the planes small
        t0 = time.perf_counter()
        want_f = so.median(host_vel[s], None, 1, 1, 1, 1, 1)
        seconds["median"] += time.perf_counter() - t0
        t0 = time.perf_counter()
        want = so.llsd(want_f, None, window.half_rays, window.az_scale, 16, window.half_gates, window.range_scale, 1, MIN_VALID,
                       MIN_FRACTION_Q16, 0)
        seconds["llsd"] += time.perf_counter() - t0
        differing["median"] += int((so.bits(got["median"][s]) != so.bits(want_f[0])).sum())
        differing["az_shear"] += int((so.bits(got["az_shear"][s]) != so.bits(want.az_shear[0])).sum())
        differing["divergence"] += int((so.bits(got["divergence"][s]) != so.bits(want.divergence[0])).sum())
    result["oracle_sweeps"] = sweeps
    result["numpy_seconds"] = {key: round(value, 3) for key, value in seconds.items()}
    result["differing_gates"] = differing
    scale = sweeps / S
    result["ratio_numpy_over_device"] = {"median": round(1000.0 * seconds["median"] / (result["calls"]["median"]["median_ms"] * scale), 1),
                                         "llsd": round(1000.0 * seconds["llsd"] / (result["calls"]["llsd"]["median_ms"] * scale), 1)}
    print(json.dumps({name: result}), flush=True)
    return result


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "shear_timing.json"))
    ap.add_argument("--launches", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--repeat", type=int, default=20, help="back-to-back calls between the two events of one sample")
    ap.add_argument("--oracle-sweeps", type=int, nargs=2, default=[12, 12], help="sweeps the restatement is run on, per volume")
    ap.add_argument("--skip-oracle", action="store_true")
    args = ap.parse_args()
    import torch
    record = {"what": "tools/measure_shear.py on one MI355X, one process: synthetic volumes of 12 sweeps (a wind that veers with height, six "
                      "Rankine vortices, noise of sigma = 1 m/s, 2 % of the gates missing at random, one sector without echo per sweep); "
                      "the window is llsd_window's default (2500 m x 750 m, at most 16 rays on either side), rays wrapping, min_valid 6, "
                      "min_fraction 0.5.  calls.*.median_ms: per call through the raw C ABI into standing buffers, from "
                      f"{args.repeat} back-to-back calls between two stream events, the kinds of sample alternating, {args.launches} "
                      f"samples after {args.warmup} warm-up rounds (the working set of either volume fits the 256 MiB Infinity Cache, so a "
                      "call finds its inputs cache-warm); median is the 3 x 3 filter, llsd writes azimuthal shear and divergence, "
                      "chain is the two back to back.  share_of_bytes_bound: 4 bytes in and 4 per output per gate at the 8 TB/s HBM "
                      "peak, over the time.  llsd_by_max_half_rays: the LLSD with the half-widths clipped to 2, 8 and 16 rays "
                      "(mean_half_rays: what is left of them).  numpy_seconds: tests/shear_oracle.py on the first oracle_sweeps sweeps in "
                      "the same process, once; differing_gates: gates of those sweeps at which an output of the device differs from it; "
                      "ratio_numpy_over_device: scaled to the same number of sweeps.  No time is a pass criterion.",
              "device": torch.cuda.get_device_name(0), "volumes": {}}
    for name, shape in VOLUMES.items():
        record["volumes"][name] = measure(name, shape, args)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(record, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
