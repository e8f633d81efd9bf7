"""Times the polar-domain phase processing (include/radargrid_phase.h) on one GPU and writes profiles/phase_timing.json.

    python tools/measure_phase.py [--out profiles/phase_timing.json] [--launches 20] [--warmup 3] [--repeat 50] [--skip-oracle]

Two volumes of synthetic dual-polarisation rays (KDP cells along every ray, a system offset, sigma = 3 degree noise, 5 % NaN,
3 % masked): the bench volume's 4320 rays x 1000 gates and C4's 10080 x 2000.  For each of the three calls through the raw
C ABI and for the chain (``process_phase_device``, allocations included): the median of ``launches`` samples after ``warmup``
rounds, a sample being ``repeat`` back-to-back calls between two stream events, divided by ``repeat`` (a single call lasts tens of
microseconds: less than an event pair resolves well), the four kinds of sample alternating; the bytes the call has to move
(every input read once, every output written once); those bytes over the time, as a share of the 8 TB/s HBM peak.  ``numpy_seconds``: the NumPy restatement (tests/phase_oracle.py)
of the same work in the same process, once, and whether every output of the device equals it bit for bit.  No time is a pass
criterion."""
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
SPACING, WRAP, HALF, MIN_VALID, MAX_DPHI = 240.0, 360.0, 15, 8, 360.0
VOLUMES = {"bench_4320x1000": (4320, 1000), "c4_10080x2000": (10080, 2000)}
BYTES_PER_GATE = {"unfold": 4 + 1 + 4, "fit": 4 + 4 + 4 + 2, "attenuation": 3 * 4 + 4 * 4}
BYTES_PER_GATE["chain"] = sum(BYTES_PER_GATE.values())


def volume(R, G, seed):
    """Rays with three KDP cells each at ray-dependent ranges; PHIDP wrapped into [-180, 180)."""
    rng = np.random.default_rng(seed)
    kdp = np.zeros((R, G), np.float32)
    x = np.arange(G)[None, :]
    for k, width in ((1.0, G // 12), (2.5, G // 25), (4.0, G // 40)):
        start = rng.integers(G // 10, G - G // 5, size=(R, 1))
        kdp[(x >= start) & (x < start + width)] = k
    truth = 100.0 + np.cumsum(2.0 * kdp.astype(np.float64) * SPACING / 1000.0, axis=1) + rng.normal(0.0, 3.0, (R, G))
    phidp = (truth - 360.0 * np.floor((truth + 180.0) / 360.0)).astype(np.float32)
    phidp[rng.random((R, G)) < 0.05] = np.nan
    mask = (rng.random((R, G)) < 0.03).astype(np.uint8)
    dbz = (20.0 + 7.0 * kdp + rng.normal(0.0, 1.0, (R, G))).astype(np.float32)
    zdr = (0.4 + 0.5 * kdp + rng.normal(0.0, 0.1, (R, G))).astype(np.float32)
    return phidp, mask, dbz, zdr


def measure(name, R, G, args):
    import torch
    import radar_processor_amd as rg
    from radar_processor_amd import _native
    import phase_oracle as po
    lib = rg.load_library()
    dev = torch.device("cuda", 0)
    alpha, beta = rg.ATTENUATION_COEFFICIENTS["C"]
    host = volume(R, G, seed=R + G)
    phidp, mask, dbz, zdr = (torch.from_numpy(a).to(dev) for a in host)
    new = lambda dtype: torch.empty((R, G), dtype=dtype, device=dev)                      # noqa: E731
    unfolded, kdp, phi_s, count = new(torch.float32), new(torch.float32), new(torch.float32), new(torch.uint16)
    dbz_out, zdr_out, pia, dphi = (new(torch.float32) for _ in range(4))
    P, scale = _native.ptr, 500.0 / (65536.0 * SPACING)
    half = (ctypes.c_int32 * 1)(HALF)

    def check(status):
        if status != 0:
            raise RuntimeError(lib.rg_last_error().decode())

    calls = {
        "unfold": lambda: check(lib.rg_phidp_unfold_f32(P(phidp), P(mask), R, G, WRAP, P(unfolded), None, _native.stream_ptr())),
        "fit": lambda: check(lib.rg_phidp_fit_f32(P(unfolded), R, G, None, None, half, 1, MIN_VALID, 0, scale, P(kdp), P(phi_s), P(count),
                                                  _native.stream_ptr())),
        "attenuation": lambda: check(lib.rg_attenuation_phidp_f32(P(phi_s), None, R, G, alpha, beta, MAX_DPHI, P(dbz), P(zdr), P(dbz_out),
                                                                  P(zdr_out), P(pia), P(dphi), _native.stream_ptr())),
        "chain": lambda: rg.process_phase_device(phidp, dbz, SPACING, zdr=zdr, mask=mask, band="C", half_window=HALF,
                                                 min_valid=MIN_VALID, max_dphi=MAX_DPHI),
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
    result = {"rays": R, "gates": G, "calls": {}}
    for key, ms in times.items():
        median = float(np.median(ms))
        moved = BYTES_PER_GATE[key] * R * G
        result["calls"][key] = {"median_ms": round(median, 4), "min_ms": round(min(ms), 4), "max_ms": round(max(ms), 4),
                                "bytes_moved": moved, "tb_per_s": round(moved / (median * 1e-3) / 1e12, 3),
                                "share_of_hbm_peak": round(moved / (median * 1e-3) / HBM_PEAK, 3)}
    if not args.skip_oracle:
        got = rg.process_phase_device(phidp, dbz, SPACING, zdr=zdr, mask=mask, band="C", half_window=HALF, min_valid=MIN_VALID,
                                      max_dphi=MAX_DPHI)
        got = {field: getattr(got, field).cpu().numpy() for field in got._fields}
        seconds = {}
        t0 = time.perf_counter()
        want_unfolded, _ = po.unfold(host[0], host[1], WRAP)
        seconds["unfold"] = time.perf_counter() - t0
        t0 = time.perf_counter()
        fit = po.fit(want_unfolded, scale, half_window=(HALF,), min_valid=MIN_VALID)
        seconds["fit"] = time.perf_counter() - t0
        t0 = time.perf_counter()
        att = po.attenuation(fit.phi_s, host[2], alpha=alpha, beta=beta, max_dphi=MAX_DPHI, zdr=host[3])
        seconds["attenuation"] = time.perf_counter() - t0
        seconds["chain"] = sum(seconds.values())
        want = dict(phidp_unfolded=want_unfolded, phidp=fit.phi_s, kdp=fit.kdp, count=fit.count, dbz=att.dbz, zdr=att.zdr, pia=att.pia,
                    dphi=att.dphi)
        result["numpy_seconds"] = {key: round(value, 3) for key, value in seconds.items()}
        result["differing_gates"] = {field: int((po.bits(got[field]) != po.bits(want[field])).sum()) for field in want}
        result["ratio_numpy_over_device"] = {key: round(1000.0 * seconds[key] / result["calls"][key]["median_ms"], 1) for key in seconds}
    print(json.dumps({name: result}), flush=True)
    return result


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "phase_timing.json"))
    ap.add_argument("--launches", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--repeat", type=int, default=50, help="back-to-back calls between the two events of one sample")
    ap.add_argument("--skip-oracle", action="store_true")
    args = ap.parse_args()
    import torch
    record = {"what": "tools/measure_phase.py on one MI355X, one process: synthetic dual-polarisation volumes (three KDP cells per ray, "
                      "offset 100 degrees, sigma = 3 degree noise, 5 % NaN, 3 % masked) at the bench volume's 4320 x 1000 and at C4's "
                      f"10080 x 2000; half-window 15, min_valid 8, C band.  median_ms: per call, from {args.repeat} back-to-back calls between "
                      f"two stream events, the four kinds of sample alternating, {args.launches} samples after {args.warmup} warm-up "
                      "rounds (so a call finds its inputs where the same call left them: cache-warm at the smaller size); unfold / "
                      "fit / attenuation through the raw C ABI into standing outputs, chain = process_phase_device with its eight allocations.  bytes_moved: every "
                      "input read once and every output written once (unfold 9, fit 14, attenuation 28 bytes per gate; the chain is "
                      "their sum); share_of_hbm_peak: those bytes over the time against 8 TB/s (at 4320 x 1000 the whole working set "
                      "fits the 256 MiB Infinity Cache, so that share is a rate, not an HBM measurement).  numpy_seconds: "
                      "tests/phase_oracle.py on the same arrays in the same process, once; differing_gates: gates at which an output "
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
