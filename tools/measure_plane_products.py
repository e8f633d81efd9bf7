#!/usr/bin/env python3
"""Products-only passes, one configuration, same process, same arrays, interleaved rounds:

    python tools/measure_plane_products.py [--config METRIC|C2] [--fields 1,3,4] [--rounds 7] [--out profiles/...json]

Per field count, three ways to get the 2-D products of one pass through ``grid_products_device``:

  (a) ``columns``  fused COLMAX + argmax + CAPPI 4000 m -- rg_csr_compact_apply_columns_f32 (what existed before the planes mode);
  (b) ``planes``   fused COLMAX + argmax + COLMIN + COLMEAN + CAPPI 4000 m + PPI 0.5 / 1.5 deg -- rg_csr_compact_apply_planes_f32
                   (+ the PPI finish kernels);
  (c) ``separate`` the same products as (b) from the stored 3-D grids: rg_csr_compact_apply_packed_f32, then the separate
                   column / CAPPI / PPI kernels.

Each round times every variant once (stream events around the whole call, host work included), in an order that rotates per
round; the median over rounds is reported.  Also checks that (b) and (c) return the same bits.  One JSON object on stdout and
in ``--out``."""
import argparse
import json
import os
import sys
import tempfile

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def _same_bits(a, b):
    import torch
    view = torch.int64 if a.element_size() == 8 else torch.int32
    return a.dtype == b.dtype and torch.equal(a.contiguous().view(view), b.contiguous().view(view))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--config", default="METRIC")
    ap.add_argument("--fields", default="1,3,4")
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--out", default="")
    args = ap.parse_args()
    import torch
    import radar_processor_amd as rg
    from radar_processor_amd import synthetic
    rg.load_library()
    dev = torch.device("cuda", 0)
    cfg = synthetic.CONFIGS[args.config]
    names = ("DBZH", "ZDR", "RHOHV")
    vol = synthetic.make_volume(cfg["n_elev"], cfg["n_az"], cfg["n_gates"], seed=0, fields=names)
    with tempfile.TemporaryDirectory() as tmp:
        geom = rg.compute_grid_geometry(vol.gate_x, vol.gate_y, vol.gate_z, cfg["grid_shape"], cfg["grid_limits"], tmp)
    compact = geom.device_compact(dev)
    assert compact is not None and compact.ensure_packed(geom.device_csr(dev)), "needs the packed records"
    base_f = [torch.from_numpy(np.ascontiguousarray(np.ma.getdata(vol.fields[n]))).to(dev) for n in names]
    base_m = [torch.from_numpy(np.ma.getmaskarray(vol.fields[n]).astype(np.uint8)).to(dev) for n in names]
    specs = {
        "columns": (dict(cappi=(4000.0,)), True),
        "planes": (dict(cappi=(4000.0,), colmin=True, colmean=True, ppi=(0.5, 1.5)), True),
        "separate": (dict(cappi=(4000.0,), colmin=True, colmean=True, ppi=(0.5, 1.5)), False),
    }
    rec = {"config": args.config, "grid_shape": list(cfg["grid_shape"]), "pairs": geom.n_pairs(), "rounds": args.rounds,
           "unit": "ms per products-only pass (events around grid_products_device)", "runs": []}

    def run(fl, ml, key):
        kw, fused = specs[key]
        return rg.grid_products_device(geom, fl, ml, products=rg.PlaneProducts(**kw), fused=fused)

    for nf in [int(x) for x in args.fields.split(",")]:
        fl = [base_f[i % 3] for i in range(nf)]
        ml = [base_m[i % 3] for i in range(nf)]
        got = {k: run(fl, ml, k) for k in specs}                       # warm-up, plans cached, and the bits compared
        same = all(_same_bits(a[key], b[key]) for a, b in zip(got["planes"], got["separate"])
                   for key in ("colmax", "argmax", "colmin", "colmean"))
        same = same and all(_same_bits(a["ppi"][e], b["ppi"][e]) for a, b in zip(got["planes"], got["separate"]) for e in (0.5, 1.5))
        same = same and all(_same_bits(a["cappi"][4000.0], b["cappi"][4000.0]) for a, b in zip(got["planes"], got["separate"]))
        del got
        times = {k: [] for k in specs}
        keys = list(specs)
        for r in range(args.rounds):
            for key in keys[r % 3:] + keys[:r % 3]:
                torch.cuda.synchronize()
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                out = run(fl, ml, key)
                e1.record()
                e1.synchronize()
                times[key].append(e0.elapsed_time(e1))
                del out
        med = {k: round(float(np.median(v)), 3) for k, v in times.items()}
        rec["runs"].append({"fields": nf, "median_ms": med, "all_ms": {k: [round(t, 3) for t in v] for k, v in times.items()},
                            "planes_vs_columns": round(med["planes"] / med["columns"], 3),
                            "planes_vs_separate": round(med["planes"] / med["separate"], 3),
                            "planes_equal_separate_bits": bool(same)})
        print(json.dumps(rec["runs"][-1]), file=sys.stderr)
    line = json.dumps(rec)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as fh:
            fh.write(json.dumps(rec, indent=1) + "\n")


if __name__ == "__main__":
    main()
