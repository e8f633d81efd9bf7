#!/usr/bin/env python3
"""Three C2-size radars (12x360x1000 gates each) on the 40x2000x2000 bench grid through the CSR-free mosaic
(rg_roi_grid_mosaic_f32), and each radar alone through rg_roi_grid_f32 on its reach window -- for a
``rocprofv3 --kernel-trace --stats`` run (profiles/README.md).  Prints one JSON line with the event-timed medians.

    rocprofv3 --kernel-trace --stats -d OUT -o mosaic -- python tools/profile_mosaic.py
"""
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

ORIGINS = [(0.0, -80e3, -90e3), (300.0, 10e3, 110e3), (600.0, 130e3, -30e3)]


def timed(fn, reps=5):
    import torch
    ts = []
    for r in range(reps + 1):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(); fn(); e1.record(); e1.synchronize()
        if r:
            ts.append(e0.elapsed_time(e1))
    return round(float(np.median(ts)), 3)


def main():
    import torch
    import radar_processor_amd as rg
    from radar_processor_amd import synthetic
    from radar_processor_amd.roi_grid import roi_grid_fields_device
    rg.load_library()
    dev = torch.device("cuda", 0)
    cfg = synthetic.CONFIGS["METRIC"]
    shape, limits = cfg["grid_shape"], cfg["grid_limits"]
    vols = [synthetic.make_volume(cfg["n_elev"], cfg["n_az"], cfg["n_gates"], seed=60 + r, fields=("DBZH",)) for r in range(3)]
    radars = [(v.gate_x, v.gate_y, v.gate_z, o) for v, o in zip(vols, ORIGINS)]
    ms = rg.MosaicSearch(radars, shape, limits, device=dev)
    fields = [[torch.from_numpy(np.ascontiguousarray(np.ma.getdata(v.fields["DBZH"]))).to(dev)] for v in vols]
    masks = [torch.from_numpy(np.ma.getmaskarray(v.fields["DBZH"]).astype(np.uint8)).to(dev) for v in vols]
    res = {"grid": list(shape), "origins": ORIGINS, "windows": [list(w) for w in ms.windows]}
    res["mosaic_ms"] = timed(lambda: rg.mosaic_fields_device(ms, fields, shared_masks=masks))
    alone = []
    for r, s in enumerate(ms.searches):
        out = torch.empty((1, *s.grid_shape), dtype=torch.float32, device=dev)
        alone.append(timed(lambda: roi_grid_fields_device(s, fields[r], [None], shared_mask=masks[r], out=out)))
    res["alone_ms"] = alone
    res["ratio_to_sum"] = round(res["mosaic_ms"] / sum(alone), 3)
    print(json.dumps(res), flush=True)


if __name__ == "__main__":
    main()
