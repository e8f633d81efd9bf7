#!/usr/bin/env python3
"""Is the nowcast better than showing the last scan again?  A sequence of COLMAX planes -> per scan the advection nowcasts for
1, 2, 3 and 6 scans ahead -> each verified against the scan it was made for, beside the persistence forecast: categorical scores
at 18 / 35 / 45 dBZ and the fractions skill score over window sizes 1 .. 64, all on the device.

The scans are made from one gridded plane by the advection kernel with a known drift of (4, -8) pixels per scan, and every scan
fades by 1 % -- something no advection can forecast, so the nowcast is good but not perfect.  Needs an MI355X and the built
library.

    python examples/nowcast_verification_example.py
"""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import torch  # noqa: E402

from radar_processor_amd import (NowcastVerifier, RoiSearch, advect_device, categorical_scores, collapse_plane_device,  # noqa: E402
                                 get_field_data, get_gate_coordinates, neighbourhood_fraction_device, roi_grid_fields_device,
                                 synthetic, verify_nowcast)

SCANS = 10
DRIFT = (4.0, -8.0)                                         # (dy, dx) pixels per scan
LEADS = (1, 2, 3, 6)
THRESHOLDS = (18.0, 35.0, 45.0)
SCALES = (1, 2, 4, 8, 16, 32, 64)


class Grid:
    grid_shape, grid_limits = (12, 400, 400), ((500.0, 12000.0), (-240e3, 240e3), (-240e3, 240e3))


def main():
    volume = synthetic.make_volume(n_elev=6, n_az=360, n_gates=480, seed=3, fields=("DBZH",))
    radar = volume.as_radar()
    search = RoiSearch(*get_gate_coordinates(radar), Grid.grid_shape, Grid.grid_limits)
    dbz = get_field_data(radar, "DBZH")
    field = torch.from_numpy(np.ascontiguousarray(dbz.filled(np.nan), dtype=np.float32).ravel()).to(search.dev)
    mask = torch.from_numpy(np.ma.getmaskarray(dbz).ravel().astype(np.uint8)).to(search.dev)
    first = collapse_plane_device(roi_grid_fields_device(search, [field], [mask])[0], "colmax").contiguous()

    # 1. the scans: the first plane drifting by DRIFT per scan and fading by 1 % per scan; nothing moves in from outside (0 dBZ)
    drift = torch.tensor([[DRIFT]], dtype=torch.float32, device=first.device)
    scans = advect_device(first, drift, [float(t) for t in range(SCANS)], lattice=(0.0, 0.0, 1.0, 1.0, 1, 1), method="nearest")
    fade = torch.tensor([0.99 ** t for t in range(SCANS)], dtype=torch.float32, device=first.device)[:, None, None]
    scans = (torch.nan_to_num(scans, nan=0.0) * fade).contiguous()

    # 2. the verifier: one update per scan.  It verifies what was forecast FOR this scan, then forecasts FROM it
    check = NowcastVerifier(LEADS, THRESHOLDS, SCALES, motion="auto", block=32, stride=16, search=16)
    frames = []
    for t in range(SCANS):
        frame = check.update(scans[t])
        frames.append(frame)
        print(f"scan {t}: verified the forecasts made {list(frame.verified)} scans ago"
              + ("" if frame.forecasts is None else f", filed {len(LEADS)} nowcasts"))

    # 3. the scores, per lead: the only host read-back
    scores = check.scores()
    for kind in ("nowcast", "persistence"):
        s = scores[kind]
        for li, lead in enumerate(LEADS):
            fss35 = " ".join(f"{v:.3f}" for v in s["fss"][li, 1])
            print(f"{kind:11s} +{lead} scans ({s['verified'][li]} verified): CSI at 35 dBZ {s['csi'][li, 1]:.3f}, ETS {s['ets'][li, 1]:.3f}, "
                  f"bias {s['bias'][li, 1]:.3f}; FSS at sizes {list(SCALES)}: {fss35} (useful from {s['useful'][li, 1]:.3f})")
    gain = scores["nowcast"]["fss"][:, 1, 0] - scores["persistence"]["fss"][:, 1, 0]
    print("FSS gained over persistence at 35 dBZ, single pixels: " + ", ".join(f"+{lead}: {g:+.3f}" for lead, g in zip(LEADS, gain)))

    # 4. the pieces by hand: the nowcast scan 1 filed for one scan ahead, against scan 2
    older = frames[1].forecasts
    both = verify_nowcast(older[:1], scans[2:3], THRESHOLDS, SCALES)
    print(f"one pair by hand: POD at 18 dBZ {categorical_scores(both.contingency)['pod'][0, 0]:.3f}, FSS at 64 px {both.fss.fss()[0, 0, -1]:.3f}")

    # 5. the product that falls out: how much of the 15 x 15 pixels around every pixel the nowcast puts at or above 35 dBZ
    prob = neighbourhood_fraction_device(older[0], (35.0,), scale=15)
    print(f"neighbourhood fraction of >= 35 dBZ within 15 px: {float((prob > 0).float().mean()):.1%} of the plane is above 0, "
          f"{float((prob >= 0.5).float().mean()):.1%} at or above one half")


if __name__ == "__main__":
    main()
