#!/usr/bin/env python3
"""With what probability does it reach 35 dBZ here in half an hour?  Two COLMAX planes one scan apart -> the motion between them
-> 20 extrapolations whose motion errs by an amount that grows with the lead -> the fraction of them at or above 18 / 35 / 45 dBZ
per pixel, 1 .. 6 scans ahead, in one kernel -> verified against the scans that then arrive: Brier score and its decomposition,
Brier skill, reliability curve and ROC area, all from an integer table built on the device.

The scans are made from one gridded plane by the advection kernel with a drift of (4, -8) pixels per scan that slowly VEERS --
something the motion estimated from the first two scans cannot know, which is what the perturbations are for -- and fade by 1 %
per scan.  Needs an MI355X and the built library.

    python examples/probabilistic_nowcast_example.py
"""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import torch  # noqa: E402

from radar_processor_amd import (RoiSearch, advect_device, collapse_plane_device, ensemble_histogram_device,  # noqa: E402
                                 get_field_data, get_gate_coordinates, probabilistic_nowcast_device, probability_scores,
                                 roi_grid_fields_device, synthetic)

LEADS = (1, 2, 3, 4, 5, 6)                                  # scans ahead
THRESHOLDS = (18.0, 35.0, 45.0)
MEMBERS = 20
DRIFT = (4.0, -8.0)                                         # (dy, dx) pixels per scan at the start
VEER = (0.35, 0.25)                                         # added to the drift with every further scan
# The speed error a * t**b + c, in pixels per scan with t in scans.  Published fits are in km/h for a lead in minutes,
# s_kmh(t_min) = A * t_min**B + C; with scans every DT minutes on pixels of PX km one scan at 1 km/h is DT / 60 / PX pixels:
DT, PX = 5.0, 1.2
UNIT = DT / 60.0 / PX


def from_kmh(A, B, C):
    return (A * DT ** B * UNIT, B, C * UNIT)


PAR, PERP = from_kmh(2.3, 0.33, 1.0), from_kmh(1.6, 0.36, 0.5)


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

    # 1. the scans: scan t is the first plane moved by the drift summed up to t, fading by 1 % per scan
    scans = []
    for t in range(2 + max(LEADS)):
        moved = [DRIFT[k] * t + VEER[k] * t * (t - 1) / 2.0 for k in (0, 1)]
        drift = torch.tensor([[moved]], dtype=torch.float32, device=first.device)
        plane = advect_device(first, drift, [1.0], lattice=(0.0, 0.0, 1.0, 1.0, 1, 1), method="bilinear")[0]
        scans.append(torch.nan_to_num(plane, nan=0.0) * 0.99 ** t)
    prev, now = scans[0], scans[1]
    observed = torch.stack([scans[1 + lead] for lead in LEADS]).contiguous()

    # 2. the forecast: motion, fill, perturbations along the mean motion, and the ensemble in one kernel
    products, grid = probabilistic_nowcast_device(prev, now, LEADS, THRESHOLDS, MEMBERS, par=PAR, perp=PERP, seed=0,
                                                  block=32, stride=16, search=16, method="bilinear", min_members=MEMBERS // 2,
                                                  want=("prob", "counts", "members", "mean"))
    mean_motion = grid.motion.double().mean(dim=(0, 1)).cpu().numpy()
    print(f"mean motion ({mean_motion[0]:+.2f}, {mean_motion[1]:+.2f}) px per scan; speed error at +6 scans: "
          f"{PAR[0] * 6 ** PAR[1] + PAR[2]:.2f} px per scan along it, {PERP[0] * 6 ** PERP[1] + PERP[2]:.2f} across")
    for li, lead in enumerate(LEADS):
        p = products.prob[li, 1]
        sure, maybe = float((p == 1).float().mean()), float(((p > 0) & (p < 1)).float().mean())
        print(f"+{lead} scans: P(>= 35 dBZ) is 1 on {sure:.2%} of the plane and strictly between 0 and 1 on {maybe:.2%}; "
              f"{float((products.members[li] == MEMBERS).float().mean()):.1%} of the pixels have all {MEMBERS} members")

    # 3. the verification: how often k of the 20 members exceeded, and how often the scan that arrived then did
    table = ensemble_histogram_device(products, observed)
    scores = probability_scores(table)                       # the only host read-back
    for li, lead in enumerate(LEADS):
        print(f"+{lead} scans at 35 dBZ: Brier {scores['brier'][li, 1]:.4f} = reliability {scores['reliability'][li, 1]:.4f} "
              f"- resolution {scores['resolution'][li, 1]:.4f} + uncertainty {scores['uncertainty'][li, 1]:.4f}; "
              f"skill {scores['bss'][li, 1]:+.3f}, ROC area {scores['roc_area'][li, 1]:.3f}")
    curve, used = scores["reliability_curve"][-1, 1], scores["sharpness"][-1, 1]
    print("reliability at +6 scans, 35 dBZ (forecast: observed frequency, pixels): "
          + ", ".join(f"{p:.2f}: {f:.2f} ({n})" for p, f, n in zip(scores["forecast_probability"][::4], curve[::4], used[::4])))

    # 4. beside it, the deterministic nowcast as a 0 / 1 forecast: the control member alone
    #    (member 0 of the ensemble), on the same pixels -- those where the ensemble is complete
    nowcast = advect_device(now, grid, LEADS, method="bilinear")
    control = (nowcast[:, None] >= torch.tensor(THRESHOLDS, device=now.device)[None, :, None, None]).to(torch.uint8)
    alone = products._replace(counts=control.contiguous(), members=(~torch.isnan(nowcast)).to(torch.uint8), n_members=1)
    brier_alone = probability_scores(ensemble_histogram_device(alone, observed, mask=products.members != MEMBERS))["brier"]
    print("Brier score at 35 dBZ, ensemble against the single nowcast: "
          + ", ".join(f"+{lead}: {scores['brier'][li, 1]:.4f} / {brier_alone[li, 1]:.4f}" for li, lead in enumerate(LEADS)))


if __name__ == "__main__":
    main()
