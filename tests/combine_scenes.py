"""The mosaic combine rules (``combine="max"`` / ``"nearest_radar"``: rg_roi_grid_mosaic_combine_f32,
rg_roi_section_mosaic_combine_f32) restated in NumPy, and the scenes of their tests -- tests/test_mosaic_combine_host.py,
tests/test_gpu_mosaic_combine.py, tests/test_gpu_mosaic_section_combine.py (a helper module: pytest does not collect it).

The rules (include/radargrid_hip.h, restated once here, in :func:`fold`).  For a field and a voxel (or section sample),
radar k of the call's table HAS A VALUE when its own live weight sum is > 0; its value m_k is what the mean entry point
stores for a table holding only entry k.

  max            walk the table in order; radar k takes over when nothing is held yet, or m_k > held, or the held value is
                 NaN and m_k is not.  Equal values, and -0.0 against +0.0, stay with the earlier table position.
  nearest_radar  among the radars that have a value, the smallest D_k = x*x + y*y + z*z, float64, unfused, from the float32
                 coordinates of the voxel in radar k's frame; equal D goes to the earlier table position.

The winner's bits are copied.  No radar has a value: the fill, and 255 in the radar map.

``tie_scene`` is a 3 x 9 x 21 grid (ragged against the lattice kernel's 16 x 4 patch and the section kernel's four-point
block) with five radars:

  slot 0     ``poison``: one unmasked NaN and one unmasked +Inf among the DBZH values of gates that are neighbours of voxels
  slots 1, 2 ``twin``: the same gates, the same fields, the same origin -- value ties and distance ties on every voxel
             they reach
  slots 3, 4 ``mirror``: antennas at x = +9 km and x = -9 km, same y and z, different gates and fields.  The grid's columns
             are whole multiples of 3 km about x = 0, so a column's float32 coordinate in one radar's frame is exactly the
             negative of the mirrored column's in the other's: on the x = 0 column the two D are equal, the values differ.
"""
import dataclasses
import functools

import numpy as np

import mosaic_scenes as ms
import mosaic_section_scenes as mss
import radar_processor_amd as rg
from oracle import radar_grid_oracle as oracle

COMBINES = ("max", "nearest_radar")
NO_RADAR = 255
FILL = -9999.0                                    # no mean of these scenes equals it: a per-radar grid's fill marks "no value"

TIE_SHAPE = (3, 9, 21)                            # 9 = 2 * 4 + 1 rows, 21 = 16 + 5 columns
TIE_LIMITS = ((0.0, 5000.0), (-12e3, 12e3), (-30e3, 30e3))          # 2.5 km levels, 3 km rows and columns; column 10 is x = 0
TIE_POISON, TIE_TWINS, TIE_MIRROR = 0, (1, 2), (3, 4)
MIRROR_COLUMN = 10


# ---- the rules ------------------------------------------------------------------------------------------------------------------
def fold(values, has, combine, d=None, fill=FILL):
    """The combine rules as a fold over a stack of per-radar grids, in table order.

    ``values`` float32 ``[R, ...]``: radar k's own mean; ``has`` bool ``[R, ...]``: whether radar k has a value there;
    ``d`` float64 ``[R, ...]`` (``nearest_radar``): D_k.  Returns ``(out float32 [...], who uint8 [...])``: the winner's
    bits (``fill`` where nobody has a value) and its table position (255 there)."""
    values = np.asarray(values, dtype=np.float32)
    has = np.asarray(has, dtype=bool)
    held = np.zeros(values.shape[1:], dtype=np.float32)
    held_d = np.zeros(values.shape[1:], dtype=np.float64)
    who = np.full(values.shape[1:], NO_RADAR, dtype=np.uint8)
    for k in range(values.shape[0]):
        nothing = who == NO_RADAR
        if combine == "max":
            with np.errstate(invalid="ignore"):
                take = has[k] & (nothing | (values[k] > held) | (np.isnan(held) & ~np.isnan(values[k])))
        elif combine == "nearest_radar":
            take = has[k] & (nothing | (np.asarray(d[k], dtype=np.float64) < held_d))
            held_d = np.where(take, d[k], held_d)
        else:
            raise ValueError(combine)
        held = np.where(take, values[k], held)           # a copy: the bits arrive unchanged
        who = np.where(take, np.uint8(k), who)
    return np.where(who == NO_RADAR, np.float32(fill), held), who


def antenna_d2(x, y, z):
    """D of the float32 coordinates (broadcast): float64, unfused, (x*x + y*y) + z*z."""
    x, y, z = (np.asarray(c, dtype=np.float32).astype(np.float64) for c in (x, y, z))
    return x * x + y * y + z * z


def lattice_d(scene, r) -> np.ndarray:
    """D of every voxel of the scene's grid in radar r's frame: its own float32 tables of the shifted limits."""
    lim = rg.mosaic_limits(scene.limits, scene.origins[r])
    zc, yc, xc = (np.linspace(lim[a][0], lim[a][1], scene.shape[a], dtype="float32") for a in range(3))
    return antenna_d2(xc[None, None, :], yc[None, :, None], zc[:, None, None])


def section_d(scene, r, xs, ys) -> np.ndarray:
    """D of the samples (level k, point i) of a section in radar r's frame, ``[nz, n_points]``."""
    x_r, y_r = mss.radar_points(scene, r, xs, ys)
    return antenna_d2(x_r[None, :], y_r[None, :], mss.levels(scene, r)[:, None])


# ---- the tie scene --------------------------------------------------------------------------------------------------------------
def _tie_specs():
    twin = ms.RadarSpec(seed=401, max_range_m=24e3, origin=(0.0, -6000.0, 3000.0))
    return [ms.RadarSpec(seed=400, max_range_m=26e3, origin=(150.0, 3000.0, -6000.0)),
            twin, twin,
            ms.RadarSpec(seed=403, max_range_m=22e3, origin=(200.0, 6000.0, 9000.0)),
            ms.RadarSpec(seed=404, max_range_m=22e3, origin=(200.0, 6000.0, -9000.0))]


@functools.lru_cache(maxsize=None)
def tie_scene() -> ms.Scene:
    specs = _tie_specs()
    scene = ms.Scene("tie", specs, [ms.volume(s) for s in specs], [s.origin for s in specs], shape=TIE_SHAPE,
                     limits=TIE_LIMITS)
    # the poison: two gates of slot 0 that are neighbours of voxels and pass the QC mask get a NaN and a +Inf, unmasked
    vol = scene.vols[TIE_POISON]
    qc = oracle.gate_mask("below", np.ma.getdata(vol.fields["RHOHV"]), 0.8)
    ip, idx, _ = scene.csr(TIE_POISON)
    rows = np.repeat(np.arange(len(ip) - 1), np.diff(ip))
    others = np.sum([np.diff(scene.csr(r)[0]) > 0 for r in range(1, len(specs))], axis=0) > 0     # voxels other radars reach
    ok = ~qc[idx] & ~np.ma.getmaskarray(vol.fields["RHOHV"])[idx]
    shared_rows = np.bincount(idx[ok & others[rows]], minlength=len(qc))      # per gate: its voxels that others reach too
    g_nan = int(np.argmax(shared_rows))
    shared_rows[np.isin(np.arange(len(qc)), idx[np.isin(rows, rows[idx == g_nan])])] = 0      # no voxel in common
    g_inf = int(np.argmax(shared_rows))
    assert shared_rows[g_inf] > 0
    data = np.ma.getdata(vol.fields["DBZH"]).copy()
    mask = np.ma.getmaskarray(vol.fields["DBZH"]).copy()
    data[g_nan], data[g_inf] = np.nan, np.inf
    mask[g_nan] = mask[g_inf] = False
    fields = dict(vol.fields)
    fields["DBZH"] = np.ma.array(data, mask=mask)
    scene.vols[TIE_POISON] = dataclasses.replace(vol, fields=fields)
    return scene


def scene(name):
    return {"scene16": ms.scene16, "tie": tie_scene}[name]()


# ---- fields ---------------------------------------------------------------------------------------------------------------------
def field_set(scene, nf, masked=True):
    """Per radar ``nf`` (values float32, mask bool) pairs and one shared QC mask (RHOHV below 0.8).  Field k is
    FIELDS[k % 3] of the radar plus k; ``masked``: its mask is the field's own (from field 3 on with 5 % more gates, seeded
    per radar and field).  ``masked=False``: no gate is masked, the shared mask is all clear and NaN values become -32 --
    except unmasked NaN / Inf values (the tie scene's poison), which stay."""
    out, shared = [], []
    for r, v in enumerate(scene.vols):
        n = len(v.gate_x)
        qc = oracle.gate_mask("below", np.ma.getdata(v.fields["RHOHV"]), 0.8) if n else np.zeros(0, dtype=bool)
        fs = []
        for k in range(nf):
            f = v.fields[ms.FIELDS[k % 3]]
            own = np.ma.getmaskarray(f).copy()
            data = (np.ma.getdata(f) + np.float32(k)).astype(np.float32)
            if masked:
                mask = own
                if k >= 3:
                    mask = mask | (np.random.default_rng(1000 * r + k).random(n) < 0.05)
            else:
                data = np.where(np.isnan(data) & own, np.float32(-32.0), data)
                mask = np.zeros(n, dtype=bool)
            fs.append((data, mask))
        out.append(fs)
        shared.append(qc if masked else np.zeros(n, dtype=bool))
    return out, shared


def radar_stats(scene, weighting, fs, shared, k, r, pairs=None):
    """oracle.voxel_stats of field k for radar r ALONE (float64 weights): its mean ``m``, its live count ``n``.  ``pairs``:
    ``(indptr, gate_indices, float64 weights)`` of a section; default: the radar's lattice CSR."""
    ip, idx, w = (scene.csr(r)[0], scene.csr(r)[1], scene.weights_f64(r, weighting)) if pairs is None else pairs
    return oracle.voxel_stats(ip, idx, w, fs[r][k][0], fs[r][k][1] | shared[r])


def section_pairs(scene, weighting, r, xs, ys, key):
    ip, idx, d2, r2 = mss.radar_pairs(scene, r, xs, ys, key)
    return ip, idx, oracle.roi_weight_f64(d2, r2, weighting)


# ---- paths ----------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def path(name):
    """``(xs, ys)`` float32 of the section through the scene: 4k + 3 points (the section kernel's last block is ragged).
    scene16: mosaic_section_scenes' dog-leg at another spacing.  tie: eight points exactly on the mirror column x = 0, then
    a diagonal across the grid."""
    if name == "scene16":
        xs, ys, _ = rg.section_path(mss.VERTICES, 1385.0)
    else:
        xs = np.concatenate([np.zeros(8), np.linspace(-28e3, 28e3, 15)]).astype(np.float32)
        ys = np.concatenate([np.linspace(-11e3, 11.5e3, 8), np.linspace(-10e3, 9e3, 15)]).astype(np.float32)
    assert len(xs) % 4 == 3, len(xs)
    return xs, ys


# ---- what the scenes must exercise (asserted by tests/test_mosaic_combine_host.py) --------------------------------------------
def count_cases(m, n, d) -> dict:
    """From per-radar float64 means ``m [R, V]``, live counts ``n [R, V]`` and ``d [R, V]``: how many samples have no radar,
    one, several; where max and nearest_radar pick different radars; where the largest value / the smallest D among the
    radars with a value is shared by two of them (ties), and where the tie is between different values / distances."""
    has = n > 0
    reach = has.sum(axis=0)
    vmax, wmax = fold(m.astype(np.float32), has, "max")
    _, wnear = fold(m.astype(np.float32), has, "nearest_radar", d)
    mm = np.where(has, m, -np.inf)
    dd = np.where(has, d, np.inf)
    with np.errstate(invalid="ignore"):
        best_v = np.nanmax(np.where(np.isnan(mm), -np.inf, mm), axis=0)
        value_tie = (has & (mm == best_v)).sum(axis=0) >= 2
    best_d = dd.min(axis=0)
    d_tie = (has & (dd == best_d)).sum(axis=0) >= 2
    at_min = has & (dd == best_d)
    vals = np.where(at_min, m, np.nan)
    import warnings
    with np.errstate(invalid="ignore"), warnings.catch_warnings():
        warnings.simplefilter("ignore", RuntimeWarning)                  # all-NaN columns: nobody has a value
        d_tie_other_values = d_tie & (np.nanmax(vals, axis=0) > np.nanmin(vals, axis=0))
    nan_taken_over = np.isnan(m[0]) & has[0] & (has[1:] & ~np.isnan(m[1:])).any(axis=0)
    return dict(none=int((reach == 0).sum()), one=int((reach == 1).sum()), several=int((reach >= 2).sum()),
                differ=int(((wmax != wnear) & (reach > 0)).sum()), value_tie=int((value_tie & (reach > 0)).sum()),
                distance_tie=int((d_tie & (reach > 0)).sum()), distance_tie_other_values=int(d_tie_other_values.sum()),
                first_radar_nan_yields=int(nan_taken_over.sum()), inf=int(np.isposinf(m).sum()))
