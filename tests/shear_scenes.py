"""Inputs of the shear tests.  ``scenes()`` maps a name to the arguments of ``rg_velocity_llsd_f32`` (a dict: ``vel``, ``mask``,
``half_rays``, ``az_scale``, ``max_half_rays``, ``half_gates``, ``range_scale``, ``wrap``, ``min_valid``,
``min_fraction_q16``, ``centre_only``), ``reference(name)`` to the restatement's result for it (computed once, shared, never
changed); ``median_data()`` and ``median_cases()`` are the inputs of ``rg_polar_median_f32``.  tests/test_shear_scenes.py holds
that every scene contains what it is there for."""
import numpy as np

import shear_oracle as so

PLANE = dict(c0=1000, c1=37, c2=-11)               # scene 6: q = c0 + c1 * ray + c2 * gate in 2^-16 m/s
_SCENES = None
_REFERENCE = {}


def _scene(vel, half_rays, half_gates, wrap, *, mask=None, az_scale=None, max_half_rays=16, range_scale=1.0 / (65536.0 * 250.0),
           min_valid=6, min_fraction_q16=16384, centre_only=0):
    vel = np.ascontiguousarray(vel, dtype=np.float32)
    G = vel.shape[-1]
    half_rays = np.ascontiguousarray(np.broadcast_to(np.asarray(half_rays, np.int32), (G,)))
    if az_scale is None:                           # 1 degree rays, 250 m gates from 250 m on
        az_scale = 1.0 / (65536.0 * (250.0 * (1 + np.arange(G))) * np.pi / 180.0)
    return dict(vel=vel, mask=mask, half_rays=half_rays, az_scale=np.ascontiguousarray(az_scale, dtype=np.float64),
                max_half_rays=max_half_rays, half_gates=half_gates, range_scale=float(range_scale), wrap=int(wrap),
                min_valid=min_valid, min_fraction_q16=min_fraction_q16, centre_only=centre_only)


def _wind(rng, S, R, G, holes, masked):
    """A smooth wind plus noise, rounded to 1/64 m/s; NaN holes and masked holes."""
    az = 2.0 * np.pi * np.arange(R) / R
    vel = np.stack([(14.0 + 3.0 * s) * np.cos(az - 0.4 * s)[:, None] * np.linspace(0.3, 1.0, G)[None, :] for s in range(S)])
    vel = np.round((vel + rng.normal(0.0, 1.5, vel.shape)) * 64.0) / 64.0
    vel = vel.astype(np.float32)
    vel[rng.random(vel.shape) < holes] = np.nan
    mask = (rng.random(vel.shape) < masked).astype(np.uint8) * np.uint8(5) if masked else None
    return vel, mask


def _build():
    out = {}
    # 1  seams: multiples of no tile, half-widths that change inside a tile (a tile's halo is wider than most of its windows),
    #    40 must clamp to 16; with wrap a window crosses ray 0 / 36; the sweeps differ
    rng = np.random.default_rng(101)
    vel, mask = _wind(rng, 2, 37, 150, 0.15, 0.15)
    half = np.array([0, 1, 2, 5, 16, 40], np.int32)[(np.arange(150) // 7) % 6]
    for wrap in (1, 0):
        out["seams_wrap" if wrap else "seams_open"] = _scene(vel, half, 3, wrap, mask=mask)
    # 2  the exactly-full circle: R = 2 * 16 + 1, every ray is in every window once
    rng = np.random.default_rng(102)
    vel, _ = _wind(rng, 1, 33, 40, 0.10, 0.0)
    out["full_circle"] = _scene(vel, 16, 2, 1)
    # 3  small shapes
    rng = np.random.default_rng(103)
    out["one_ray"] = _scene(_wind(rng, 2, 1, 20, 0.1, 0.0)[0], 2, 2, 0, min_valid=3, min_fraction_q16=0)
    out["two_rays"] = _scene(_wind(rng, 2, 2, 20, 0.1, 0.0)[0], 2, 2, 0, min_valid=3, min_fraction_q16=0)
    out["one_gate"] = _scene(_wind(rng, 1, 10, 1, 0.0, 0.0)[0], 2, 1, 0, min_valid=3, min_fraction_q16=0)
    out["five_gates"] = _scene(_wind(rng, 2, 12, 5, 0.1, 0.0)[0], 3, 8, 0, min_valid=3, min_fraction_q16=0)
    # 4  degenerate windows: the valid gates lie on one line, D = 0
    rng = np.random.default_rng(104)
    vel, _ = _wind(rng, 1, 12, 12, 0.0, 0.0)
    a, g = np.meshgrid(np.arange(12), np.arange(12), indexing="ij")
    for name, keep in (("single_ray", a == 5), ("single_column", g == 7), ("diagonal", a == g)):
        out["degenerate_" + name] = _scene(vel, 3, 3, 0, mask=(~keep)[None].astype(np.uint8), min_valid=3, min_fraction_q16=0)
    # 5  magnitudes: +-16384 m/s, both half-widths 16.  Sweep 0: 17 rays of one sign, then 17 of the other -- at a ray where the
    #    sign turns, sum(i * q) is as large as a window allows and |P| is within a factor 4 of its bound.  Sweep 1: the sign
    #    alternates from ray to ray, a checkerboard along i -- the largest swings between neighbours, but (-1)^i is even in i, so
    #    sum(i * q) cancels exactly and P = 0: the large sums there are Sq and Sjq.  One value just above the limit and one inf are not valid.
    sign = np.stack([np.where((np.arange(68) % 34) < 17, 1.0, -1.0), np.where(np.arange(68) % 2 == 0, 1.0, -1.0)])
    vel = np.broadcast_to((16384.0 * sign)[:, :, None], (2, 68, 40)).astype(np.float32).copy()
    vel[0, 50, 2] = np.float32(16384.01)
    vel[0, 51, 3] = np.inf
    out["magnitudes"] = _scene(vel, 16, 16, 1, az_scale=np.full(40, 1e-9), range_scale=1e-9)
    # 6  a plane in fixed point, all valid, no wrap
    a, g = np.meshgrid(np.arange(50), np.arange(70), indexing="ij")
    q = PLANE["c0"] + PLANE["c1"] * a + PLANE["c2"] * g
    out["plane"] = _scene((q / 65536.0)[None], 1 + np.arange(70) % 6, 2, 0)
    # 7  thresholds: the same volume under other thresholds
    rng = np.random.default_rng(107)
    vel, mask = _wind(rng, 1, 20, 30, 0.25, 0.1)
    base = dict(min_valid=6, min_fraction_q16=0, centre_only=0)
    for name, kw in (("base", {}), ("min_valid", dict(min_valid=16)), ("fraction", dict(min_fraction_q16=52429)),
                     ("centre", dict(centre_only=1))):
        out["thresholds_" + name] = _scene(vel, 2, 2, 0, mask=mask, **{**base, **kw})
    # 9  more than one band of rays and more than one tile of gates, the widest halo in both directions
    rng = np.random.default_rng(109)
    vel, mask = _wind(rng, 2, 95, 70, 0.2, 0.1)
    half = np.array([16, 3, 0, 9, 1, 16, 2], np.int32)[(np.arange(70) // 5) % 7]
    for wrap in (1, 0):
        out["bands_wrap" if wrap else "bands_open"] = _scene(vel, half, 16, wrap, mask=mask, min_fraction_q16=8192)
    out["bands_narrow"] = _scene(vel, np.minimum(half, 2), 1, 1, mask=mask, max_half_rays=2)
    return out


def scenes():
    global _SCENES
    if _SCENES is None:
        _SCENES = _build()
    return _SCENES


def llsd_args(scene):
    return (scene["vel"], scene["mask"], scene["half_rays"], scene["az_scale"], scene["max_half_rays"], scene["half_gates"],
            scene["range_scale"], scene["wrap"], scene["min_valid"], scene["min_fraction_q16"], scene["centre_only"])


def reference(name):
    if name not in _REFERENCE:
        ref = so.llsd(*llsd_args(scenes()[name]))
        for plane in ref:
            plane.setflags(write=False)
        _REFERENCE[name] = ref
    return _REFERENCE[name]


def interior(name):
    """Gates whose window no edge clips."""
    s = scenes()[name]
    _, R, G = s["vel"].shape
    ka = so.clamp_half(s["half_rays"], s["max_half_rays"])
    a, g = np.meshgrid(np.arange(R), np.arange(G), indexing="ij")
    return ((a - ka[None, :] >= 0) & (a + ka[None, :] < R) & (g - s["half_gates"] >= 0) & (g + s["half_gates"] < G))[None]


# ---- 8  the median -----------------------------------------------------------------------------------------------------------
def median_data():
    """Two sweeps of 12 rays x 17 gates: values from a small set of quarters (many ties, no zero of either sign), NaN holes and
    masked holes, so that windows hold even and odd counts."""
    rng = np.random.default_rng(108)
    vel = (rng.integers(1, 12, (2, 12, 17)) * np.where(rng.random((2, 12, 17)) < 0.5, -0.25, 0.25)).astype(np.float32)
    vel[rng.random(vel.shape) < 0.2] = np.nan
    vel[1, 3, 4] = np.inf
    mask = (rng.random(vel.shape) < 0.1).astype(np.uint8)
    return vel, mask


def median_cases():
    """(half_rays, half_gates, wrap, min_valid, centre_only): all eight windows, each with wrap on and off and centre_only both
    ways; min_valid 1 and one that bites."""
    return [(hr, hg, wrap, min_valid, centre)
            for hr in range(3) for hg in range(3) if hr or hg
            for wrap in (1, 0) for centre in (1, 0)
            for min_valid in ((1, 4) if (hr, hg) in ((1, 1), (2, 2)) else (1,))]
