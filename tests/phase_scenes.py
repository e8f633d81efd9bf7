"""Scenes for the polar-domain phase processing (csrc/rg_phase.hip), each built to reach one thing; tests/test_phase_scenes.py
asserts on the CPU, through the oracle alone, that it does.  Dual-polarisation test data lives here, not in ``synthetic.py``.

Ray lengths and counts: ``G`` in {1, 2, 63, 64, 65, 128, 129, 200} x ``R`` in {1, 5, 9} (``SHAPES``) for all three calls: the
trips of 64 gates end inside, at and just after a seam, and the last workgroup of four rays is partial.

Unfold (``unfold_scenes()``):
``ramp_RxG``     a noisy ramp wrapped into [-180, 180) with NaN and masked gates;
``seams``        G = 200, one row per case -- 0: up-folds whose two gates are 63|64 and 127|128; 1: the previous valid gate two
                 trips back (gate 60, then 70 invalid gates: the whole trip 64 .. 127); 2: all invalid (NaN, +-inf, masked);
                 3: valid only at the last gate; 4: d exactly +half and -half (no fold) next to d one ulp beyond (a fold);
                 5: an up-fold, then down-folds with K returning through 0 and on below -2; 6: +-inf and masked gates planted
                 between the two gates of a fold;
``seams_180``    the same rows halved (exact in float32) under wrap = 180.

Fit (``fit_scenes()``):
``fit_RxG``      noisy unfolded ramps with NaN gaps, four classes (half-windows 2, 7, 40, 255: G < L everywhere but at 200), dbz
                 on the edges and NaN; ``centre_only`` alternates with the shape;
``l1`` / ``l255``  G = 200 with L = 1 and L = 255: the long window is clipped at both ends and spans four trips;
``sparse``       G = 65, L = 5, min_valid = 3: rows of few valid gates -- N = min_valid and min_valid - 1 side by side, two valid
                 gates (min_valid = 2 in ``pairs``: den > 0), one valid gate (den = 0), all valid gates of a window on one side;
``limits``       |phi| = 2^14 exactly (valid) and one ulp above (invalid), +-inf;
``gaps`` / ``gaps_centre``   the same gappy rays with centre_only off and on.

Attenuation (``attenuation_scenes()``):
``att_RxG``      rising noisy phi_s with NaN runs, phi0 NULL, with ZDR;
``paths``        G = 200, one row per case -- 0: first defined phi_s in trip 2 (gate 130); 1: NaN runs across the seams 63|64 and
                 127|128; 2: a decreasing phi_s (the maximum holds); 3: phi_s below its origin everywhere but gate 0 (all zeros);
                 4: a ramp to 300 degrees (with max_dphi = 100: the cap is reached mid-ray); 5: no phi_s at all; 6: NaN dbz;
                 7: +inf and -inf in phi_s;
``paths_phi0``   the same with phi0 given: finite for some rays (above every value for row 3), NaN for others.

``weather()``    9 rays x 300 gates at 240 m: KDP blocks of 2 deg/km (gates 60 .. 109) and 4 deg/km (gates 150 .. 194), a system
                 offset of +100 degrees, noise of sigma = 3 degrees, 5 % NaN, so PHIDP ends 134.4 degrees above its start and
                 folds once.  With L = 15: unfolded within 1.2e-5 degrees of the unwrapped truth, 2.02 +- 0.11 deg/km in the
                 first block, and an end-of-ray path of 134.1 .. 137.0 degrees above the offset (given as phi0).

Everything is deterministic, computed once, read-only, and importable without a GPU."""
import functools
from typing import NamedTuple, Optional

import numpy as np

SHAPES = tuple((R, G) for G in (1, 2, 63, 64, 65, 128, 129, 200) for R in (1, 5, 9))
EDGES4 = (10.0, 30.0, 45.0)
HALF4 = (2, 7, 40, 255)


class Unfold(NamedTuple):
    phidp: np.ndarray               # float32 [R, G]
    mask: Optional[np.ndarray]      # uint8 [R, G]
    wrap: float


class Fit(NamedTuple):
    phi: np.ndarray                 # float32 [R, G], unfolded
    dbz: Optional[np.ndarray]
    edges: tuple
    half_window: tuple
    min_valid: int
    centre_only: bool
    spacing: float


class Attenuation(NamedTuple):
    phi_s: np.ndarray
    phi0: Optional[np.ndarray]      # float32 [R]
    dbz: np.ndarray
    zdr: Optional[np.ndarray]
    alpha: float
    beta: float
    max_dphi: float


class Weather(NamedTuple):
    phidp: np.ndarray               # wrapped, noisy, with NaN
    truth: np.ndarray               # float64: the noisy unwrapped phase the wrapped one was made from
    clean: np.ndarray               # float64: the noise-free phase
    dbz: np.ndarray                 # attenuated
    zdr: np.ndarray
    dbz_true: np.ndarray
    spacing: float
    blocks: tuple                   # ((gate_lo, gate_hi, kdp), ...)
    offset: float                   # the system offset in degrees: what a user who knows it passes as phi0


def _frozen(scene):
    for a in scene:
        if isinstance(a, np.ndarray):
            a.setflags(write=False)
    return scene


def _wrapped(truth, wrap=360.0):
    """float64 phase -> float32 in [-wrap/2, wrap/2)."""
    return (truth - wrap * np.floor((truth + 0.5 * wrap) / wrap)).astype(np.float32)


def _holes(rng, a, share):
    a = a.copy()
    a[rng.random(a.shape) < share] = np.nan
    return a


# ---- unfold --------------------------------------------------------------------------------------------------------------------
def _seam_rows():
    G = 200
    rows = np.zeros((7, G), np.float32)
    mask = np.zeros((7, G), np.uint8)
    rows[0, :64] = 170.0
    rows[0, 64:128] = np.linspace(-100.0, 170.0, 64)
    rows[0, 128:] = -100.0
    rows[1] = 150.0
    rows[1, 61:131] = np.nan
    rows[1, 131:] = -120.0
    rows[2] = np.nan
    rows[2, 10], rows[2, 70], rows[2, 150] = np.inf, -np.inf, 33.0
    mask[2, 150] = 1
    rows[3] = np.nan
    rows[3, G - 1] = 77.0
    rows[4] = 0.0
    above = np.nextafter(np.float32(180.0), np.float32(np.inf))
    rows[4, 5], rows[4, 7], rows[4, 9], rows[4, 11] = 180.0, -180.0, above, -above
    up = np.array([170.0, 60.0, -50.0, -170.0], np.float32)              # falls without a fold, then wraps to 170: k = -1
    rows[5, :4] = [100.0, 170.0, -170.0, 170.0]                          # K: 0, 0, +1, 0
    rows[5, 4:] = np.tile(up, 49)                                        # ... -1 and below
    rows[5, 100:] = rows[5, 99]
    rows[6] = np.linspace(120.0, 170.0, G)
    rows[6, 60:] -= 360.0                                                # a fold between gates 59 and 60 ...
    rows[6, 60], rows[6, 61] = np.inf, -np.inf                           # ... whose upper gate is now gate 63
    rows[6, 62] = 0.0
    mask[6, 62] = 7
    rows[6, 128], mask[6, 128] = 170.0, 1                                # a masked gate that would fold back
    return rows, mask


@functools.lru_cache(maxsize=None)
def unfold_scenes():
    out = {}
    for R, G in SHAPES:
        rng = np.random.default_rng(1000 * R + G)
        truth = 80.0 + np.cumsum(rng.uniform(0.0, 6.0, (R, G)), axis=1) + rng.normal(0.0, 2.0, (R, G))
        phidp = _holes(rng, _wrapped(truth), 0.1)
        mask = (rng.random((R, G)) < 0.1).astype(np.uint8) * np.uint8(3)
        out[f"ramp_{R}x{G}"] = _frozen(Unfold(phidp, mask, 360.0))
    rows, mask = _seam_rows()
    out["seams"] = _frozen(Unfold(rows, mask, 360.0))
    out["seams_180"] = _frozen(Unfold(rows * np.float32(0.5), mask.copy(), 180.0))
    return out


# ---- fit -----------------------------------------------------------------------------------------------------------------------
def _ramp(rng, R, G, holes=0.1):
    phi = 100.0 + np.cumsum(rng.uniform(0.0, 1.5, (R, G)), axis=1) + rng.normal(0.0, 3.0, (R, G))
    return _holes(rng, phi.astype(np.float32), holes)


def _class_dbz(rng, R, G):
    """dBZ spanning the four classes, exactly on the edges at every 5th gate and NaN at every 7th."""
    dbz = rng.uniform(-5.0, 60.0, (R, G)).astype(np.float32)
    flat = dbz.reshape(-1)
    flat[::5] = np.resize(np.array(EDGES4, np.float32), flat[::5].shape)
    flat[::7] = np.nan
    return dbz


def _sparse():
    G = 65
    phi = np.full((6, G), np.nan, np.float32)
    value = lambda g: np.float32(50.0 + 0.37 * g)                        # noqa: E731
    for g in (10, 12, 15, 16):                                           # row 0: windows of 4, 3 and 2 valid gates
        phi[0, g] = value(g)
    for g in (20, 44):                                                   # row 1: two valid gates, 24 apart
        phi[1, g] = value(g)
    phi[2, 30] = value(30)                                               # row 2: one valid gate
    phi[3, :10] = value(np.arange(10))                                   # row 3: gates 10 .. 14 see valid gates on one side only
    phi[4, 63], phi[4, 64] = value(63), value(64)                        # row 4: the two gates either side of the seam
    phi[5] = value(np.arange(G))
    phi[5, 31:34] = np.nan
    return phi


@functools.lru_cache(maxsize=None)
def fit_scenes():
    out = {}
    for n, (R, G) in enumerate(SHAPES):
        rng = np.random.default_rng(2000 * R + G)
        out[f"fit_{R}x{G}"] = _frozen(Fit(_ramp(rng, R, G), _class_dbz(rng, R, G), EDGES4, HALF4, 3, bool(n % 2), 240.0))
    rng = np.random.default_rng(7)
    long_rays = _ramp(rng, 2, 200)
    out["l1"] = _frozen(Fit(long_rays, None, (), (1,), 2, False, 240.0))
    out["l255"] = _frozen(Fit(long_rays.copy(), None, (), (255,), 8, False, 240.0))
    out["sparse"] = _frozen(Fit(_sparse(), None, (), (5,), 3, False, 125.0))
    out["pairs"] = _frozen(Fit(_sparse(), None, (), (30,), 2, False, 125.0))
    limit = np.float32(16384.0)
    phi = np.tile(np.linspace(16000.0, 16380.0, 70).astype(np.float32), (3, 1))
    phi[0, 20], phi[0, 40] = limit, np.nextafter(limit, np.float32(np.inf))
    phi[1] = -phi[1]
    phi[1, 20], phi[1, 40] = -limit, np.nextafter(-limit, np.float32(-np.inf))
    phi[2, 20], phi[2, 40] = np.inf, -np.inf
    out["limits"] = _frozen(Fit(phi, None, (), (4,), 3, False, 240.0))
    gappy = _ramp(np.random.default_rng(8), 5, 129, holes=0.35)
    out["gaps"] = _frozen(Fit(gappy, None, (), (3,), 3, False, 240.0))
    out["gaps_centre"] = _frozen(Fit(gappy.copy(), None, (), (3,), 3, True, 240.0))
    return out


# ---- attenuation ---------------------------------------------------------------------------------------------------------------
def _paths():
    G = 200
    rng = np.random.default_rng(9)
    phi = np.zeros((8, G), np.float32)
    x = np.arange(G, dtype=np.float32)
    phi[0] = 90.0 + 0.5 * x
    phi[0, :130] = np.nan
    phi[1] = 20.0 + 0.25 * x + rng.normal(0.0, 0.5, G).astype(np.float32)
    phi[1, 58:70] = np.nan
    phi[1, 120:136] = np.nan
    phi[2] = 150.0 - 0.5 * x
    phi[2, 40] = 155.0                                                   # one gate above the origin: the path holds 5 from there
    phi[3] = 60.0 - 0.1 * x
    phi[4] = 1.5 * x
    phi[5] = np.nan
    phi[6] = 10.0 + 0.3 * x
    phi[7] = 5.0 + 0.2 * x
    phi[7, 70], phi[7, 150] = -np.inf, np.inf
    dbz = rng.uniform(0.0, 55.0, (8, G)).astype(np.float32)
    dbz[6, ::3] = np.nan
    dbz[5, 17] = np.nan
    zdr = rng.uniform(-1.0, 4.0, (8, G)).astype(np.float32)
    return phi, dbz, zdr


@functools.lru_cache(maxsize=None)
def attenuation_scenes():
    out = {}
    for R, G in SHAPES:
        rng = np.random.default_rng(3000 * R + G)
        phi = (30.0 + np.cumsum(rng.uniform(-0.5, 1.5, (R, G)), axis=1)).astype(np.float32)
        for r in range(R):                                               # NaN runs, some from gate 0
            start = int(rng.integers(0, G))
            phi[r, start:start + int(rng.integers(1, 40))] = np.nan
        if R > 1:
            phi[1, :G // 2] = np.nan
        dbz = _holes(rng, rng.uniform(0.0, 55.0, (R, G)).astype(np.float32), 0.1)
        zdr = rng.uniform(-1.0, 4.0, (R, G)).astype(np.float32)
        out[f"att_{R}x{G}"] = _frozen(Attenuation(phi, None, dbz, zdr, 0.08, 0.02, 360.0))
    phi, dbz, zdr = _paths()
    out["paths"] = _frozen(Attenuation(phi, None, dbz, zdr, 0.08, 0.02, 100.0))
    phi0 = np.array([np.nan, 25.0, np.nan, 70.0, -10.0, 3.0, np.nan, 0.0], np.float32)
    out["paths_phi0"] = _frozen(Attenuation(phi.copy(), phi0, dbz.copy(), None, 0.25, 0.035, 100.0))
    return out


# ---- the weather scene ---------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def weather():
    R, G, spacing = 9, 300, 240.0
    blocks = ((60, 110, 2.0), (150, 195, 4.0))
    rng = np.random.default_rng(2024)
    kdp = np.zeros(G)
    for lo, hi, k in blocks:
        kdp[lo:hi] = k
    clean = np.tile(100.0 + np.cumsum(2.0 * kdp * spacing / 1000.0), (R, 1))          # two-way degrees
    truth = clean + rng.normal(0.0, 3.0, (R, G))
    phidp = _holes(rng, _wrapped(truth), 0.05)
    dbz_true = np.full((R, G), 22.0)
    dbz_true[:, 60:110], dbz_true[:, 150:195] = 46.0, 52.0
    dbz_true += rng.normal(0.0, 1.0, (R, G))
    zdr_true = 0.4 + 0.04 * (dbz_true - 20.0)
    path = clean - 100.0
    dbz = (dbz_true - 0.08 * path).astype(np.float32)
    zdr = (zdr_true - 0.02 * path).astype(np.float32)
    return _frozen(Weather(phidp, truth, clean, dbz, zdr, dbz_true.astype(np.float32), spacing, blocks, 100.0))
