"""The rim-case generator (oracle/roi_rim.py) on the CPU: its float32 emulation of the ROI kernel's distance against
exact rational arithmetic, its labels against direct float64 evaluation, its case counts and its determinism."""
from fractions import Fraction

import numpy as np
import pytest

from oracle import roi_rim

GEOM = dict(grid_shape=(2, 5, 19), grid_limits=((500.0, 3000.0), (-5e3, 5e3), (-22.5e3, 22.5e3)), min_radius=1000.0,
            beam_factor=0.0)
BEAM = dict(grid_shape=(2, 5, 19), grid_limits=((1000.0, 5000.0), (-8e3, 8e3), (-36e3, 36e3)), min_radius=100.0,
            beam_factor=0.05)


def _fma_exact(a, b, c):
    return roi_rim._round_f32_exact(Fraction(float(a)) * Fraction(float(b)) + Fraction(float(c)))


def test_vectorised_fmaf_rounds_once():
    """Random operands and operands built so that rounding a*b + c to float64 first and then to float32 would round
    twice (the sum lies just off a float32 midpoint)."""
    rng = np.random.default_rng(0)
    a = rng.uniform(-3e3, 3e3, 4000).astype(np.float32)
    b = rng.uniform(-3e3, 3e3, 4000).astype(np.float32)
    c = rng.uniform(0, 2e7, 4000).astype(np.float32)
    # (1 - 2^-20) * -(1 + 2^-20) + (2^24 + 2) = 2^24 + 1 + 2^-40: float64 rounds it onto the float32 midpoint 2^24 + 1,
    # which then goes to even (2^24); rounded once it is 2^24 + 2.  The mirrored case rounds down.
    t = np.float32(1.0 - 2.0 ** -20), np.float32(1.0 + 2.0 ** -20)
    a = np.concatenate([a, np.float32([t[0], -t[0]])])
    b = np.concatenate([b, np.float32([-t[1], t[1]])])
    c = np.concatenate([c, np.float32([2.0 ** 24 + 2.0, -(2.0 ** 24 + 2.0)])])
    got = roi_rim._fmaf(a, b, c)
    want = np.array([_fma_exact(x, y, z) for x, y, z in zip(a, b, c)], dtype=np.float32)
    np.testing.assert_array_equal(got.view(np.int32), want.view(np.int32))
    naive = (a.astype(np.float64) * b + c).astype(np.float32)
    assert np.any(naive != want)           # the double rounding the emulation avoids does happen here


@pytest.mark.parametrize("geom", [GEOM, BEAM], ids=["minr", "beam"])
def test_labels_against_direct_evaluation(geom):
    cloud = roi_rim.rim_cloud(seed=3, **geom)
    assert cloud.misses == 0 and len(cloud) > 100
    zc, yc, xc = roi_rim.voxel_centres(geom["grid_shape"], geom["grid_limits"])
    nz, ny, nx = geom["grid_shape"]
    for i in range(len(cloud)):
        iz, rem = divmod(int(cloud.voxel[i]), ny * nx)
        iy, ix = divmod(rem, nx)
        x, y, z = float(xc[ix]), float(yc[iy]), float(zc[iz])
        r = max(geom["min_radius"], float(np.sqrt(x * x + y * y + z * z)) * geom["beam_factor"])
        r2 = r * r
        gx, gy, gz = (float(v) for v in (cloud.gx[i], cloud.gy[i], cloud.gz[i]))
        d2 = (gx - x) * (gx - x) + (gy - y) * (gy - y) + (gz - z) * (gz - z)
        d2f = roi_rim.d2f_exact(cloud.gx[i], cloud.gy[i], cloud.gz[i], xc[ix], yc[iy], zc[iz])
        r2f = np.float32(r2)
        r2_lo = np.float32(r2 * (1.0 - 2e-6)) * (np.float32(1.0) - np.float32(2.4e-7))
        r2_hi = np.float32(r2 * (1.0 + 2e-6)) * (np.float32(1.0) + np.float32(2.4e-7))
        band = r2_lo < d2f <= r2_hi
        case = cloud.case[i]
        if case == "A":
            assert d2 < r2 and d2f >= r2f
        elif case == "B":
            assert d2 < r2 and band and d2f < r2f
        elif case == "C":
            assert d2 >= r2 and band and d2f < r2f
        elif case == "D":
            assert d2 == r2
        else:
            assert case == "E"
            ulps = [abs(int(np.float32(d2f).view(np.int32)) - int(np.float32(t).view(np.int32))) for t in (r2_lo, r2_hi)]
            assert min(ulps) <= roi_rim.E_ULPS
        # the kernel's rule gives the float64 answer wherever the planted gate lies
        kernel_in = d2f <= r2_lo or (d2f <= r2_hi and d2 < r2)
        assert kernel_in == (d2 < r2)


def test_case_counts_and_determinism():
    a = roi_rim.rim_cloud(seed=5, **GEOM)
    b = roi_rim.rim_cloud(seed=5, **GEOM)
    c = roi_rim.rim_cloud(seed=6, **GEOM)
    for f in ("gx", "gy", "gz", "voxel", "case"):
        np.testing.assert_array_equal(getattr(a, f), getattr(b, f))
    assert not np.array_equal(a.gx, c.gx)
    counts = a.counts()
    assert all(counts[k] >= 20 for k in roi_rim.CASES), counts
    assert sum(counts.values()) == len(a)
    beam = roi_rim.rim_cloud(seed=5, **BEAM).counts()
    assert all(beam[k] >= 20 for k in "ABCE"), beam
    np.testing.assert_array_equal(roi_rim.relabel(a, **GEOM), a.case)


def test_pythagorean_offsets_and_vertical_gates():
    offs = roi_rim.pythagorean_offsets(1000)
    assert np.all((offs ** 2).sum(axis=1) == 1e6) and len(offs) > 100
    assert {(600.0, 800.0, 0.0), (360.0, 480.0, 800.0)} <= set(map(tuple, offs))
    shape, limits = (3, 3, 3), ((2345.6, 6000.0), (-5e3, 5e3), (-5e3, 5e3))
    cloud = roi_rim.vertical_cloud(shape, limits, 100.0, 0.3, [4, 13, 22])
    zc = roi_rim.voxel_centres(shape, limits)[0].astype(np.float64)
    assert np.all(cloud.gx == 0) and np.all(cloud.gy == 0)
    r = 0.3 * zc[cloud.voxel // 9]
    d2 = (cloud.gz.astype(np.float64) - zc[cloud.voxel // 9]) ** 2
    inside = np.arange(len(cloud)) % 2 == 0
    assert np.all((d2 < r * r) == inside)
    # innermost / outermost: one float32 step further out / in flips the side
    step = np.where(cloud.gz > zc[cloud.voxel // 9], 1, -1) * np.where(inside, 1, -1)
    moved = np.array([np.nextafter(z, np.float32(np.inf) if s > 0 else np.float32(-np.inf)) for z, s in zip(cloud.gz, step)])
    d2m = (moved.astype(np.float64) - zc[cloud.voxel // 9]) ** 2
    assert np.all((d2m < r * r) != inside)
