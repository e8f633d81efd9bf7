"""CPU-side checks of the column profile products (no GPU needed): known answers for the float64 restatement of the
contract (tests/column_profile_oracle.py), the refusals of ``rg_column_profile_f32`` and of the Python surface that are
decided before any device work, and the ABI bookkeeping (header, ctypes binding, version)."""
import ctypes
import os
import re

import numpy as np
import pytest

import column_profile_oracle as cpo
import radar_processor_amd as rg
from conftest import REPO
from radar_processor_amd import _native

P = 1 << 12                                  # a 16-byte aligned address that is never dereferenced
Z4 = np.array([0.0, 1000.0, 2000.0, 3000.0])
COL = np.array([40.0, 30.0, 20.0, 10.0], dtype=np.float32)
NAN = np.float32(np.nan)


# ---- the restatement ------------------------------------------------------------------------------------------------------
def test_echo_top_and_base_known_answers():
    assert cpo.echo_top_column(COL, Z4, 18.0) == np.float32(2200.0)        # 2000 + (20 - 18) / (20 - 10) * 1000
    assert cpo.echo_top_column(COL, Z4, 35.0) == np.float32(500.0)         # 0 + (40 - 35) / (40 - 30) * 1000
    assert cpo.echo_base_column(COL, Z4, 18.0) == np.float32(0.0)          # the bottom of the window: its own height
    assert cpo.echo_base_column(COL, Z4, 35.0) == np.float32(0.0)
    assert np.isnan(cpo.echo_top_column(COL, Z4, 50.0)) and np.isnan(cpo.echo_base_column(COL, Z4, 50.0))
    for fn in (cpo.echo_top_column, cpo.echo_base_column):
        assert fn(COL, Z4, 18.0).dtype == np.float32
    gap = COL.copy()
    gap[3] = NAN                                                             # a NaN neighbour: the level's own height
    assert cpo.echo_top_column(gap, Z4, 18.0) == np.float32(2000.0)
    assert cpo.echo_top_column(COL, Z4, 18.0, linear=False) == np.float32(2000.0)
    assert cpo.echo_top_column(COL, Z4, 35.0, linear=False) == np.float32(0.0)
    rising = COL[::-1].copy()                                                # 10 20 30 40: the base interpolates downwards
    assert cpo.echo_base_column(rising, Z4, 18.0) == np.float32(800.0)     # 1000 - (20 - 18) / (20 - 10) * 1000
    assert cpo.echo_base_column(rising, Z4, 18.0, linear=False) == np.float32(1000.0)
    assert cpo.echo_top_column(rising, Z4, 18.0) == np.float32(3000.0)     # the top of the window


def test_a_level_equal_to_the_threshold_reaches_it():
    col = np.array([5.0, 18.0, 5.0, NAN], dtype=np.float32)
    assert cpo.echo_top_column(col, Z4, 18.0) == np.float32(1000.0)        # (18 - 18) / (18 - 5) = 0
    assert cpo.echo_base_column(col, Z4, 18.0) == np.float32(1000.0)
    assert np.isnan(cpo.echo_top_column(col, Z4, np.nextafter(18.0, 19.0)))


def test_two_cells_top_from_the_upper_base_from_the_lower():
    z = np.arange(7) * 500.0
    col = np.array([0.0, 30.0, 10.0, 0.0, 25.0, 35.0, 15.0], dtype=np.float32)
    assert cpo.echo_top_column(col, z, 20.0) == np.float32(2500.0 + (35.0 - 20.0) / (35.0 - 15.0) * 500.0)
    assert cpo.echo_base_column(col, z, 20.0) == np.float32(500.0 - (30.0 - 20.0) / (30.0 - 0.0) * 500.0)
    # a window holds what lies inside it only: the upper cell alone, and its louder neighbours outside are never read
    assert cpo.echo_base_column(col, z, 20.0, lo=4, hi=5) == np.float32(2000.0)
    assert cpo.echo_top_column(col, z, 20.0, lo=1, hi=1) == np.float32(500.0)
    assert np.isnan(cpo.echo_top_column(col, z, 20.0, lo=2, hi=3))


def test_infinite_values_fall_to_the_level_height():
    inf = np.float32(np.inf)
    assert cpo.echo_top_column(np.array([inf, 10.0], dtype=np.float32), Z4[:2], 18.0) == np.float32(0.0)
    assert cpo.echo_top_column(np.array([30.0, -inf], dtype=np.float32), Z4[:2], 18.0) == np.float32(0.0)
    assert cpo.echo_base_column(np.array([-inf, 30.0], dtype=np.float32), Z4[:2], 18.0) == np.float32(1000.0)
    assert cpo.echo_base_column(np.array([10.0, inf], dtype=np.float32), Z4[:2], 18.0) == np.float32(1000.0)


def test_vil_known_answers():
    two = np.array([30.0, 30.0], dtype=np.float32)
    want = np.float32(3.44e-3 * 1000.0 ** (4.0 / 7.0))                      # 3.44e-6 * (1000)^(4/7) * 1000 m
    got = cpo.vil_column(two, Z4[:2])
    assert got.dtype == np.float32 and abs(float(got) - float(want)) <= float(np.spacing(want))
    loud = np.array([70.0, 70.0, 20.0], dtype=np.float32)
    capped = np.array([56.0, 56.0, 20.0], dtype=np.float32)
    assert cpo.vil_column(loud, Z4[:3], 56.0) == cpo.vil_column(capped, Z4[:3], 56.0)
    assert cpo.vil_column(loud, Z4[:3], 80.0) > cpo.vil_column(capped, Z4[:3], 80.0)
    assert np.isnan(cpo.vil_column(np.full(4, NAN), Z4))
    assert cpo.vil_column(np.array([NAN, 30.0, NAN], dtype=np.float32), Z4[:3], lo=1, hi=1) == np.float32(0.0)
    # a NaN level is no echo: half the layer's mean on either side of it
    holed = np.array([30.0, NAN, 30.0], dtype=np.float32)
    assert cpo.vil_column(holed, Z4[:3]) == np.float32(3.44e-6 * (500.0 ** (4.0 / 7.0) * 1000.0 + 500.0 ** (4.0 / 7.0) * 1000.0))
    grid = np.stack([COL, COL[::-1]], axis=1).reshape(4, 1, 2)
    np.testing.assert_array_equal(cpo.echo_top(grid, Z4, 18.0), np.float32([[2200.0, 3000.0]]))
    assert cpo.vil(grid, Z4).shape == (1, 2) and cpo.echo_base(grid, Z4, 18.0).dtype == np.float32


# ---- the C entry point: refusals decided on the host -----------------------------------------------------------------------
def _profile(grid=P, nz=4, n_xy=64, z_lo=0, z_hi=3, z_levels=P, thresholds=(18.0,), n=None, linear=1, top=P, base=None,
             vil_max=56.0, vil=None):
    lib = rg.load_library(require_device=False)
    arr = (ctypes.c_double * max(1, len(thresholds)))(*thresholds)
    return lib.rg_column_profile_f32(grid, nz, n_xy, z_lo, z_hi, z_levels, arr, len(thresholds) if n is None else n, linear,
                                     top, base, vil_max, vil, None)


def test_entry_point_refuses_bad_arguments():
    """Every call fails validation (or has nothing to do) before anything would be launched."""
    lib = rg.load_library(require_device=False)
    E = _native.RG_EINVAL
    assert _native.RG_MAX_PROFILE_THRESHOLDS == 4
    assert _profile(thresholds=(10.0, 20.0, 30.0, 40.0, 50.0)) == E and b"thresholds" in lib.rg_last_error()
    assert _profile(n=-1) == E
    assert _profile(grid=None) == E and b"null" in lib.rg_last_error()
    assert _profile(z_levels=None) == E
    assert _profile(top=None) == E and b"nothing to produce" in lib.rg_last_error()
    assert _profile(thresholds=(), top=P) == E and _profile(thresholds=(), top=None, base=P, vil=P) == E
    for bad in (float("nan"), float("inf"), float("-inf")):
        assert _profile(thresholds=(18.0, bad)) == E and b"not finite" in lib.rg_last_error()
        assert _profile(vil=P, vil_max=bad) == E and b"vil_max_dbz" in lib.rg_last_error()
    for lo, hi in ((-1, 3), (0, 4), (2, 1)):
        assert _profile(z_lo=lo, z_hi=hi) == E and b"window" in lib.rg_last_error(), (lo, hi)
    assert _profile(nz=0) == E and _profile(n_xy=-1) == E
    # valid, and nothing to do
    assert _profile(n_xy=0) == _native.RG_OK
    assert _profile(n_xy=0, thresholds=(), top=None, vil=P) == _native.RG_OK
    assert _profile(n_xy=0, thresholds=(1.0, 2.0, 3.0, 4.0), base=P, vil=P, linear=0) == _native.RG_OK


def test_symbol_is_declared_and_bound():
    header = open(os.path.join(REPO, "include", "radargrid_hip.h")).read()
    declared = set(re.findall(r"^(?:int|int64_t|const char\*)\s+(rg_\w+)\s*\(", header, flags=re.M))
    assert "rg_column_profile_f32" in declared and "rg_column_profile_f32" in _native.SIGNATURES
    assert declared == set(_native.SIGNATURES)
    restype, argtypes = _native.SIGNATURES["rg_column_profile_f32"]
    assert restype is ctypes.c_int32 and len(argtypes) == 14
    assert "#define RG_MAX_PROFILE_THRESHOLDS 4" in header and "#define RG_VERSION 104" in header
    lib = rg.load_library(require_device=False)
    assert lib.rg_version() == _native.ABI_VERSION == 104                  # a function was added; no signature changed
    assert hasattr(lib, "rg_column_profile_f32")


# ---- the Python surface: refusals decided before the device is touched ----------------------------------------------------
class _Geom:
    grid_shape = (4, 2, 3)
    grid_limits = ((0.0, 3000.0), (-1.0, 1.0), (-1.0, 1.0))


GRID = np.zeros((4, 2, 3), dtype=np.float32)


def test_python_surface_refusals():
    for name in ("column_profile", "echo_top", "echo_base", "vertically_integrated_liquid"):
        assert name in rg.__all__ and callable(getattr(rg, name))
    with pytest.raises(ValueError, match="nothing requested"):
        rg.column_profile(GRID, _Geom())
    with pytest.raises(ValueError, match="Unknown interpolation method: cubic"):
        rg.column_profile(GRID, _Geom(), echo_top=(18.0,), interpolation="cubic")
    with pytest.raises(ValueError, match="Unknown interpolation method"):
        rg.echo_top(GRID, _Geom(), interpolation="cubic")
    with pytest.raises(ValueError, match="Unknown interpolation method"):
        rg.echo_base(GRID, _Geom(), interpolation="spline")
    for bad in (float("nan"), float("inf")):
        with pytest.raises(ValueError, match="finite"):
            rg.echo_top(GRID, _Geom(), threshold=bad)
        with pytest.raises(ValueError, match="finite"):
            rg.column_profile(GRID, _Geom(), echo_base=(18.0, bad))
        with pytest.raises(ValueError, match="finite"):
            rg.vertically_integrated_liquid(GRID, _Geom(), max_dbz=bad)
    with pytest.raises(ValueError, match="levels"):
        rg.echo_top(np.zeros((5, 2, 3), dtype=np.float32), _Geom())
    with pytest.raises(ValueError, match="empty level window"):
        rg.echo_top(GRID, _Geom(), z_min_idx=3, z_max_idx=1)
    with pytest.raises(ValueError, match="empty level window"):
        rg.vertically_integrated_liquid(GRID, _Geom(), z_min_alt=5000.0)

    class Flat(_Geom):
        grid_limits = ((1000.0, 1000.0), (-1.0, 1.0), (-1.0, 1.0))
    with pytest.raises(ValueError, match="strictly increasing"):
        rg.echo_top(GRID, Flat())


def test_plane_products_profile_arguments():
    old = rg.PlaneProducts()
    assert (old.echo_top, old.echo_base, old.vil, old.vil_max_dbz, old.profile_interpolation) == ((), (), False, 56.0, "linear")
    assert not old.profile and old.columns and not old.needs_planes_mode
    # what a request without the new arguments held before is what it holds now
    assert (old.colmax, old.argmax, old.cappi, old.interpolation, old.fused, old.window) == (True, True, (), "linear", None,
                                                                                             (None, None, None, None))
    assert (old.colmin, old.colmean, old.ppi, old.ppi_interpolation, old.earth_curvature, old.ke) == (
        False, False, (), "linear", True, 4.0 / 3.0)
    assert repr(old).startswith("<radar_processor_amd.gridding.PlaneProducts object at ")
    spec = rg.PlaneProducts(echo_top=(18, 30.0, 18.0), echo_base=[18], vil=True, vil_max_dbz=50, profile_interpolation="nearest")
    assert spec.echo_top == (18.0, 30.0) and spec.echo_base == (18.0,) and all(isinstance(t, float) for t in spec.echo_top)
    assert spec.vil is True and spec.vil_max_dbz == 50.0 and spec.profile_interpolation == "nearest" and spec.profile
    assert not spec.needs_planes_mode                                        # the fused planes kernel does not produce them
    assert rg.PlaneProducts(colmax=False, argmax=False, vil=True).profile
    with pytest.raises(ValueError, match="fused=True"):
        rg.PlaneProducts(fused=True, vil=True)
    with pytest.raises(ValueError, match="fused=True"):
        rg.PlaneProducts(fused=True, echo_top=(18.0,))
    rg.PlaneProducts(fused=False, vil=True)
    with pytest.raises(ValueError, match="Unknown interpolation method"):
        rg.PlaneProducts(echo_top=(18.0,), profile_interpolation="cubic")
    with pytest.raises(ValueError, match="finite"):
        rg.PlaneProducts(echo_base=(float("nan"),))
    with pytest.raises(ValueError, match="finite"):
        rg.PlaneProducts(vil=True, vil_max_dbz=float("inf"))


def test_fused_products_pass_refuses_a_profile_product_before_any_device_work():
    torch = pytest.importorskip("torch")
    f = torch.zeros(8, dtype=torch.float32)                                   # a host tensor: device work would raise NativeUnavailable
    geom = rg.GridGeometry((2, 2, 2), ((0.0, 1000.0), (-1.0, 1.0), (-1.0, 1.0)), np.arange(9, dtype=np.int32),
                           np.arange(8, dtype=np.int32), np.ones(8, dtype=np.float32), toa=17000.0)
    with pytest.raises(ValueError, match="fused=True"):
        rg.grid_products_device(geom, [f], products=rg.PlaneProducts(vil=True), fused=True)
