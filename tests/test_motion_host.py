"""The host side of ``radar_processor_amd/motion.py`` with no device present: every ``ValueError`` of the Python surface is
raised before the library is loaded (the loader is monkeypatched to raise), the lattice arithmetic, and
``motion_to_velocity``."""
from types import SimpleNamespace

import numpy as np
import pytest

import motion_oracle as mo
import radar_processor_amd as rg
from radar_processor_amd import _native, motion


class DeviceTouched(AssertionError):
    pass


@pytest.fixture
def no_device(monkeypatch):
    def refuse(*args, **kwargs):
        raise DeviceTouched("the library was loaded before the arguments were validated")
    monkeypatch.setattr(_native, "load_library", refuse)
    monkeypatch.setattr(_native, "device", refuse)


PLANE = np.zeros((40, 48), dtype=np.float32)
STACK = np.zeros((3, 40, 48), dtype=np.float32)
LEVELS = np.zeros((40, 48), dtype=np.uint8)
FIELD = np.zeros((4, 5, 2), dtype=np.float32)
LAT = (7.5, 7.5, 8.0, 8.0, 4, 5)


def _grid(motion_=None, shape=(40, 48), lead_axis=False):
    m = np.zeros((1, 4, 5, 2) if lead_axis else (4, 5, 2), dtype=np.float32) if motion_ is None else motion_
    return motion.MotionGrid(m, np.ones(m.shape[:-1], dtype=np.float32), np.zeros(m.shape, dtype=np.int16), 16, 8, 6, shape,
                             7.5, 8.0)


def test_valid_arguments_reach_the_loader(no_device):
    """The fixture works: with nothing to refuse, each function gets as far as loading the library."""
    for call in (lambda: motion.quantize_planes_device(PLANE), lambda: motion.estimate_motion_device(PLANE, PLANE),
                 lambda: motion.estimate_motion_device(LEVELS, LEVELS, block=16, stride=8, search=6),
                 lambda: motion.advect_device(PLANE, FIELD, [1.0], lattice=LAT), lambda: motion.advect_device(STACK, _grid(), 2),
                 lambda: motion.nowcast_device(PLANE, PLANE, [1, 2], block=16, method="bilinear")):
        with pytest.raises(DeviceTouched):
            call()


def test_quantize_refusals(no_device):
    q = motion.quantize_planes_device
    for bad in (PLANE.astype(np.float64), PLANE[0], np.zeros((0, 4, 4), dtype=np.float32), np.zeros((1, 2, 3, 4), dtype=np.float32),
                [[1.0]]):
        with pytest.raises(ValueError, match="planes"):
            q(bad)
    for lo, hi in ((0.0, 0.0), (5.0, 1.0), (np.nan, 1.0), (0.0, np.inf), (0.0, 1e-44)):
        with pytest.raises(ValueError, match="lo"):
            q(PLANE, lo, hi)
    with pytest.raises(ValueError, match="mask of shape"):
        q(PLANE, mask=np.zeros((40, 47), dtype=np.uint8))
    with pytest.raises(ValueError, match="mask of shape"):
        q(STACK, mask=np.zeros((40, 48), dtype=np.uint8))


def test_estimate_refusals(no_device):
    e = motion.estimate_motion_device
    with pytest.raises(ValueError, match="prev must be"):
        e(PLANE.astype(np.float64), PLANE)
    with pytest.raises(ValueError, match="differ"):
        e(PLANE, PLANE[:, :-1])
    with pytest.raises(ValueError, match="differ"):
        e(PLANE[None], PLANE)
    with pytest.raises(ValueError, match="quantise both or neither"):
        e(PLANE, LEVELS)
    for block in (0, 2, 6, 68, 16.0, True, "16"):
        with pytest.raises(ValueError, match="block must be"):
            e(PLANE, PLANE, block=block)
    for stride in (0, -1, 1.5):
        with pytest.raises(ValueError, match="stride must be"):
            e(PLANE, PLANE, stride=stride)
    for search in (-1, 33, 2.0):
        with pytest.raises(ValueError, match="search must be"):
            e(PLANE, PLANE, search=search)
    for min_echo in (0, 16 * 16 + 1, 3.5):
        with pytest.raises(ValueError, match="min_echo must be"):
            e(PLANE, PLANE, block=16, min_echo=min_echo)
    with pytest.raises(ValueError, match="smaller than a block"):
        e(PLANE, PLANE, block=44)
    with pytest.raises(ValueError, match="lo and hi"):
        e(PLANE, PLANE, lo=3.0, hi=3.0)
    with pytest.raises(ValueError, match="mask_next of shape"):
        e(PLANE, PLANE, mask_next=np.zeros((2, 2), dtype=np.uint8))
    with pytest.raises(ValueError, match="uint8 levels already"):
        e(LEVELS, LEVELS, mask_prev=LEVELS)


def test_fill_refusals(no_device):
    with pytest.raises(ValueError, match="MotionGrid"):
        motion.fill_motion_device(FIELD)
    with pytest.raises(ValueError, match="NaN"):
        motion.fill_motion_device(_grid(), float("nan"))
    with pytest.raises(ValueError, match="tensors"):
        motion.fill_motion_device(_grid())                               # ndarrays: not what estimate_motion_device returned


def test_advect_refusals(no_device):
    a = motion.advect_device
    with pytest.raises(ValueError, match="planes must be"):
        a(LEVELS, FIELD, [1.0], lattice=LAT)
    for bad in (FIELD.astype(np.float64), FIELD[..., :1], FIELD[0], "field"):
        with pytest.raises(ValueError, match="motion must be"):
            a(PLANE, bad, [1.0], lattice=LAT)
    with pytest.raises(ValueError, match="needs a lattice"):
        a(PLANE, FIELD, [1.0])
    with pytest.raises(ValueError, match="nodes for motion"):
        a(PLANE, FIELD, [1.0], lattice=(0, 0, 1, 1, 5, 4))
    for lat in ((0, 0, 0.0, 1, 4, 5), (0, 0, 1, -1.0, 4, 5), (np.nan, 0, 1, 1, 4, 5), (0, np.inf, 1, 1, 4, 5), (0, 0, 1, 1, 0, 5),
                (0, 0, 1, 1, 4.5, 5), (0, 0, 1, 1), "lattice"):
        with pytest.raises(ValueError, match="lattice"):
            a(PLANE, FIELD, [1.0], lattice=lat)
    nan_field = FIELD.copy()
    nan_field[1, 2, 0] = np.nan
    with pytest.raises(ValueError, match="fill it first"):
        a(PLANE, nan_field, [1.0], lattice=LAT)
    with pytest.raises(ValueError, match="own lattice"):
        a(PLANE, _grid(), [1.0], lattice=LAT)
    with pytest.raises(ValueError, match="estimated on planes"):
        a(PLANE, _grid(shape=(40, 56)), [1.0])
    with pytest.raises(ValueError, match="ONE plane pair"):
        a(PLANE, _grid(np.zeros((2, 4, 5, 2), dtype=np.float32)), [1.0])
    with pytest.raises(ValueError, match="at most 16 leads"):
        a(PLANE, FIELD, list(range(17)), lattice=LAT)
    for leads in ([np.nan], [1.0, np.inf], ["soon"], [None]):
        with pytest.raises(ValueError, match="leads must be"):
            a(PLANE, FIELD, leads, lattice=LAT)
    with pytest.raises(ValueError, match="method must be"):
        a(PLANE, FIELD, [1.0], lattice=LAT, method="cubic")
    for substeps in (0, 17, 2.0, True):
        with pytest.raises(ValueError, match="substeps must be"):
            a(PLANE, FIELD, [1.0], lattice=LAT, substeps=substeps)
    with pytest.raises(ValueError, match="out must be a tensor of shape"):
        a(PLANE, FIELD, [1.0, 2.0], lattice=LAT, out=np.zeros((2, 40, 48), dtype=np.float32))


def test_nowcast_refusals(no_device):
    with pytest.raises(ValueError, match="unknown keyword"):
        motion.nowcast_device(PLANE, PLANE, [1.0], blocks=16)
    with pytest.raises(ValueError, match="one float32"):
        motion.nowcast_device(STACK, STACK, [1.0])
    with pytest.raises(ValueError, match="leads must be"):
        motion.nowcast_device(PLANE, PLANE, [np.nan])
    with pytest.raises(ValueError, match="method must be"):
        motion.nowcast_device(PLANE, PLANE, [1.0], method="cubic")
    with pytest.raises(ValueError, match="block must be"):
        motion.nowcast(PLANE, PLANE, [1.0], block=5)
    # the later stages' arguments are refused before the first stage runs
    with pytest.raises(ValueError, match="substeps must be"):
        motion.nowcast_device(PLANE, PLANE, [1.0], substeps=0)
    with pytest.raises(ValueError, match="out must be a tensor of shape"):
        motion.nowcast_device(PLANE, PLANE, [1.0], out=np.zeros((1, 40, 48), dtype=np.float32))
    with pytest.raises(ValueError, match="min_score"):
        motion.nowcast_device(PLANE, PLANE, [1.0], min_score=float("nan"))


def test_lattice_arithmetic():
    for (h, w), B, S in (((61, 83), 16, 8), ((45, 71), 16, 8), ((2000, 2000), 32, 16), ((9, 13), 4, 8), ((64, 64), 64, 1),
                         ((130, 140), 64, 8), ((17, 16), 16, 3)):
        lat = motion.block_lattice((h, w), B, S)
        assert lat == mo.block_lattice((h, w), B, S)
        assert (lat.origin_y, lat.origin_x, lat.step_y, lat.step_x) == ((B - 1) / 2.0, (B - 1) / 2.0, float(S), float(S))
        # the last block fits, the one after it does not
        assert (lat.ny - 1) * S + B <= h < lat.ny * S + B and (lat.nx - 1) * S + B <= w < lat.nx * S + B
    assert motion.block_lattice((2000, 2000), 32, 16)[-2:] == (124, 124)
    assert motion.block_lattice((3, 61, 83), 16, 8)[-2:] == (6, 9)      # a leading axis is ignored
    with pytest.raises(ValueError, match="smaller than a block"):
        motion.block_lattice((15, 83), 16, 8)
    # a MotionGrid carries the lattice of its blocks: ((B - 1) / 2, S)
    grid = _grid(lead_axis=True)
    assert grid.lattice == motion.Lattice(7.5, 7.5, 8.0, 8.0, 4, 5) == motion.block_lattice((40, 48), 16, 8)
    assert (grid.origin, grid.step) == ((16 - 1) / 2, 8)
    assert motion.MotionGrid._fields == ("motion", "score", "disp", "block", "stride", "search", "shape", "origin", "step")
    # the node of a block is the centre of its pixels
    assert grid.lattice.origin_y + 2 * grid.lattice.step_y == np.arange(2 * 8, 2 * 8 + 16).mean()


def test_motion_to_velocity():
    geometry = SimpleNamespace(grid_shape=(20, 481, 961), grid_limits=((0.0, 15e3), (-120e3, 120e3), (-240e3, 240e3)))
    vectors = np.array([[[3.0, -5.0], [0.0, 0.0]], [[1.5, 2.25], [np.nan, 1.0]]], dtype=np.float32)
    u, v = rg.motion_to_velocity(vectors, geometry, 300.0)              # 500 m steps, 5 minutes
    assert u.dtype == v.dtype == np.float64 and u.shape == v.shape == (2, 2)
    assert u[0, 0] == -5.0 * 500.0 / 300.0 and v[0, 0] == 3.0 * 500.0 / 300.0        # dx is east, dy is north
    assert u[1, 0] == 3.75 and v[1, 0] == 2.5 and np.isnan(v[1, 1]) and u[1, 1] == 500.0 / 300.0
    # steps of the two axes are taken apart
    skew = SimpleNamespace(grid_shape=(11, 21), grid_limits=((0.0, 10e3), (0.0, 5e3)))
    u, v = rg.motion_to_velocity(np.array([2.0, 2.0]), skew, 100.0)
    assert (float(u), float(v)) == (5.0, 20.0)
    grid = _grid(np.full((4, 5, 2), 2.0, dtype=np.float32), shape=(11, 21))
    u2, v2 = rg.motion_to_velocity(grid, skew, 100.0)
    assert u2.shape == (4, 5) and (u2 == 5.0).all() and (v2 == 20.0).all()
    for interval in (0.0, -1.0, np.nan, np.inf):
        with pytest.raises(ValueError, match="interval_seconds"):
            rg.motion_to_velocity(vectors, geometry, interval)
    with pytest.raises(ValueError, match="geometry must carry"):
        rg.motion_to_velocity(vectors, object(), 300.0)
    with pytest.raises(ValueError, match="geometry: at least"):
        rg.motion_to_velocity(vectors, SimpleNamespace(grid_shape=(1, 5), grid_limits=((0, 1), (0, 1))), 300.0)
    with pytest.raises(ValueError, match=r"\[\.\., 2\]"):
        rg.motion_to_velocity(np.zeros((4, 3)), geometry, 300.0)
    with pytest.raises(ValueError, match="the geometry has"):
        rg.motion_to_velocity(_grid(), skew, 100.0)
