"""The NumPy restatement of the rain rate (tests/accumulation_oracle.py) against its classes and a float64 ``pow``; the ABI
bookkeeping of the two new entry points; and the host side of ``radar_processor_amd/accumulation.py`` with no device present:
every ``ValueError`` is raised before the library is loaded (the loader is monkeypatched to raise)."""
import ctypes
import os
import re

import numpy as np
import pytest

import accumulation_oracle as ao
import radar_processor_amd as rg
from radar_processor_amd import _native, accumulation, build, motion

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FUNCTIONS = ("rg_rain_rate_f32", "rg_accumulate_advected_f32")


# ---- the rate ----------------------------------------------------------------------------------------------------------------
def test_rate_classes_of_the_restatement():
    src = np.array([np.nan, 30.0, 30.0, 4.999, 5.0, -np.inf, -40.0, 55.0, 60.0, np.inf, 54.999], dtype=np.float32)
    mask = np.array([0, 0, 9, 0, 0, 0, 0, 0, 0, 0, 0], dtype=np.uint8)
    got = ao.rain_rate(src, mask=mask)
    assert got.dtype == np.float32
    assert got.view(np.uint32)[0] == ao.NAN_BITS and got.view(np.uint32)[2] == ao.NAN_BITS        # NaN, mask: no coverage
    assert got[3] == 0.0 and got[5] == 0.0 and got[6] == 0.0 and not np.signbit(got[[3, 5, 6]]).any()     # below min_dbz, -inf
    assert got[4] > 0.0                                                                           # min_dbz itself is wet
    cap = got[7]
    assert got[8] == cap and got[9] == cap and got[10] < cap and np.isfinite(cap)                 # the cap, +inf included
    assert ao.rain_rate(src)[2] == got[1]                                                         # without the mask
    both = ao.rain_rate(np.stack([src, src]).reshape(2, 1, -1))                                   # any shape
    assert both.shape == (2, 1, src.size) and np.array_equal(both[1, 0], ao.rain_rate(src), equal_nan=True)
    # another relation, other limits
    wide = ao.rain_rate(src, a=300.0, b=1.4, min_dbz=-50.0, max_dbz=70.0)
    assert wide[6] > 0.0 and wide[8] > wide[7] and wide[9] == ao.rain_rate(np.float32([70.0]), 300.0, 1.4, -50.0, 70.0)[0]


def test_marshall_palmer_spot_values_against_a_float64_pow():
    for a, b in ((200.0, 1.6), (300.0, 1.4), (250.0, 1.2)):
        p, q = ao.zr_constants(a, b)
        for dbz in (5.0, 10.0, 23.0, 30.0, 40.0, 47.5, 55.0):
            want = (10.0 ** (dbz / 10.0) / a) ** (1.0 / b)
            assert abs(np.exp(dbz * p - q) - want) <= 1e-12 * want, (a, b, dbz)
            got = ao.rain_rate(np.float32([dbz]), a, b, 0.0, 60.0)[0]
            assert got in (np.float32(want), np.nextafter(np.float32(want), np.float32(0)), np.nextafter(np.float32(want), np.float32(1e9)))
    # the values every textbook lists for Z = 200 R^1.6
    for dbz, rate in ((23.0, 1.0), (39.0, 10.0), (55.0, 100.0)):
        assert abs(ao.rain_rate(np.float32([dbz]))[0] - rate) < 0.01 * rate


# ---- ABI bookkeeping ---------------------------------------------------------------------------------------------------------
def test_abi_bookkeeping_and_exports():
    header = open(os.path.join(REPO, "include", "radargrid_hip.h")).read()
    declared = set(re.findall(r"^(?:int|int64_t|const char\*)\s+(rg_\w+)\s*\(", header, flags=re.M))
    assert "#define RG_VERSION 104" in header and _native.ABI_VERSION == 104
    assert "#define RG_MAX_ACC_STEPS 64" in header and _native.RG_MAX_ACC_STEPS == 64 == accumulation.MAX_STEPS == ao.MAX_ACC_STEPS
    assert "Rain rate and accumulation" in header
    assert ("rg_accumulate.hip", []) in build.SOURCES
    lib = rg.load_library(require_device=False)
    for name in FUNCTIONS:
        assert name in declared and getattr(lib, name).argtypes == _native.SIGNATURES[name][1]
        args = re.search(r"^int %s\((.*?)\);" % name, header, flags=re.S | re.M).group(1).split(",")
        want = []
        for a in args:
            a = " ".join(a.split())
            want.append(_native.MotionLattice if a.startswith("rg_motion_lattice") else
                        ctypes.c_void_p if ("*" in a or a.startswith("rg_stream_t")) else
                        ctypes.c_double if a.startswith("double ") else
                        ctypes.c_float if a.startswith("float ") else ctypes.c_int32)
        assert want == _native.SIGNATURES[name][1], name
    for name in ("rain_rate_device", "accumulate_device", "accumulate", "RainAccumulator", "AccumulationFrame"):
        assert name in rg.__all__ and getattr(rg, name) is getattr(accumulation, name)
    # the advection and the accumulation call ONE copy of the displacement
    csrc = os.path.join(REPO, "radar_processor_amd", "csrc")
    for unit in ("rg_motion.hip", "rg_accumulate.hip"):
        text = open(os.path.join(csrc, unit)).read()
        assert '#include "rg_motion_field.hpp"' in text and "rg::displacement(" in text and "clamp_node(double" not in text


# ---- host validation ---------------------------------------------------------------------------------------------------------
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
FIELD = np.zeros((4, 5, 2), dtype=np.float32)
LAT = (7.5, 7.5, 8.0, 8.0, 4, 5)


def _grid(shape=(40, 48)):
    m = np.zeros((4, 5, 2), dtype=np.float32)
    return motion.MotionGrid(m, np.ones(m.shape[:-1], dtype=np.float32), np.zeros(m.shape, dtype=np.int16), 16, 8, 6, shape, 7.5, 8.0)


def test_valid_arguments_reach_the_loader(no_device):
    """The fixture works: with nothing to refuse, each function gets as far as loading the library."""
    for call in (lambda: rg.rain_rate_device(PLANE), lambda: rg.rain_rate_device(STACK, a=300.0, b=1.4, mask=STACK != 0),
                 lambda: rg.accumulate_device(PLANE, PLANE, None, 0.1, steps=1),
                 lambda: rg.accumulate_device(STACK, STACK, FIELD, 0.1, steps=64, lattice=LAT, method="nearest", substeps=16, min_steps=1),
                 lambda: rg.accumulate_device(PLANE, PLANE, _grid(), 0.1, steps=8, return_steps=True),
                 lambda: rg.accumulate(PLANE, PLANE, None, 0.1, steps=2),
                 lambda: rg.RainAccumulator().update(PLANE, 0.0),
                 lambda: rg.RainAccumulator(motion=None, steps=4).update(PLANE, 10.0, mask=PLANE != 0)):
        with pytest.raises(DeviceTouched):
            call()


def test_rain_rate_refusals(no_device):
    r = rg.rain_rate_device
    for bad in (PLANE.astype(np.float64), PLANE[0], np.zeros((0, 4, 4), dtype=np.float32), [[1.0]]):
        with pytest.raises(ValueError, match="planes"):
            r(bad)
    for kw in (dict(a=0.0), dict(a=-200.0), dict(a=np.nan), dict(a=np.inf), dict(b=0.0), dict(b=-1.6), dict(b=np.nan), dict(b=np.inf),
               dict(a="x")):
        with pytest.raises(ValueError, match="a"):
            r(PLANE, **kw)
    for kw in (dict(min_dbz=np.nan), dict(max_dbz=np.inf), dict(min_dbz=-np.inf), dict(min_dbz=60.0), dict(min_dbz=10.0, max_dbz=9.0)):
        with pytest.raises(ValueError, match="min_dbz and max_dbz"):
            r(PLANE, **kw)
    with pytest.raises(ValueError, match="no finite rate"):
        r(PLANE, a=1e300, b=1e-308)
    with pytest.raises(ValueError, match="mask of shape"):
        r(PLANE, mask=np.zeros((40, 47), dtype=np.uint8))


def test_accumulate_refusals(no_device):
    for acc in (rg.accumulate_device, rg.accumulate):
        with pytest.raises(ValueError, match="rate_prev must be"):
            acc(PLANE.astype(np.float64), PLANE, None, 0.1, steps=1)
        with pytest.raises(ValueError, match="rate_next must be"):
            acc(PLANE, PLANE.astype(np.float64), None, 0.1, steps=1)
        for other in (PLANE[:, :-1], STACK, PLANE[None]):
            with pytest.raises(ValueError, match="differ"):
                acc(PLANE, other, None, 0.1, steps=1)
        with pytest.raises(ValueError, match="zero motion"):
            acc(PLANE, PLANE, None, 0.1, steps=1, lattice=LAT)
        with pytest.raises(ValueError, match="needs a lattice"):
            acc(PLANE, PLANE, FIELD, 0.1, steps=1)
        with pytest.raises(ValueError, match="NaN or inf"):
            acc(PLANE, PLANE, np.full((4, 5, 2), np.nan, dtype=np.float32), 0.1, steps=1, lattice=LAT)
        with pytest.raises(ValueError, match="estimated on planes"):
            acc(PLANE, PLANE, _grid((40, 50)), 0.1, steps=1)
        for hours in (0.0, -1.0, np.nan, np.inf, "soon", None):
            with pytest.raises(ValueError, match="hours"):
                acc(PLANE, PLANE, None, hours, steps=1)
        for steps in (0, 65, -1, 2.0, True, None):
            with pytest.raises(ValueError, match="steps must be"):
                acc(PLANE, PLANE, None, 0.1, steps=steps)
        for substeps in (0, 17, 1.0):
            with pytest.raises(ValueError, match="substeps"):
                acc(PLANE, PLANE, None, 0.1, steps=4, substeps=substeps)
        for min_steps in (0, 5, -1, 2.0):
            with pytest.raises(ValueError, match="min_steps"):
                acc(PLANE, PLANE, None, 0.1, steps=4, min_steps=min_steps)
        with pytest.raises(ValueError, match="method"):
            acc(PLANE, PLANE, None, 0.1, steps=4, method="cubic")
        with pytest.raises(ValueError, match="out must be a tensor"):
            acc(PLANE, PLANE, None, 0.1, steps=4, out=np.zeros((40, 48), dtype=np.float32))
    with pytest.raises(TypeError):
        rg.accumulate_device(PLANE, PLANE, None, 0.1)                   # steps has no default


def test_accumulator_refusals(no_device):
    R = rg.RainAccumulator
    for kw in (dict(a=0.0), dict(b=np.nan), dict(min_dbz=9.0, max_dbz=8.0), dict(motion="fast"), dict(motion=3), dict(steps=0), dict(steps=65),
               dict(method="cubic"), dict(window_seconds=0.0), dict(window_seconds=np.inf), dict(max_gap_seconds=0.0),
               dict(min_score=np.nan), dict(block=18), dict(search=40), dict(lo=5.0, hi=5.0), dict(leads=3), dict(mask_prev=PLANE),
               dict(motion=None, block=16), dict(motion=_grid()), dict(motion=(FIELD, LAT)), dict(motion=(FIELD,), steps=3)):
        with pytest.raises(ValueError):
            R(**kw)
    assert R().steps == 16 and R(search=6).steps == 6 and R(search=0).steps == 1 and R(motion=None).steps == 1
    assert R(steps=9).steps == 9 and R(motion=_grid(), steps=5).steps == 5 and R(motion=(FIELD, LAT), steps=5).steps == 5
    acc = R(motion=None)
    assert acc.total() is None and acc.intervals == []
    for plane in (PLANE.astype(np.float64), STACK, PLANE[0]):
        with pytest.raises(ValueError, match="plane_dbz"):
            acc.update(plane, 0.0)
    for t in (np.nan, np.inf, "now", None):
        with pytest.raises(ValueError, match="time_seconds"):
            acc.update(PLANE, t)
    with pytest.raises(ValueError, match="mask of shape"):
        acc.update(PLANE, 0.0, mask=np.zeros((40, 47), dtype=np.uint8))
    with pytest.raises(ValueError, match="window_seconds"):
        acc.total(window_seconds=0.0)
    # a time that does not increase, a plane of another shape: refused against the scan held, before the device
    acc._last = (100.0, PLANE, None, PLANE)
    for t in (100.0, 99.0, -5.0):
        with pytest.raises(ValueError, match="must increase"):
            acc.update(PLANE, t)
    with pytest.raises(ValueError, match="after planes of"):
        acc.update(PLANE[:, :-1], 200.0)
