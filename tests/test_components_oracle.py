"""CPU-side checks of the connected-component feature (no GPU needed): the flood-fill restatement
(tests/components_oracle.py) against ``scipy.ndimage.label`` and hand-written answers, the scenes, every refusal of the Python
surface before any device work, and the ABI bookkeeping."""
import ctypes
import os
import re

import numpy as np
import pytest

import component_scenes as cs
import components_oracle as co
import radar_processor_amd as rg
from conftest import REPO
from radar_processor_amd import _native, components

STRUCTURES = {4: [[0, 1, 0], [1, 1, 1], [0, 1, 0]], 8: [[1, 1, 1], [1, 1, 1], [1, 1, 1]]}


# ---- the restatement -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("connectivity", (4, 8))
@pytest.mark.parametrize("shape", cs.SHAPES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_oracle_numbers_cells_like_scipy(shape, connectivity):
    ndimage = pytest.importorskip("scipy.ndimage")
    for name in cs.NON_WRAPPING:
        s = cs.scene(shape, name)
        labels, cell_ptr = co.label(s.planes, s.lo, s.hi, s.mask, connectivity)
        fg = co.foreground(s.planes, s.lo, s.hi, s.mask)
        for p in range(s.planes.shape[0]):
            want, count = ndimage.label(fg[p], structure=STRUCTURES[connectivity])
            assert cell_ptr[p + 1] - cell_ptr[p] == count, (name, p)
            np.testing.assert_array_equal(labels[p], want, err_msg=name)


@pytest.mark.parametrize("connectivity", (4, 8))
@pytest.mark.parametrize("shape", cs.SHAPES[3:], ids=lambda s: f"{s[0]}x{s[1]}")
def test_wrap_is_invariant_under_rolling_the_rows(shape, connectivity):
    """Rolling a plane by k rows moves every pixel but, with wrap_rows, not the partition into cells."""
    h, w = shape
    for name in cs.WRAPPING:
        s = cs.scene(shape, name)
        fg = co.foreground(s.planes, s.lo, s.hi, s.mask)
        for p in range(fg.shape[0]):
            base = co.partition(co.label_plane(fg[p], connectivity, True)[0])
            for k in (1, h // 2, h - 1):
                rolled = co.label_plane(np.roll(fg[p], k, axis=0), connectivity, True)[0]
                back = {frozenset(((i // w - k) % h) * w + i % w for i in cell) for cell in co.partition(rolled)}
                assert back == base, (name, p, k)


def test_scenes_are_what_the_module_says():
    th, tw = cs.TH, cs.TW
    assert cs.SHAPES == ((1, 1), (1, 2 * tw + 3), (2 * th + 3, 1), (th, tw), (th + 1, tw + 1), (2 * th + 5, 3 * tw + 7))
    assert max(h * w for h, w in cs.SHAPES) < 200 * 300
    big = cs.SHAPES[-1]
    count = lambda name, c, wrap=False: int(co.label(*cs.scene(big, name)[1:5], connectivity=c, wrap_rows=wrap)[1][-1])
    n_fg = lambda name: int(co.foreground(*cs.scene(big, name)[1:5]).sum())
    assert count("all_nan", 8) == 0 and count("all_foreground", 4) == 1
    assert count("checkerboard", 8) == 1 and count("checkerboard", 4) == n_fg("checkerboard") == (big[0] * big[1] + 1) // 2
    assert count("diagonals", 4) == n_fg("diagonals") and count("diagonals", 8) < n_fg("diagonals") // 8
    assert count("serpentine", 4) == count("spiral", 4) == count("comb", 4) == 1
    assert n_fg("spiral") > big[0] * big[1] // 3
    # the wrap scenes hold cells that only the wrap joins
    for name in ("wrap_blob", "wrap_antidiagonals", "wrap_random_0.45"):
        assert count(name, 8, True) < count(name, 8, False), name
    assert count("wrap_blob", 8, True) == 4 and count("wrap_blob", 4, True) == 5 and count("wrap_blob", 8, False) == 6
    # three planes: the middle one empty, foreground on both sides of each plane border
    three = cs.scene(big, "three_planes")
    fg = co.foreground(three.planes, three.lo)
    assert fg[0, -1, -1] and not fg[1].any() and fg[2, 0, 0]
    ptr = co.label(three.planes, three.lo)[1]
    assert ptr[1] == ptr[2] and ptr[3] > ptr[2] > 0
    # the lattice holds pixels exactly at both bounds, and every special value
    lat = cs.scene(big, "lattice")
    for v in (20.0, 30.0, np.inf, -np.inf):
        assert (lat.planes == v).any()
    assert np.isnan(lat.planes).any() and (np.signbit(lat.planes) & (lat.planes == 0)).any() and lat.mask.any()


def test_known_answers():
    nan = np.nan
    plane = np.array([[[5, 0, 5, 5],
                       [0, 5, 0, nan],
                       [5, 0, 0, 7],
                       [5, 0, 9, 7]]], np.float32)
    labels8, ptr8 = co.label(plane, 5.0)
    assert labels8[0].tolist() == [[1, 0, 1, 1], [0, 1, 0, 0], [1, 0, 0, 2], [1, 0, 2, 2]] and ptr8.tolist() == [0, 2]
    labels4, ptr4 = co.label(plane, 5.0, connectivity=4)
    assert labels4[0].tolist() == [[1, 0, 2, 2], [0, 3, 0, 0], [4, 0, 0, 5], [4, 0, 5, 5]] and ptr4.tolist() == [0, 5]
    # lo is inclusive, hi too; NaN is never foreground; the mask excludes
    assert co.label(plane, 5.0, hi=7.0)[0][0].tolist() == [[1, 0, 1, 1], [0, 1, 0, 0], [1, 0, 0, 2], [1, 0, 0, 2]]
    mask = np.zeros(plane.shape, np.uint8)
    mask[0, 1, 1] = 3
    assert co.label(plane, 5.0, mask=mask)[1].tolist() == [0, 4]
    # wrap: rows 0 and 3 are neighbours, so with 4-connectivity the cell of (0, 0) and that of (2, 0), (3, 0) are one
    assert co.label(plane, 5.0, connectivity=4, wrap_rows=True)[0][0].tolist() == \
        [[1, 0, 2, 2], [0, 3, 0, 0], [1, 0, 0, 2], [1, 0, 2, 2]]
    t = co.stats(plane, labels8, ptr8)
    assert t["area"].tolist() == [6, 3] and t["bbox"].tolist() == [[0, 3, 0, 3], [2, 3, 2, 3]]
    assert t["sum_yx"].tolist() == [[6, 6], [8, 8]] and t["vmax"].tolist() == [5.0, 9.0]
    assert t["argmax"].tolist() == [0, 14] and t["vsum"].tolist() == [30.0, 23.0]          # ties: the smallest index
    assert t["plane"].tolist() == [0, 0] and t["id"].tolist() == [1, 2]
    # -0 sorts below +0
    z = np.array([[[-0.0, 0.0, -0.0]]], np.float32)
    tz = co.stats(z, *co.label(z, -1.0))
    assert tz["argmax"].tolist() == [1] and not np.signbit(tz["vmax"][0])
    # despeckle: min_size 4 removes the cell of three pixels, bit for bit elsewhere
    out, removed = co.despeckle(plane, 5.0, 4, fill=-1.0)
    assert removed[0].tolist() == [[0, 0, 0, 0], [0, 0, 0, 0], [0, 0, 0, 1], [0, 0, 1, 1]]
    assert out[0, 2:, 2:].tolist() == [[0.0, -1.0], [-1.0, -1.0]]
    keep = removed == 0
    assert (out.view(np.uint32)[keep] == plane.view(np.uint32)[keep]).all()
    assert co.despeckle(plane, 5.0, 1)[1].sum() == 0 and co.despeckle(plane, 5.0, 7)[1].sum() == 9
    # centroids on a 4 x 4 grid of 1 km nodes from -1500 m
    c = co.centroids(t, (1, 4, 4), ((0.0, 0.0), (-1500.0, 1500.0), (-1500.0, 1500.0)))
    assert c["centroid_y"].tolist() == [-500.0, -1500.0 + 8.0 / 3.0 * 1000.0] and c["peak_x"].tolist() == [-1500.0, 500.0]
    assert c["area_km2"].tolist() == [6.0, 3.0]


# ---- refusals: all before any device call ----------------------------------------------------------------------------------
def test_every_refusal_raises_without_a_device(monkeypatch):
    def no_device(*a, **k):
        raise AssertionError("the device was touched")
    for name in ("load_library", "canonical_device", "device", "torch_mod"):
        monkeypatch.setattr(_native, name, no_device)
    plane = np.zeros((5, 7), np.float32)
    for fn, args in ((rg.label_components_device, (plane, 35.0)), (rg.despeckle_device, (plane, 35.0, 3)),
                     (rg.despeckle, (plane, 35.0, 3))):
        for bad in (6, 0, "8", True, None):
            with pytest.raises(ValueError, match=f"connectivity must be 4 or 8, not {bad!r}"):
                fn(*args, connectivity=bad)
        with pytest.raises(ValueError, match="upper 30.0 lies below threshold 35.0"):
            fn(*args, upper=30.0)
        with pytest.raises(ValueError, match=r"mask of shape \[7, 5\]"):
            fn(*args, mask=np.zeros((7, 5), np.uint8))
        with pytest.raises(ValueError, match=r"mask of shape \[1, 5, 7\]"):
            fn(*args, mask=np.zeros((1, 5, 7), np.uint8))
        for bad_planes in (plane.astype(np.float64), plane.astype(np.int32), plane.ravel(), plane[None, None]):
            with pytest.raises(ValueError, match="planes must be float32"):
                fn(bad_planes, *args[1:])
    for bad in (0, -1, 2.5, True, 2 ** 31):
        with pytest.raises(ValueError, match="min_size must be an integer of at least 1"):
            rg.despeckle_device(plane, 35.0, bad)
        with pytest.raises(ValueError, match="min_size must be an integer of at least 1"):
            rg.identify_cells(plane, None, 35.0, min_size=bad)
    with pytest.raises(ValueError, match="NaN"):
        rg.label_components_device(plane, np.nan)
    with pytest.raises(ValueError, match="connectivity must be 4 or 8, not 5"):
        rg.identify_cells(plane, None, 35.0, connectivity=5)
    with pytest.raises(ValueError, match="plane must be float32"):
        rg.identify_cells(plane[None], None, 35.0)
    with pytest.raises(ValueError, match="labels of shape"):
        rg.cell_table_device(plane, np.zeros((7, 5), np.int32), np.zeros(2, np.int32))

    class Geometry:
        grid_shape, grid_limits = (3, 5, 8), ((0.0, 1.0), (0.0, 1.0), (0.0, 1.0))
    with pytest.raises(ValueError, match=r"geometry of planes \[5, 8\]"):
        rg.cell_table_device(plane, np.zeros((5, 7), np.int32), np.zeros(2, np.int32), Geometry())


# ---- bookkeeping -----------------------------------------------------------------------------------------------------------
FUNCTIONS = ("rg_label_components_f32", "rg_component_stats_f32", "rg_despeckle_select_f32")
HEADER = os.path.join(REPO, "include", "radargrid_hip.h")


def _kind(arg):
    arg = " ".join(arg.split())
    return (ctypes.c_void_p if ("*" in arg or arg.startswith("rg_stream_t")) else ctypes.c_float if arg.startswith("float ") else
            ctypes.c_int64 if arg.startswith("int64_t ") else ctypes.c_int32)


def test_header_declares_the_functions_with_the_stated_arguments():
    header = open(HEADER).read()
    declared = set(re.findall(r"^(?:int|int64_t|const char\*)\s+(rg_\w+)\s*\(", header, flags=re.M))
    assert "#define RG_VERSION 104" in header and _native.ABI_VERSION == 104
    assert f"#define RG_CC_TILE_H {_native.RG_CC_TILE_H}\n" in header and f"#define RG_CC_TILE_W {_native.RG_CC_TILE_W}\n" in header
    stated = {
        "rg_label_components_f32": "src mask n_planes h w lo hi connectivity wrap_rows labels cell_ptr workspace "
                                   "workspace_bytes stream",
        "rg_component_stats_f32": "src labels cell_ptr n_planes h w n_cells area bbox sum_yx vmax argmax vsum stream",
        "rg_despeckle_select_f32": "src labels cell_ptr area n_planes h w min_size fill out out_mask stream",
    }
    for name in FUNCTIONS + ("rg_components_workspace_bytes",):
        assert name in declared and name in _native.SIGNATURES
    for name in FUNCTIONS:
        args = re.search(r"^int %s\((.*?)\);" % name, header, flags=re.S | re.M).group(1).split(",")
        assert [re.sub(r"\W", "", a.split()[-1]) for a in args] == stated[name].split(), name
        restype, argtypes = _native.SIGNATURES[name]
        assert restype is ctypes.c_int32 and [_kind(a) for a in args] == argtypes, name
    assert _native.SIGNATURES["rg_components_workspace_bytes"] == (ctypes.c_int64, [ctypes.c_int32] * 3)
    from radar_processor_amd import build
    assert ("rg_components.hip", []) in build.SOURCES


def test_library_exports_the_functions():
    lib = rg.load_library(require_device=False)
    assert lib.rg_version() == 104
    for name in FUNCTIONS + ("rg_components_workspace_bytes",):
        assert getattr(lib, name).argtypes == _native.SIGNATURES[name][1]
    # sizes are checked on the host: a workspace for n pixels and their chunks of 1024; 2^31 pixels are refused
    assert lib.rg_components_workspace_bytes(1, 1, 1) == 16
    assert lib.rg_components_workspace_bytes(3, 100, 100) == (3 * 10000 + 3 * 10) * 4 + 8
    assert lib.rg_components_workspace_bytes(2, 32768, 32768) == _native.RG_EINVAL
    assert lib.rg_components_workspace_bytes(1, 46341, 46341) == _native.RG_EINVAL
    assert lib.rg_components_workspace_bytes(0, 4, 4) == _native.RG_EINVAL
    assert lib.rg_components_workspace_bytes(1, 46340, 46340) > 4 * 46340 * 46340


def test_names_are_importable_from_the_package():
    for name in ("label_components_device", "cell_table_device", "despeckle_device", "despeckle", "identify_cells",
                 "CellTable"):
        assert name in rg.__all__ and getattr(rg, name) is getattr(components, name)
    assert rg.CellTable._fields[:8] == ("plane", "id", "area", "bbox", "sum_yx", "vmax", "argmax", "vsum")
    assert rg.CellTable._fields[8:] == ("centroid_x", "centroid_y", "peak_x", "peak_y", "area_km2")
