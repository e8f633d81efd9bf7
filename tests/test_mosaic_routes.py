"""The single routes of the mosaic and section code: the point check against a rectangle and the section weighting check
(section.py), the public signatures of mosaic.py and section.py, and on the MI355X: both constructions of a MosaicSearch
set the same attributes, the row-stacking builder with one radar at the origin is ``compute_section_geometry``, and the
joint mean of the public calls -- launched through the combine entry points -- is the mean entry points' output bit for bit."""
import inspect

import numpy as np
import pytest

import radar_processor_amd as rg
from radar_processor_amd import mosaic, section

RECTANGLE = (-8000.0, 8000.0, -4000.0, 4000.0)          # of test_section_host's _NoDevice grid


# ---- host ---------------------------------------------------------------------------------------------------------------------
def test_the_point_check_against_a_rectangle_refuses_what_check_points_refuses():
    ok = np.float32([0.0, 100.0])
    cases = [                                           # the inputs of test_section_host.py, and its messages
        (np.float32([0.0, 8000.5]), ok, "point 1 .*outside the rectangle"),
        (np.float32([-8001.0, 0.0]), ok, "point 0 .*outside the rectangle"),
        (ok, np.float32([0.0, 4000.5]), "point 1 .*outside the rectangle"),
        (ok, np.float32([-4000.5, 0.0]), "point 0 .*outside the rectangle"),
        (np.float32([0.0, np.nan]), ok, "finite"),
        (ok, np.float32([np.inf, 0.0]), "finite"),
        (np.float32([-np.inf, 0.0]), ok, "finite"),
        (np.zeros(0, np.float32), np.zeros(0, np.float32), "n_points == 0"),
        (ok, np.float32([0.0]), "equal length"),
        (np.zeros((2, 2), np.float32), np.zeros((2, 2), np.float32), "one-dimensional"),
    ]

    class Search:                                       # what section_rectangle reads of a search
        full_shape, grid_limits, window = (3, 5, 9), ((0.0, 2000.0), (-4000.0, 4000.0), (-8000.0, 8000.0)), (0, 5, 0, 9)

    assert section.section_rectangle(Search) == RECTANGLE
    for xs, ys, what in cases:
        with pytest.raises(ValueError, match=what) as by_rectangle:
            section._check_points_in(RECTANGLE, xs, ys)
        with pytest.raises(ValueError, match=what) as by_search:
            section._check_points(Search, xs, ys, "barnes2")
        assert str(by_rectangle.value) == str(by_search.value)
    # the rim is inside; lists come back as contiguous float32
    xs, ys = section._check_points_in(RECTANGLE, [-8000.0, 8000.0], [-4000.0, 4000.0])
    assert xs.dtype == ys.dtype == np.float32 and xs.tolist() == [-8000.0, 8000.0] and ys.tolist() == [-4000.0, 4000.0]
    # a window's rectangle: the slices of the whole grid's float32 tables
    yc, xc = np.linspace(-4000.0, 4000.0, 5, dtype="float32"), np.linspace(-8000.0, 8000.0, 9, dtype="float32")
    assert section._grid_rectangle(Search.full_shape, Search.grid_limits, (1, 3, 2, 7)) == (
        float(xc[2]), float(xc[6]), float(yc[1]), float(yc[2]))
    assert section._grid_rectangle(Search.full_shape, Search.grid_limits) == RECTANGLE


@pytest.mark.parametrize("noun", ["a section", "a mosaic section"])
def test_the_section_weighting_check(noun):
    with pytest.raises(ValueError) as e:
        section._refuse_closest("closest", noun)
    assert str(e.value) == f"weighting 'closest' is a single-radar lattice mode; {noun} takes barnes2, cressman or nearest"
    with pytest.raises(ValueError) as e:
        section._refuse_closest("gauss", noun)
    assert str(e.value) == "Unknown weighting function: gauss"
    for weighting in ("barnes2", "cressman", "nearest"):
        section._refuse_closest(weighting, noun)
    with pytest.raises(ValueError, match="a section takes"):          # the default noun
        section._refuse_closest("closest")


SIGNATURES = {          # written down from the commit before the routes were merged
    ("mosaic", "MosaicSearch.__init__"): "(self, radars, grid_shape, grid_limits, min_radius: 'float' = 250.0, beam_factor: 'float' = 0.01746, toa: 'float' = 17000.0, device=None)",
    ("mosaic", "MosaicSearch.for_path"): "(radars, xs, ys, z_limits, nz, min_radius: 'float' = 250.0, beam_factor: 'float' = 0.01746, toa: 'float' = 17000.0, device=None) -> \"'MosaicSearch'\"",
    ("mosaic", "MosaicSearch.table"): "(self, radars: 'Sequence[int]', offsets: 'Sequence[int]')",
    ("mosaic", "MosaicSearch.section_table"): "(self, radars: 'Sequence[int]', offsets: 'Sequence[int]', points: 'Sequence')",
    ("mosaic", "apply_mosaic"): "(geometry: 'GridGeometry', fields: 'Sequence', additional_filters: 'Optional[Sequence]' = None, fill_value: 'float' = nan) -> 'np.ndarray'",
    ("mosaic", "apply_mosaic_multi"): "(geometry: 'GridGeometry', fields: 'Dict[str, Sequence]', additional_filters: 'Optional[Dict[str, Sequence]]' = None, fill_value: 'float' = nan) -> 'Dict[str, np.ndarray]'",
    ("mosaic", "compute_mosaic_geometry"): "(radars, grid_shape, grid_limits, temp_dir: 'str', min_radius: 'float' = 250.0, beam_factor: 'float' = 0.01746, weighting: 'str' = 'barnes2', toa: 'float' = 17000.0, n_workers: 'Optional[int]' = None) -> 'GridGeometry'",
    ("mosaic", "compute_mosaic_section_geometry"): "(radars, xs, ys, z_limits, nz, min_radius: 'float' = 250.0, beam_factor: 'float' = 0.01746, weighting: 'str' = 'barnes2', toa: 'float' = 17000.0) -> 'GridGeometry'",
    ("mosaic", "mosaic_fields_device"): "(target, fields: 'Sequence[Sequence]', masks: 'Optional[Sequence]' = None, shared_masks: 'Optional[Sequence]' = None, weighting: 'str' = 'barnes2', fill_value: 'float' = nan, products=None, radars: 'Optional[Sequence[int]]' = None, combine: 'str' = 'mean', return_radar: 'bool' = False)",
    ("mosaic", "mosaic_limits"): "(grid_limits, origin) -> 'Tuple[Tuple[float, float], ...]'",
    ("mosaic", "mosaic_section_fields_device"): "(search: 'MosaicSearch', xs, ys, fields: 'Sequence[Sequence]', masks: 'Optional[Sequence]' = None, shared_masks: 'Optional[Sequence]' = None, weighting: 'str' = 'barnes2', fill_value: 'float' = nan, radars: 'Optional[Sequence[int]]' = None, combine: 'str' = 'mean', return_radar: 'bool' = False)",
    ("mosaic", "mosaic_section_points"): "(search: 'MosaicSearch', xs, ys) -> 'List[Tuple[np.ndarray, np.ndarray]]'",
    ("mosaic", "mosaic_vertical_section"): "(radars, fields: 'Sequence', vertices, spacing, z_limits, nz, additional_filters=None, min_radius: 'float' = 250.0, beam_factor: 'float' = 0.01746, weighting: 'str' = 'barnes2', toa: 'float' = 17000.0, fill_value: 'float' = nan, combine: 'str' = 'mean')",
    ("mosaic", "path_reach"): "(gate_x, gate_y, gate_z, origin, rectangle, min_radius: 'float' = 250.0, beam_factor: 'float' = 0.01746, toa: 'float' = 17000.0) -> 'bool'",
    ("mosaic", "reach_window"): "(gate_x, gate_y, gate_z, grid_shape, grid_limits, origin, min_radius: 'float' = 250.0, beam_factor: 'float' = 0.01746, toa: 'float' = 17000.0) -> 'Tuple[int, int, int, int]'",
    ("section", "compute_section_geometry"): "(search: 'RoiSearch', xs, ys, weighting: 'str' = 'barnes2') -> 'GridGeometry'",
    ("section", "section_fields_device"): "(search: 'RoiSearch', xs, ys, fields: 'Sequence', masks: 'Optional[Sequence]' = None, shared_mask=None, weighting: 'str' = 'barnes2', fill_value: 'float' = nan, out=None)",
    ("section", "section_path"): "(vertices, spacing: 'float') -> 'Tuple[np.ndarray, np.ndarray, np.ndarray]'",
    ("section", "section_rectangle"): "(search) -> 'Tuple[float, float, float, float]'",
    ("section", "vertical_section"): "(gate_x, gate_y, gate_z, field_data, vertices, spacing, z_limits, nz, additional_filters=None, radar_altitude=0.0, min_radius=250.0, beam_factor=0.01746, weighting='barnes2', toa=17000.0, fill_value=nan)",
}


def test_public_signatures_are_those_of_the_parent():
    modules = {"mosaic": mosaic, "section": section}
    for (module, name), want in SIGNATURES.items():
        obj = modules[module]
        for part in name.split("."):
            obj = getattr(obj, part)
        assert str(inspect.signature(obj)) == want, f"{module}.{name}"
    # ... and nothing public has gone: every public function / class defined in the two modules is in the table
    for module, mod in modules.items():
        for name, obj in vars(mod).items():
            if not name.startswith("_") and getattr(obj, "__module__", None) == mod.__name__ and inspect.isfunction(obj):
                assert (module, name) in SIGNATURES, f"{module}.{name} is new"


# ---- GPU ----------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def dev():
    import torch
    rg.load_library()
    return torch.device("cuda", 0)


@pytest.mark.gpu
def test_both_constructions_of_a_mosaic_search_set_the_same_attributes(dev):
    import combine_scenes as cs
    scene = cs.tie_scene()
    kw = dict(min_radius=scene.min_radius, beam_factor=scene.beam_factor, toa=scene.toa)
    lattice = rg.MosaicSearch(scene.radars(), scene.shape, scene.limits, **kw)
    xs, ys = cs.path("tie")
    along = rg.MosaicSearch.for_path(scene.radars(), xs, ys, scene.limits[0], scene.shape[0], **kw)
    assert set(vars(lattice)) == set(vars(along)) and {"windows", "searches", "dev"} <= set(vars(along))
    for a in (lattice, along):
        assert a.n_radars == scene.n_radars == len(a.windows) == len(a.n_gates) and a.dev.type == "cuda"
        assert (a.min_radius, a.beam_factor, a.toa) == (scene.min_radius, scene.beam_factor, scene.toa)
    assert lattice.grid_shape == scene.shape and along.grid_shape == (scene.shape[0], 2, 2)


@pytest.mark.gpu
@pytest.mark.parametrize("weighting", ["barnes2", "cressman", "nearest"])
def test_one_radar_at_the_origin_through_the_stacker_is_the_section_geometry(dev, weighting):
    import section_scenes as sc
    vol = sc.volume()
    xs, ys, _ = sc.path_points("dogleg")
    xs, ys = xs[156:161], ys[156:161]                   # five points about the radar, where the rows are longest
    nz = 3
    kw = dict(min_radius=sc.MIN_RADIUS, beam_factor=sc.BEAM_FACTOR, toa=sc.TOA)
    limits = (sc.Z_LIMITS, (float(ys.min()), float(ys.max())), (float(xs.min()), float(xs.max())))
    search = rg.RoiSearch(vol.gate_x, vol.gate_y, vol.gate_z, (nz, 2, 2), limits, **kw)
    want = rg.compute_section_geometry(search, xs, ys, weighting)
    got = rg.compute_mosaic_section_geometry([(vol.gate_x, vol.gate_y, vol.gate_z, (0.0, 0.0, 0.0))], xs, ys, sc.Z_LIMITS, nz,
                                             weighting=weighting, **kw)
    assert want.n_pairs() > 0 and got.grid_shape == want.grid_shape == (nz, 1, 5)
    for name in ("indptr", "gate_indices", "weights"):
        a, b = np.asarray(getattr(got, name)), np.asarray(getattr(want, name))
        assert a.dtype == b.dtype and a.tobytes() == b.tobytes(), name
    assert got.gate_offsets.tolist() == [0, len(vol.gate_x)] and np.array_equal(got.origins, np.zeros((1, 3)))


@pytest.mark.gpu
@pytest.mark.parametrize("nf", [1, 3])
def test_the_public_mean_is_the_mean_entry_point(dev, nf):
    import torch
    import combine_scenes as cs
    from radar_processor_amd import _native
    from radar_processor_amd.roi_grid import pack_and_grid
    lib = _native.load_library()
    scene = cs.scene("scene16")
    search = rg.MosaicSearch(scene.radars(), scene.shape, scene.limits, min_radius=scene.min_radius,
                             beam_factor=scene.beam_factor, toa=scene.toa)
    sel = list(range(scene.n_radars))
    counts = [search.n_gates[r] for r in sel]
    offsets, n_total = mosaic._offsets(counts)[:-1], sum(counts)
    fs, shared = cs.field_set(scene, nf)

    def on_dev(a, dtype=torch.float32):
        return torch.from_numpy(np.ascontiguousarray(a)).to(dev, dtype=dtype)
    fields = [[on_dev(d) for d, _ in fs[r]] for r in sel]
    masks = [[on_dev(m.astype(np.uint8), torch.uint8) for _, m in fs[r]] for r in sel]
    shared_t = [on_dev(shared[r].astype(np.uint8), torch.uint8) for r in sel]
    cat = mosaic._concat_on_device(fields, masks, shared_t, counts, nf, torch, dev)
    nz, ny, nx = scene.shape
    xs, ys = cs.path("scene16")
    points = [None if np.isnan(p[0]).all() else (on_dev(p[0]), on_dev(p[1])) for p in rg.mosaic_section_points(search, xs, ys)]
    routes = [("rg_roi_grid_mosaic_f32", (search.table(sel, offsets), len(sel), nz, ny, nx), scene.shape,
               lambda: rg.mosaic_fields_device(search, fields, masks, shared_t, weighting="cressman", combine="mean")),
              ("rg_roi_section_mosaic_f32", (search.section_table(sel, offsets, points), len(sel), nz, len(xs)), (nz, len(xs)),
               lambda: rg.mosaic_section_fields_device(search, xs, ys, fields, masks, shared_t, weighting="cressman",
                                                       combine="mean"))]
    for entry, head, out_shape, public in routes:
        def launch(packed, nf_, stride, out_view, stream):
            _native.check(getattr(lib, entry)(*head, search.min_radius, search.beam_factor, _native.WEIGHTINGS["cressman"],
                                              _native.ptr(packed), nf_, stride, n_total, float("nan"), _native.ptr(out_view),
                                              stream), entry)
        want = pack_and_grid(dev, n_total, *cat, None, out_shape, launch).cpu().numpy()
        got = public().cpu().numpy()
        assert got.shape == want.shape == (nf,) + tuple(out_shape) and np.isfinite(want).sum() > 50 * nf, entry
        assert got.tobytes() == want.tobytes(), entry
