"""The closest-gate mode of ``rg_roi_grid_f32`` (``RG_W_CLOSEST``, csrc/rg_roi_grid.hip) -- the mode the processor seam calls --
against ``oracle.closest_gate_choice`` on EVERY voxel of every field: the oracle predicts the kernel's choice exactly
(float64 membership, then the minimum of (the kernel's float32 d2, gate index)), ties included, so nothing is skipped and
nothing is compared to a tolerance.  Field values are index-coded (tests/closest_scenes.py), so a gridded value names the
chosen gate; a second set of runs carries real values and checks that their bits arrive unchanged.

Scenes: polar volumes with natural ties, dense clouds on ragged grids (the survivor ring wraps), planted ties, planted rim
gates.  Field counts 1, 2, 3, 4, 5, 8 and 11 (every value-ring / gather variant of the kernel and two groups), a different mask
per field, a shared mask, per-level lists or one list, tiny cells, finite fill values and preallocated outputs.  What the
scenes are required to contain is asserted on the CPU by tests/test_closest_oracle.py."""
from types import SimpleNamespace

import numpy as np
import pytest

import closest_scenes as cs

pytestmark = pytest.mark.gpu

# forced cell sizes: more than 64 cell rows in the search box of every full voxel block (asserted in _search)
SMALL_CELL = dict(polar_const=60.0, polar_beam=40.0, ragged_a=50.0, ragged_b=50.0, ties=40.0, rim=100.0)
_SEARCHES = {}


@pytest.fixture(scope="module")
def rg():
    import radar_processor_amd as pkg
    pkg.load_library()
    return pkg


def _search(rg, s, **variant):
    """The scene's RoiSearch for a variant (``per_level``, ``cell_size``), built once per process."""
    key = (s.name, tuple(sorted(variant.items())))
    if key not in _SEARCHES:
        import torch
        search = rg.RoiSearch(s.gx, s.gy, s.gz, s.shape, s.limits, device=torch.device("cuda", 0), **s.search_kw(), **variant)
        if variant.get("per_level") is not None:
            assert search.per_level == variant["per_level"]
        if variant.get("cell_size") is not None:
            assert search.cell_size == variant["cell_size"]
            dy = (s.limits[1][1] - s.limits[1][0]) / (s.shape[1] - 1)
            assert (3 * dy + 2 * s.min_radius) / search.cell_size > 64
        _SEARCHES[key] = search
    return _SEARCHES[key]


def _coded_fields(s, n):
    """Field k carries ``g + k * n_gates`` on gate g: the gate can be read back, and so can the field it came from."""
    assert (n + 1) * s.n_gates < 2 ** 24
    return [(np.arange(s.n_gates, dtype=np.int64) + k * s.n_gates).astype(np.float32) for k in range(n)]


def _grid(rg, search, fields, masks, shared=None, fill=np.nan, prefill=None):
    import torch
    dev = search.dev
    f_t = [torch.from_numpy(np.ascontiguousarray(f)).to(dev) for f in fields]
    m_t = [None if m is None else torch.from_numpy(m.astype(np.uint8)).to(dev) for m in masks]
    s_t = None if shared is None else torch.from_numpy(shared.astype(np.uint8)).to(dev)
    out = None
    if prefill is not None:
        out = torch.full((len(fields),) + tuple(search.grid_shape), float(prefill), dtype=torch.float32, device=dev)
    got = rg.roi_grid_fields_device(search, f_t, m_t, shared_mask=s_t, weighting="closest", fill_value=fill, out=out)
    if out is not None:
        assert got.data_ptr() == out.data_ptr()
    return got.cpu().numpy()


def _assert_choice(got, want_idx, n_gates, fill, label):
    """Every voxel of every field: the fill value exactly where the oracle has no gate, the oracle's gate everywhere else."""
    n = got.shape[0]
    want_idx = want_idx[:n]
    empty = np.isnan(got) if np.isnan(fill) else got == np.float32(fill)
    with np.errstate(invalid="ignore"):
        code = np.where(empty, -1.0, got.astype(np.float64))
    assert np.array_equal(code, np.floor(code)), f"{label}: a gridded value is not an index code"
    base = (np.arange(n, dtype=np.int64) * n_gates).reshape((n,) + (1,) * (got.ndim - 1))
    gate = np.where(empty, -1, code.astype(np.int64) - base)
    bad = np.argwhere(gate != want_idx)
    assert bad.shape[0] == 0, (
        f"{label}: {bad.shape[0]} of {gate.size} voxels differ from the oracle "
        f"({int(((gate < 0) != (want_idx < 0)).sum())} of them filled on one side only); first (field, iz, iy, ix) got / want: "
        + ", ".join(f"{tuple(int(t) for t in b)} {int(gate[tuple(b)])} / {int(want_idx[tuple(b)])}" for b in bad[:6]))


# ---- 1. every scene, every field count ---------------------------------------------------------------------------------
@pytest.mark.parametrize("n_fields", cs.FIELD_COUNTS)
@pytest.mark.parametrize("name", cs.SCENES)
def test_chosen_gate_on_every_voxel(rg, name, n_fields):
    s = cs.scene(name)
    got = _grid(rg, _search(rg, s), _coded_fields(s, n_fields), s.masks(n_fields))
    assert got.shape == (n_fields,) + tuple(s.shape)
    _assert_choice(got, s.choice()["idx32"], s.n_gates, np.nan, f"{name}, {n_fields} fields")


@pytest.mark.parametrize("name", cs.SCENES)
def test_shared_mask(rg, name):
    s = cs.scene(name)
    got = _grid(rg, _search(rg, s), _coded_fields(s, 3), s.masks(3), shared=s.shared_mask())
    _assert_choice(got, s.choice_shared(3)["idx32"], s.n_gates, np.nan, f"{name}, shared mask")


# ---- 2. search variants, fill values, preallocated outputs -----------------------------------------------------------------
VARIANTS = {
    "per_level": (dict(per_level=True), np.nan, None),
    "one_list": (dict(per_level=False), -5.0, 123.0),
    "small_cells": (dict(cell_size=True), -1.0, np.nan),
    "small_cells_one_list": (dict(cell_size=True, per_level=False), 3.0e38, -2.0),
}


@pytest.mark.parametrize("variant", sorted(VARIANTS))
@pytest.mark.parametrize("name", cs.SCENES)
def test_search_variants_fill_value_and_preallocated_out(rg, name, variant):
    """Per-level gate lists or one list, cells small enough for more than 64 cell rows per search box (the chunked row
    loop), a finite fill value (negative: never an index code) and an ``out`` tensor that held another number."""
    s = cs.scene(name)
    kw, fill, prefill = VARIANTS[variant]
    kw = dict(kw)
    if kw.get("cell_size"):
        kw["cell_size"] = SMALL_CELL[name]
    if kw.get("per_level") and s.shape[0] == 1:
        kw.pop("per_level")                        # one level: there is one list either way
    search = _search(rg, s, **kw)
    if fill > 0:                                   # a positive fill must not be an index code
        assert fill > 2 ** 24
    for n_fields in (1, 2, 5):
        got = _grid(rg, search, _coded_fields(s, n_fields), s.masks(n_fields), fill=fill, prefill=prefill)
        _assert_choice(got, s.choice()["idx32"], s.n_gates, fill, f"{name}, {variant}, {n_fields} fields")


# ---- 3. the bits of the chosen value ------------------------------------------------------------------------------------
@pytest.mark.parametrize("n_fields", [1, 2, 4, 8])
@pytest.mark.parametrize("name", cs.SCENES)
def test_value_bits_are_transported(rg, name, n_fields):
    """Real data with -0.0, a subnormal, +inf, -inf and an unmasked NaN on gates that win somewhere: the output holds the
    bits of ``values[idx32]`` (for NaN: a NaN), the fill value where there is no gate."""
    s = cs.scene(name)
    val, special = s.real_values()
    fields = [(val * np.float32(1 + k)).astype(np.float32) for k in range(n_fields)]
    fill = np.float32(-999.0)
    got = _grid(rg, _search(rg, s), fields, s.masks(n_fields), fill=float(fill))
    idx = s.choice()["idx32"][:n_fields]
    for k in range(n_fields):
        want = np.where(idx[k] >= 0, fields[k][np.maximum(idx[k], 0)], fill).astype(np.float32)
        nan = np.isnan(want)
        np.testing.assert_array_equal(np.isnan(got[k]), nan, err_msg=f"{name} field {k}")
        diff = (got[k].view(np.uint32) != want.view(np.uint32)) & ~nan
        assert not diff.any(), f"{name} field {k}: {int(diff.sum())} voxels with other bits than values[idx32]"
    if n_fields >= 2:                              # field 1 excludes nothing: every special value is in the grid
        bits = set(got[1].view(np.uint32).ravel().tolist())
        for key in ("neg_zero", "subnormal", "pos_inf", "neg_inf"):
            assert int(fields[1][special[key]:special[key] + 1].view(np.uint32)[0]) in bits, key
        assert np.isnan(got[1]).any()


@pytest.mark.parametrize("name", ["polar_const", "ragged_a", "ties"])
def test_two_runs_give_the_same_bits(rg, name):
    s = cs.scene(name)
    for n_fields in (1, 3, 8):
        a = _grid(rg, _search(rg, s), _coded_fields(s, n_fields), s.masks(n_fields))
        b = _grid(rg, _search(rg, s), _coded_fields(s, n_fields), s.masks(n_fields))
        assert np.array_equal(a.view(np.uint32), b.view(np.uint32))


# ---- 4. the processor seam, end to end ----------------------------------------------------------------------------------
def test_processor_seam_package_on_the_polar_scene(rg):
    """``build_grid3d_package`` (NaN data masked by masked_invalid, the QC filter's gate_excluded) returns values[idx32] with
    the mask exactly where the oracle has no gate."""
    from radar_processor_amd import processor_seam as seam
    s = cs.scene("polar_const")
    rng = np.random.default_rng(41)
    nrays, ngates = cs.POLAR["n_elev"] * cs.POLAR["n_az"], cs.POLAR["n_gates"]
    data = rng.normal(15.0, 12.0, (nrays, ngates)).astype(np.float32)
    data[rng.random((nrays, ngates)) < 0.1] = np.nan
    excluded = rng.random(s.n_gates) < 0.2
    radar = SimpleNamespace(nrays=nrays, ngates=ngates,
                            fields={"DBZH": {"data": np.ma.masked_invalid(data), "units": "dBZ"}},
                            gate_x={"data": s.gx.reshape(nrays, ngates)}, gate_y={"data": s.gy.reshape(nrays, ngates)},
                            gate_z={"data": s.gz.reshape(nrays, ngates)},
                            latitude={"data": np.array([-31.4])}, longitude={"data": np.array([-64.2])})
    pkg = seam.build_grid3d_package(radar, "DBZH", cs.POLAR_Z, cs.POLAR_Y, cs.POLAR_X, cs.POLAR_RES, gate_excluded=excluded)
    drop = excluded | ~np.isfinite(data.ravel())
    idx = s.choice_for([drop], "seam")["idx32"][0]
    arr = pkg["arr3d"]
    assert arr.shape == s.shape and isinstance(arr, np.ma.MaskedArray) and pkg["field_metadata"] == {"units": "dBZ"}
    np.testing.assert_array_equal(np.ma.getmaskarray(arr), idx < 0)
    filled = idx >= 0
    assert 0.3 < filled.mean() < 0.95
    np.testing.assert_array_equal(np.ma.getdata(arr)[filled].view(np.uint32), data.ravel()[idx[filled]].view(np.uint32))
