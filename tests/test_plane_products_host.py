"""CPU-side checks of the planes mode (no GPU needed): the PlaneProducts request (defaults, validation, the old positional
meaning), the ctypes mirror of rg_plane_request, and the argument validation of rg_csr_compact_apply_planes_f32 /
rg_csr_planes_workspace_bytes / rg_elevation_ppi_plan_f32 / rg_elevation_ppi_finish_f32 -- every call here fails
validation (or has nothing to do) before anything would be launched."""
import ctypes
import os
import re

import numpy as np
import pytest

import radar_processor_amd as rg
from conftest import REPO
from radar_processor_amd import _native

P = 1 << 12                                  # a 16-byte aligned address that is never dereferenced


def test_plane_products_defaults_and_positional_meaning():
    spec = rg.PlaneProducts()
    assert (spec.colmax, spec.argmax, spec.cappi, spec.interpolation, spec.fused) == (True, True, (), "linear", None)
    assert (spec.colmin, spec.colmean, spec.ppi) == (False, False, ())
    assert (spec.ppi_interpolation, spec.earth_curvature, spec.ke) == ("linear", True, 4.0 / 3.0)
    assert not spec.needs_planes_mode and spec.columns
    # the arguments before `fused` keep their positions
    spec = rg.PlaneProducts(False, False, (1000, 2000.5), "nearest", 1, 5, None, None, True)
    assert (spec.colmax, spec.argmax, spec.cappi, spec.interpolation) == (False, False, (1000.0, 2000.5), "nearest")
    assert spec.window == (1, 5, None, None) and spec.fused is True
    assert not spec.columns and not spec.needs_planes_mode
    spec = rg.PlaneProducts(colmax=False, argmax=False, colmin=True)
    assert spec.columns and spec.needs_planes_mode and not spec.colmax
    spec = rg.PlaneProducts(ppi=(0.5, 2), ppi_interpolation="nearest", earth_curvature=False, ke=1)
    assert spec.ppi == (0.5, 2.0) and all(isinstance(e, float) for e in spec.ppi)
    assert (spec.ppi_interpolation, spec.earth_curvature, spec.ke) == ("nearest", False, 1.0) and spec.needs_planes_mode
    assert rg.PlaneProducts(colmean=True).needs_planes_mode


def test_plane_products_validation_follows_constant_elevation_ppi():
    with pytest.raises(ValueError, match="Unknown interpolation method"):
        rg.PlaneProducts(ppi=(0.5,), ppi_interpolation="cubic")
    with pytest.raises(ValueError, match="Unknown interpolation method"):
        rg.PlaneProducts(interpolation="cubic")


def test_plane_request_layout_matches_the_header():
    header = open(os.path.join(REPO, "include", "radargrid_hip.h")).read()
    assert re.search(r"#define RG_MAX_SEL_PLANES (\d+)", header).group(1) == str(_native.RG_MAX_SEL_PLANES)
    assert "#define RG_PPI_SEL_NONE (-1)" in header and _native.RG_PPI_SEL_NONE == -1
    R = _native.PlaneRequest
    assert ctypes.sizeof(R) == 112                   # 64-bit pointers, int32 pairs: no padding anywhere
    assert (R.keep_lo.offset, R.col_max.offset, R.col_lo.offset, R.n_sel.offset) == (16, 24, 56, 64)
    assert (R.sel_levels.offset, R.sel_samples.offset) == (72, 104)


def _request(**kw):
    req = _native.PlaneRequest(col_lo=0, col_hi=1)
    for k, v in kw.items():
        if k == "sel_levels":
            for i, p in enumerate(v):
                req.sel_levels[i] = p
        else:
            setattr(req, k, v)
    return req


def _planes(req, n_fields=1, n_vox=128, z_pieces=1, workspace=None, workspace_bytes=0, stride=None):
    """rg_csr_compact_apply_planes_f32 on a 2 x 1 x 64 grid without pairs; `req` None passes a null request."""
    lib = rg.load_library(require_device=False)
    stride = (1 if n_fields == 1 else 2 if n_fields == 2 else 4 if n_fields <= 4 else 8) if stride is None else stride
    return lib.rg_csr_compact_apply_planes_f32(P, 0, P, P, _native.RG_REC_ORDER_DISPATCH, 120 << 23, P, P, n_vox, 0, 64, 1, P,
                                               n_fields, stride, 64, 0.0, None if req is None else ctypes.byref(req), 256,
                                               z_pieces, None, workspace, workspace_bytes, 0, None)


def test_apply_planes_argument_validation():
    lib = rg.load_library(require_device=False)
    ok = _request(col_min=P)
    assert _planes(ok, n_vox=0) == _native.RG_OK                       # valid, and nothing to do: no launch
    assert _planes(None) == _native.RG_EINVAL and b"null request" in lib.rg_last_error()
    for nf in (0, 5):
        assert _planes(ok, n_fields=nf) == _native.RG_EUNSUPPORTED, nf
    assert _planes(ok, n_fields=2, stride=4) == _native.RG_EINVAL
    # the mean's running sum is one piece
    assert _planes(_request(col_mean=P), z_pieces=2) == _native.RG_EINVAL and b"z_pieces" in lib.rg_last_error()
    assert _planes(_request(col_mean=P), z_pieces=1, n_vox=0) == _native.RG_OK
    # selections: at most RG_MAX_SEL_PLANES, every plane and the samples present
    cap = _native.RG_MAX_SEL_PLANES
    assert _planes(_request(n_sel=cap + 1, sel_levels=[P] * cap, sel_samples=P)) == _native.RG_EINVAL
    assert _planes(_request(n_sel=-1, col_min=P)) == _native.RG_EINVAL
    assert _planes(_request(n_sel=2, sel_levels=[P, P])) == _native.RG_EINVAL and b"sel_samples" in lib.rg_last_error()
    assert _planes(_request(n_sel=2, sel_levels=[P], sel_samples=P)) == _native.RG_EINVAL
    assert _planes(_request(n_sel=cap, sel_levels=[P] * cap, sel_samples=P), n_vox=0) == _native.RG_OK
    # nothing to produce
    assert _planes(_request()) == _native.RG_EINVAL and b"nothing to produce" in lib.rg_last_error()
    assert _planes(_request(col_arg=P, col_min=P)) == _native.RG_EINVAL             # an arg plane needs the max
    # level windows (the grid has 2 planes)
    for lo, hi in ((1, 0), (-1, 1), (0, 2)):
        assert _planes(_request(col_min=P, col_lo=lo, col_hi=hi)) == _native.RG_EINVAL, (lo, hi)
        assert _planes(_request(col_mean=P, col_lo=lo, col_hi=hi)) == _native.RG_EINVAL, (lo, hi)
    assert _planes(_request(level_planes=P, keep_lo=1, n_keep=2)) == _native.RG_EINVAL
    assert _planes(_request(col_max=P), z_pieces=3) == _native.RG_EINVAL               # more pieces than planes
    # level pieces of the max / min need the workspace rg_csr_planes_workspace_bytes names
    need = lib.rg_csr_planes_workspace_bytes(1, 64, 1, 2, 1, 1)
    assert _planes(_request(col_max=P, col_min=P), z_pieces=2) == _native.RG_EWORKSPACE
    assert _planes(_request(col_max=P, col_min=P), z_pieces=2, workspace=P, workspace_bytes=need - 1) == _native.RG_EWORKSPACE
    assert _planes(_request(col_min=P), z_pieces=2, workspace=P,
                   workspace_bytes=lib.rg_csr_planes_workspace_bytes(1, 64, 1, 2, 0, 1) - 1) == _native.RG_EWORKSPACE


def test_planes_workspace_bytes():
    lib = rg.load_library(require_device=False)
    ny, nx = 10, 64
    assert lib.rg_csr_planes_workspace_bytes(ny, nx, 3, 1, 1, 1) == 0
    assert lib.rg_csr_planes_workspace_bytes(ny, nx, 3, 2, 1, 1) == 2 * 3 * ny * nx * 12
    assert lib.rg_csr_planes_workspace_bytes(ny, nx, 3, 2, 0, 1) == 2 * 3 * ny * nx * 4
    assert lib.rg_csr_planes_workspace_bytes(ny, nx, 3, 2, 0, 0) == 0
    assert lib.rg_csr_planes_workspace_bytes(ny, nx, 4, 3, 1, 0) == lib.rg_csr_columns_workspace_bytes(ny, nx, 4, 3)
    for bad in ((0, nx, 1, 2), (ny, -1, 1, 2), (ny, nx, 0, 2), (ny, nx, 5, 2), (ny, nx, 1, 0)):
        assert lib.rg_csr_planes_workspace_bytes(*bad, 1, 1) == _native.RG_EINVAL, bad


def test_elevation_ppi_plan_and_finish_argument_validation():
    lib = rg.load_library(require_device=False)
    scal = (0.99, 0.1, 0.1, 8.5e6, 7.2e13, 0.0, 10000.0, 500.0)

    def plan(xc=P, yc=P, nz=21, ny=8, nx=8, z_step=500.0, linear=1, sel=P, w_hi=P):
        s = scal[:7] + (z_step,)
        return lib.rg_elevation_ppi_plan_f32(xc, yc, nz, ny, nx, *s, 1, linear, sel, w_hi, None)
    assert plan(xc=None) == _native.RG_EINVAL and plan(sel=None) == _native.RG_EINVAL
    assert plan(w_hi=None) == _native.RG_EINVAL and b"w_hi" in lib.rg_last_error()
    assert plan(nz=0) == _native.RG_EINVAL and plan(nz=0xFFFF) == _native.RG_EINVAL and plan(ny=0) == _native.RG_EINVAL
    assert plan(z_step=0.0) == _native.RG_EINVAL
    assert lib.rg_elevation_ppi_finish_f32(None, P, P, 64, 1, P, None) == _native.RG_EINVAL
    assert lib.rg_elevation_ppi_finish_f32(P, P, None, 64, 1, P, None) == _native.RG_EINVAL
    assert lib.rg_elevation_ppi_finish_f32(P, None, P, 64, 1, P, None) == _native.RG_EINVAL
    assert lib.rg_elevation_ppi_finish_f32(P, P, P, -1, 1, P, None) == _native.RG_EINVAL
    assert lib.rg_elevation_ppi_finish_f32(P, None, P, 0, 0, P, None) == _native.RG_OK       # nearest needs no weights


def test_products_only_pass_refuses_host_tensors():
    torch = pytest.importorskip("torch")
    f = torch.zeros(8, dtype=torch.float32)
    geom = rg.GridGeometry((2, 2, 2), ((0.0, 1000.0), (-1.0, 1.0), (-1.0, 1.0)), np.arange(9, dtype=np.int32),
                           np.arange(8, dtype=np.int32), np.ones(8, dtype=np.float32), toa=17000.0)
    with pytest.raises(_native.NativeUnavailable):
        rg.grid_products_device(geom, [f], products=rg.PlaneProducts(colmin=True, colmean=True, ppi=(0.5,)), fused=True)


# ---- ProductPlan: a request resolved against a grid spec, on the host ---------------------------------------------------------
class _Spec:
    grid_shape = (5, 3, 5)
    grid_limits = ((1000, 5000), (-1, 1), (-1, 1))


def test_product_plan_resolves_window_cappi_plans_kept_levels_and_angles_once(caplog):
    from radar_processor_amd.plane_products import ProductPlan
    spec = rg.PlaneProducts(cappi=(500.0, 3000.0, 3500.0, 3000.0), ppi=(1.5, 0.5, 1.5), z_min_idx=1, z_max_idx=3)
    with caplog.at_level("WARNING", logger="radar_grid.products"):
        plan = ProductPlan(spec, _Spec())
    assert plan.window == (1, 3)
    assert plan.cappi == {500.0: ("outside",), 3000.0: ("level", 2), 3500.0: ("blend", 2, 0.5, 0.5)}
    assert list(plan.cappi) == [500.0, 3000.0, 3500.0]
    assert (plan.keep_lo, plan.n_keep) == (2, 2)
    assert plan.angles == [1.5, 0.5]
    warnings = [r.getMessage() for r in caplog.records if r.levelname == "WARNING"]
    assert warnings == ["Altitude 500.0m is outside grid range [1000, 5000]m"]


def test_product_plan_refuses_an_empty_window_only_for_window_products():
    from radar_processor_amd.plane_products import ProductPlan
    empty = dict(z_min_idx=3, z_max_idx=1)
    with pytest.raises(ValueError, match="empty level window"):
        ProductPlan(rg.PlaneProducts(colmax=True, argmax=False, **empty), _Spec())
    with pytest.raises(ValueError, match="empty level window"):
        ProductPlan(rg.PlaneProducts(colmax=False, argmax=False, vil=True, **empty), _Spec())
    plan = ProductPlan(rg.PlaneProducts(colmax=False, argmax=False, cappi=(3500.0,), **empty), _Spec())
    assert plan.window == (3, 1) and (plan.keep_lo, plan.n_keep) == (2, 2)


def test_product_plan_refuses_levels_that_do_not_increase_at_resolve_time():
    from radar_processor_amd.plane_products import ProductPlan

    class Flat(_Spec):
        grid_limits = ((1000, 1000), (-1, 1), (-1, 1))
    with pytest.raises(ValueError, match="strictly increasing"):
        ProductPlan(rg.PlaneProducts(colmax=False, argmax=False, vil=True), Flat())
    ProductPlan(rg.PlaneProducts(), Flat())                  # no profile product: the levels are nobody's business


def test_ordered_record_fixes_the_key_order_of_every_subset():
    import itertools
    import random
    from radar_processor_amd.plane_products import RECORD_KEYS, ordered_record
    assert RECORD_KEYS == ("colmax", "argmax", "colmin", "colmean", "cappi", "ppi", "echo_top", "echo_base", "vil")
    rng = random.Random(0)
    for n in range(len(RECORD_KEYS) + 1):
        for subset in itertools.combinations(RECORD_KEYS, n):
            keys = list(subset)
            rng.shuffle(keys)
            planes = {k: object() for k in keys}
            rec = ordered_record(planes)
            assert list(rec) == list(subset)
            assert all(rec[k] is planes[k] for k in subset)
