"""From a :class:`gridding.PlaneProducts` request to its planes: the one route every caller takes.

* :class:`ProductPlan` resolves a request against a grid spec -- anything with ``grid_shape`` / ``grid_limits`` (a
  ``GridGeometry``, a ``RoiSearch``, a ``MosaicSearch``) -- once, on the host: level window, refusals, CAPPI plans, the
  levels a fused pass keeps, the distinct PPI angles.  :meth:`ProductPlan.planes_of_grid` / ``planes_of_grids`` reduce
  stored grids with the separate kernels; ``batch.VolumeBatch`` (CSR-free gridder) and the search route of
  ``mosaic.mosaic_fields_device`` reduce their grids through them.
* :func:`grid_products_device` grids through a CSR geometry and either reduces the same way or takes the planes out of the
  gridding kernel's epilogue (``fused``).
* :func:`ordered_record` is the one place that fixes the key order of a field's record.
"""
from __future__ import annotations

from typing import List, Optional, Sequence

import numpy as np

from . import _native, pass_policy
from . import grid_products as gp
from .grid_geometry import GridGeometry
from .gridding import CsrGridder, PlaneProducts, _pass_groups

RECORD_KEYS = ("colmax", "argmax", "colmin", "colmean", "cappi", "ppi", "echo_top", "echo_base", "vil")


def ordered_record(planes: dict) -> dict:
    """One field's record: the planes of ``planes`` under the keys of ``RECORD_KEYS``, in that order."""
    return {key: planes[key] for key in RECORD_KEYS if key in planes}


class ProductPlan:
    """A ``PlaneProducts`` request resolved against ``spec`` (``grid_shape`` / ``grid_limits``).  Host code, no device:

    * ``window``: the level window ``(lo, hi)`` of the column and profile products; a request that holds one is refused
      with ``ValueError`` when the window is empty, a profile product also when the levels are not strictly increasing;
    * ``cappi``: ``{altitude: grid_products.cappi_plan}``, altitudes outside the grid warned about as
      ``constant_altitude_ppi`` does -- once per plan;
    * ``keep_lo``, ``n_keep``: the level range those plans read (what a fused pass keeps of every grid);
    * ``angles``: the distinct PPI angles, in request order."""

    def __init__(self, products: PlaneProducts, spec):
        self.products, self.spec = products, spec
        self.grid_shape = nz, _, _ = tuple(int(s) for s in spec.grid_shape)
        self.window = lo, hi = gp._level_window(nz, *products.window, spec)
        if (products.columns or products.profile) and lo > hi:
            raise ValueError(f"empty level window [{lo}, {hi}]")
        if products.profile:
            gp.profile_levels(spec, nz)
        z_min, z_max = spec.grid_limits[0]
        self.cappi = {alt: gp.cappi_plan((z_min, z_max), nz, alt, products.interpolation) for alt in products.cappi}
        needed = set()
        for alt, plan in self.cappi.items():
            if plan[0] == "outside":
                gp.logger.warning(f"Altitude {alt}m is outside grid range [{z_min}, {z_max}]m")
            else:
                needed.update((plan[1], plan[1] + 1) if plan[0] == "blend" else (plan[1],))
        self.keep_lo, self.n_keep = (min(needed), max(needed) - min(needed) + 1) if needed else (0, 0)
        self.angles = list(dict.fromkeys(products.ppi))
        self._levels = {}

    def profile_levels_device(self, device):
        """The level heights ``rg_column_profile_f32`` reads, on ``device``: uploaded on first use, once per plan."""
        if device not in self._levels:
            self._levels[device] = gp.profile_levels_device(self.spec, self.grid_shape[0], device)
        return self._levels[device]

    def cappi_planes(self, level, dev) -> dict:
        """The CAPPI planes of the request; ``level(z)`` returns grid level ``z`` as a ``[ny, nx]`` plane (levels ``z`` and
        ``z + 1`` adjacent in one buffer).  Launches on the current device's stream."""
        torch = _native.torch_mod()
        lib = _native.load_library()
        _, ny, nx = self.grid_shape
        out = {}
        for alt, plan in self.cappi.items():
            if plan[0] == "outside":
                out[alt] = torch.full((ny, nx), float("nan"), dtype=torch.float32, device=dev)
            elif plan[0] == "level":
                out[alt] = level(plan[1])
            else:
                plane = torch.empty((ny, nx), dtype=torch.float32, device=dev)
                _native.check(lib.rg_cappi_lerp_f32(_native.ptr(level(plan[1])), ny * nx, 0, float(np.float32(plan[2])),
                                                    float(np.float32(plan[3])), _native.ptr(plane), _native.stream_ptr()),
                              "rg_cappi_lerp_f32")
                out[alt] = plane
        return out

    def planes_of_grid(self, grid) -> dict:
        """The record of one stored grid ``[nz, ny, nx]`` (device) through the separate kernels: the planes
        ``column_argmax`` / ``column_max`` / ``column_min`` / ``column_mean`` (over ``window``), ``constant_altitude_ppi``,
        ``constant_elevation_ppi`` and ``column_profile`` give on it, bit for bit."""
        p, (lo, hi) = self.products, self.window
        rec = {}
        with _native.torch_mod().cuda.device(grid.device):
            if p.argmax:
                rec["colmax"], rec["argmax"] = gp._column("max", grid, lo, hi, None, None, None, want_arg=True)
            elif p.colmax:
                rec["colmax"] = gp._column("max", grid, lo, hi, None, None, None)
            if p.colmin:
                rec["colmin"] = gp._column("min", grid, lo, hi, None, None, None)
            if p.colmean:
                rec["colmean"] = gp._column("mean", grid, lo, hi, None, None, None)
            if p.cappi:
                rec["cappi"] = self.cappi_planes(lambda z: grid[z], grid.device)
            if p.ppi:
                rec["ppi"] = {e: gp.constant_elevation_ppi(grid, self.spec, e, p.ppi_interpolation, p.earth_curvature, p.ke)
                              for e in self.angles}
            if p.profile:
                rec.update(gp._profile_planes(grid, self.profile_levels_device(grid.device), lo, hi, p.echo_top, p.echo_base,
                                              p.vil, p.vil_max_dbz, p.profile_interpolation))
        return ordered_record(rec)

    def planes_of_grids(self, grids) -> List[dict]:
        """One record per grid of ``[F, nz, ny, nx]`` (device)."""
        return [self.planes_of_grid(grids[k]) for k in range(grids.shape[0])]


def grid_products_device(geometry: GridGeometry, fields: Sequence, masks: Optional[Sequence] = None, shared_mask=None,
                         products: Optional[PlaneProducts] = None, fill_value: float = np.nan, fused: Optional[bool] = None):
    """Grid device-resident fields and return ONLY 2-D products: a list with one ``dict`` per field --
    ``{"colmax": [ny, nx] float32, "argmax": [ny, nx] int32, "colmin": [ny, nx] float32, "colmean": [ny, nx] float32,
    "cappi": {altitude: [ny, nx] float32}, "ppi": {angle: [ny, nx] float64 / float32}}`` (keys present as requested by
    ``products``).  The planes are bit-identical to ``column_argmax`` / ``column_min`` / ``column_mean`` /
    ``constant_altitude_ppi`` / ``constant_elevation_ppi`` applied to the grid ``grid_fields_device`` returns for the same
    pass.

    ``fused=True``: on large geometries (packed records present) every group of up to four field-volumes runs as ONE launch
    of the row-wise kernel in column mode with its products epilogue -- no 3-D grid is written or read back (640 MB each
    way per field on the bench grid), so a pass needs no grid memory at all; it takes about as long as gridding + reducing
    separately (measured, see below).  COLMAX / argmax / CAPPI alone run ``rg_csr_compact_apply_columns_f32``; a request
    with a column minimum, mean or PPI runs ``rg_csr_compact_apply_planes_f32`` (a mean keeps each column in one workgroup;
    more than ``RG_MAX_SEL_PLANES`` PPIs take further launches of it, each gridding the fields again).  Default
    (``fused=None``) and ``fused=False``: grid as usual, reduce with the separate kernels
    (:meth:`ProductPlan.planes_of_grids`).

    A request with a column profile product (``echo_top`` / ``echo_base`` / ``vil``) adds ``"echo_top": {T: plane}``,
    ``"echo_base": {T: plane}``, ``"vil": plane`` -- what ``column_profile`` returns for the same grid -- and always grids,
    then reduces; ``fused=True`` with one is a ``ValueError``."""
    torch = _native.torch_mod()
    products = products if products is not None else PlaneProducts()
    if fused is None:
        fused = products.fused
    if fused and products.profile:
        raise ValueError("fused=True cannot produce echo_top / echo_base / vil (grid, then reduce: leave fused unset)")
    n_fields = len(fields)
    if n_fields == 0:
        raise ValueError("no fields to grid")
    dev = fields[0].device
    if dev.type != "cuda":
        raise _native.NativeUnavailable("grid_products_device needs device-resident (cuda) tensors")
    if masks is None:
        masks = [None] * n_fields
    plan = ProductPlan(products, geometry)
    nz, ny, nx = plan.grid_shape
    n_gates = int(fields[0].numel())
    results = []
    with torch.cuda.device(dev):
        # the products epilogue (column mode of the row-wise kernel) takes 1-4 fields
        cap = pass_policy.COLUMNS_MAX_FIELDS if fused else None
        for f0, f1, gridder in _pass_groups(geometry, n_gates, n_fields, dev, cap):
            nf = f1 - f0
            gridder.pack(fields[f0:f1], masks[f0:f1], shared_mask)
            if not pass_policy.run_fused(gridder.has_columns_kernel, products.profile, nf, fused):
                grids = torch.empty((nf, nz, ny, nx), dtype=torch.float32, device=dev)
                gridder.apply(grids.view(nf, -1), fill_value)
                results += plan.planes_of_grids(grids)
                continue
            got = {}
            if products.colmax:
                got["colmax"] = torch.empty((nf, ny, nx), dtype=torch.float32, device=dev)
            if products.argmax:
                got["argmax"] = torch.empty((nf, ny, nx), dtype=torch.int32, device=dev)
            kept = torch.empty((nf, plan.n_keep, ny, nx), dtype=torch.float32, device=dev) if plan.n_keep else None
            if products.needs_planes_mode:
                got.update(_fused_planes_pass(gridder, plan, fill_value, kept, got.get("colmax"), got.get("argmax")))
            elif got or kept is not None:            # (neither: nothing but out-of-range CAPPIs)
                gridder.apply_columns(out=None, fill_value=fill_value, level_planes=kept, keep_lo=plan.keep_lo,
                                      col_max=got.get("colmax"), col_arg=got.get("argmax"), col_window=plan.window)
            for k in range(nf):
                rec = {key: per_field[k] for key, per_field in got.items()}
                if products.cappi:
                    rec["cappi"] = plan.cappi_planes(lambda z: kept[k, z - plan.keep_lo], dev)
                results.append(ordered_record(rec))
    return results


def _fused_planes_pass(gridder: CsrGridder, plan: ProductPlan, fill_value, kept, cmax, carg) -> dict:
    """The planes-mode launches of one field group (``grid_products_device``): the first computes every column product, the
    kept levels and the samples of the first ``RG_MAX_SEL_PLANES`` PPIs; any further PPIs take one more launch per
    ``RG_MAX_SEL_PLANES``.  Returns ``{"colmin": [F, ny, nx], "colmean": [F, ny, nx], "ppi": [one {angle: plane} per field]}``
    (keys as requested)."""
    torch = _native.torch_mod()
    products, angles = plan.products, plan.angles
    dev = gridder.dev
    nf = gridder.n_fields
    _, ny, nx = gridder.grid_shape
    got = {}
    cmin = torch.empty((nf, ny, nx), dtype=torch.float32, device=dev) if products.colmin else None
    cmean = torch.empty((nf, ny, nx), dtype=torch.float32, device=dev) if products.colmean else None
    ppi_plans = [gp.ppi_plan(plan.spec, e, products.ppi_interpolation, products.earth_curvature, products.ke, dev)
                 for e in angles]
    cap = _native.RG_MAX_SEL_PLANES
    groups = [list(range(g0, min(len(angles), g0 + cap))) for g0 in range(0, len(angles), cap)] or [[]]
    per_field = [{} for _ in range(nf)]
    for gi, group in enumerate(groups):
        first = gi == 0
        samples = torch.empty((nf, len(group), 2, ny, nx), dtype=torch.float32, device=dev) if group else None
        gridder.apply_planes(out=None, fill_value=fill_value, level_planes=kept if first else None, keep_lo=plan.keep_lo,
                             col_max=cmax if first else None, col_arg=carg if first else None,
                             col_min=cmin if first else None, col_mean=cmean if first else None, col_window=plan.window,
                             sel_levels=[ppi_plans[i][0] for i in group], sel_samples=samples)
        for j, i in enumerate(group):
            for k in range(nf):
                per_field[k][angles[i]] = gp.ppi_finish(ppi_plans[i], samples[k, j], products.ppi_interpolation)
    if cmin is not None:
        got["colmin"] = cmin
    if cmean is not None:
        got["colmean"] = cmean
    if products.ppi:
        got["ppi"] = per_field
    return got
