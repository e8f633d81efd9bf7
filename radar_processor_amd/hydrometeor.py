"""Hydrometeor classification in the polar domain, on the device (include/radargrid_hydro.h; kernels in csrc/rg_hydro.hip): what
KDP and the corrected Z and ZDR are produced for -- the echo type of every gate.

* :func:`texture_device` is the standard deviation (and mean) of a field in a window along the ray (``rg_polar_texture_f32``):
  SD(Z) and SD(PHIDP), the two variables that tell weather from clutter and insects;
* :class:`MembershipTable` holds a fuzzy-logic scheme -- classes, variables, trapezoids per bin of a condition variable,
  weights -- validates it and compiles the block of cells the kernel reads;
* :func:`classify_device` scores every gate against a table and returns the winning class (``rg_fuzzy_classify_f32``);
* :func:`beam_temperature` turns a sounding into the per-sweep temperature table (host, float64, no device);
* :func:`classify_hydrometeors_device` chains them: two textures, then the classifier with :data:`HYDROMETEOR_TABLE_S_BAND`
  (or a table of the caller's); :func:`classify_hydrometeors` is its NumPy-in, NumPy-out form;
* :func:`class_mask_device` turns classes into the uint8 mask the other polar-domain calls and the gridders take.

Fields are float32 ``[n_rays, n_gates]`` (tensor or ndarray): one row is one ray, the sweeps of a volume are stacked.  The
outputs have the same shape; ``classes.float().reshape(-1)`` is a field the closest-gate weighting of the gridders can grid.

The contract is this build's own (the header states it; ``tests/hydro_oracle.py`` restates it in NumPy and the tests hold the
kernels EQUAL to that, bit for bit: the sums of the texture are integers in 2^-10 fixed point and every float step of the
classifier is stated).  Parity with the WSR-88D HCA, wradlib and CSU RadarTools is unpinned.  The device functions enqueue on
torch's current stream, validate every argument before the device is touched and never synchronise with the host.
"""
from __future__ import annotations

import math
from typing import Dict, NamedTuple, Optional, Sequence, Tuple

import numpy as np

from . import _native
from .convection import _finite
from .grid_products import compute_beam_height
from .motion import _device_of, _dtype_name, _is_int, _to_device
from .phase import _check_like

MAX_ABS = _native.RG_HYDRO_MAX_ABS
MAX_HALF_GATES = _native.RG_HYDRO_MAX_HALF_GATES
TEXTURE_TILE = _native.RG_HYDRO_TEXTURE_TILE
MAX_VARS = _native.RG_HYDRO_MAX_VARS
MAX_CLASSES = _native.RG_HYDRO_MAX_CLASSES
MAX_BINS = _native.RG_HYDRO_MAX_BINS
MAX_CELLS = _native.RG_HYDRO_MAX_CELLS
UNCLASSIFIED = _native.RG_HYDRO_UNCLASSIFIED
MAX_GATES = _native.RG_PHASE_MAX_GATES
KINDS = {"additive": 0, "multiplicative": 1}

#: the variables of :func:`classify_hydrometeors_device`, in the order its tables hold them
HYDROMETEOR_VARIABLES = ("Z", "ZDR", "KDP", "RHOHV", "SD(Z)", "SD(PHIDP)", "T")
#: the classes of the preset, after Park et al. 2009; class ``k`` of this tuple is the value ``k + 1`` of ``classes``
HYDROMETEOR_CLASSES = ("ground clutter", "biological", "dry snow", "wet snow", "crystals", "graupel", "big drops", "rain",
                       "heavy rain", "rain and hail")


class Texture(NamedTuple):
    """What :func:`texture_device` returns, each of the field's shape or ``None`` when not asked for: ``sd`` float32 (the
    population standard deviation of the valid gates of the window), ``mean`` float32, both NaN where the window holds too few
    valid gates, and ``count`` uint16 (valid gates of the window, written everywhere)."""
    sd: object
    mean: object
    count: object


class FuzzyClasses(NamedTuple):
    """What :func:`classify_device` returns: ``classes`` uint8 (class ``c`` of the table is ``c + 1``; 0 = unclassified),
    ``score`` float32 (the winner's score, NaN where unclassified) and ``second`` uint8 (the runner-up, 0 where there is none);
    the last two ``None`` when not asked for."""
    classes: object
    score: object
    second: object


class HydrometeorClasses(NamedTuple):
    """What :func:`classify_hydrometeors_device` returns: the three members of :class:`FuzzyClasses` and the two textures it
    formed on the way (``sd_phidp`` is ``None`` without a PHIDP)."""
    classes: object
    score: object
    second: object
    sd_dbz: object
    sd_phidp: object


# ---- the table ---------------------------------------------------------------------------------------------------------------
class MembershipTable:
    """A fuzzy-logic scheme: ``classes`` (C names), ``variables`` (V names), ``vertices`` float ``[B][C][V][4]`` -- the trapezoid
    ``(x1, x2, x3, x4)`` of every (bin, class, variable); ``[C][V][4]`` is taken for every bin -- and ``weights`` ``[C][V]``.
    ``kinds`` names every variable ``"additive"`` (its memberships enter the weighted mean) or ``"multiplicative"`` (they
    multiply the mean; the weight is not used); ``required`` names the variables without which a gate is not classified;
    ``condition`` names the variable whose value chooses the bin, by ``edges`` (B - 1 ascending numbers: the bin of a gate is
    the number of edges at or below its value, compared in float32).

    Validated here, since the kernel trusts the table: every vertex finite or infinite (never NaN), ``x1 <= x2 <= x3 <= x4``
    after rounding to float32, a flank (``x1 < x2`` or ``x3 < x4``) between two finite vertices (an infinite vertex is an open
    shoulder: ``x1 = x2 = -inf`` or ``x3 = x4 = +inf``), weights finite and not negative, the sizes within the limits of the
    header.  ``cells`` is the compiled float64 ``[B][C][V][6]`` block ``(x1, x2, x3, x4, r, f)``: the vertices as float32
    values, ``r = 1 / (x2 - x1)`` where ``x2 > x1``, else 0, and ``f = 1 / (x4 - x3)`` likewise."""

    def __init__(self, classes: Sequence[str], variables: Sequence[str], vertices, weights, *, kinds: Optional[Sequence[str]] = None,
                 required: Sequence[str] = (), condition: Optional[str] = None, edges: Sequence[float] = ()):
        self.class_names = tuple(classes)
        self.variable_names = tuple(variables)
        for names, what, most in ((self.class_names, "classes", MAX_CLASSES), (self.variable_names, "variables", MAX_VARS)):
            if not names or len(names) > most or not all(isinstance(n, str) for n in names) or len(set(names)) != len(names):
                raise ValueError(f"{what} must be 1 .. {most} different names, got {names!r}")
        C, V = len(self.class_names), len(self.variable_names)
        kinds = ("additive",) * V if kinds is None else tuple(kinds)
        if len(kinds) != V or any(k not in KINDS for k in kinds):
            raise ValueError(f"kinds: one of {sorted(KINDS)} per variable, got {kinds!r}")
        if all(k == "multiplicative" for k in kinds):
            raise ValueError("kinds: at least one variable must be additive")
        self.kinds = tuple(KINDS[k] for k in kinds)
        required = tuple(required)
        if any(name not in self.variable_names for name in required):
            raise ValueError(f"required names a variable the table does not have: {required!r}")
        self.required = required
        self.required_bits = sum(1 << self.variable_names.index(name) for name in set(required))
        if condition is not None and condition not in self.variable_names:
            raise ValueError(f"condition names a variable the table does not have: {condition!r}")
        self.condition = condition
        self.cond_var = -1 if condition is None else self.variable_names.index(condition)
        try:
            self.edges = tuple(_finite(e, "edges: every edge") for e in edges)
        except TypeError:
            raise ValueError(f"edges must be a sequence of numbers, not {edges!r}") from None
        if any(b < a for a, b in zip(self.edges, self.edges[1:])):
            raise ValueError(f"edges must ascend, got {self.edges!r}")
        B = len(self.edges) + 1
        if B > MAX_BINS:
            raise ValueError(f"edges: at most {MAX_BINS - 1} edges ({MAX_BINS} bins), got {len(self.edges)}")
        if condition is None and B > 1:
            raise ValueError("edges without a condition variable")
        if B * C * V > MAX_CELLS:
            raise ValueError(f"{B} bins x {C} classes x {V} variables are more than {MAX_CELLS} cells")
        vertices = np.asarray(vertices, dtype=np.float64)
        if vertices.shape == (C, V, 4):
            vertices = np.broadcast_to(vertices, (B, C, V, 4))
        if vertices.shape != (B, C, V, 4):
            raise ValueError(f"vertices must be [{B}][{C}][{V}][4] (bins, classes, variables, x1 .. x4), got {list(vertices.shape)}")
        if np.isnan(vertices).any():
            raise ValueError("vertices: NaN is not a vertex")
        with np.errstate(over="ignore"):
            rounded = vertices.astype(np.float32).astype(np.float64)
        if (np.isinf(rounded) & np.isfinite(vertices)).any():
            raise ValueError("vertices: a finite vertex is beyond float32")
        if (rounded[..., 1:] < rounded[..., :-1]).any():
            raise ValueError("vertices must ascend: x1 <= x2 <= x3 <= x4 for every bin, class and variable")
        for lo, hi, what in ((0, 1, "x1 < x2"), (2, 3, "x3 < x4")):
            a, b = rounded[..., lo], rounded[..., hi]
            if ((a != b) & ~(np.isfinite(a) & np.isfinite(b))).any():
                raise ValueError(f"vertices: a flank ({what}) needs two finite vertices; an open shoulder has both infinite")
        weights = np.asarray(weights, dtype=np.float64)
        if weights.shape != (C, V) or not np.isfinite(weights).all() or (weights < 0).any():
            raise ValueError(f"weights must be [{C}][{V}], finite and not negative")
        self.vertices = np.ascontiguousarray(rounded)
        self.weights = np.ascontiguousarray(weights)
        self.cells = compile_cells(self.vertices)
        for a in (self.vertices, self.weights, self.cells):
            a.setflags(write=False)
        self._device_cells: Dict[object, object] = {}

    n_bins = property(lambda self: len(self.edges) + 1)
    n_classes = property(lambda self: len(self.class_names))
    n_vars = property(lambda self: len(self.variable_names))

    def class_value(self, name: str) -> int:
        """The value of ``classes`` that stands for the class called ``name``: its index plus one."""
        if name not in self.class_names:
            raise ValueError(f"the table has no class {name!r}: {self.class_names!r}")
        return self.class_names.index(name) + 1

    def device_cells(self, dev):
        """The cells as a float64 tensor on ``dev``; the copy is made once per device."""
        dev = _native.canonical_device(dev)
        if dev not in self._device_cells:
            self._device_cells[dev] = _to_device(self.cells, dev)
        return self._device_cells[dev]


def compile_cells(vertices) -> np.ndarray:
    """Vertices ``[..., 4]`` (already float32 values, ascending) -> cells float64 ``[..., 6] = (x1, x2, x3, x4, r, f)`` with
    ``r = 1 / (x2 - x1)`` where ``x2 > x1`` and both are finite, else 0, and ``f = 1 / (x4 - x3)`` likewise."""
    v = np.asarray(vertices, dtype=np.float64)
    cells = np.zeros(v.shape[:-1] + (6,), np.float64)
    cells[..., :4] = v
    for lo, hi, at in ((0, 1, 4), (2, 3, 5)):
        a, b = v[..., lo], v[..., hi]
        ok = np.isfinite(a) & np.isfinite(b) & (b > a)
        with np.errstate(invalid="ignore"):                   # inf - inf at an open shoulder: not used
            cells[..., at] = np.where(ok, 1.0 / np.where(ok, b - a, 1.0), 0.0)
    return cells


# ---- validation (host only) --------------------------------------------------------------------------------------------------
def _check_field(field, what: str) -> Tuple[int, int]:
    if not hasattr(field, "shape") or not hasattr(field, "dtype"):
        raise ValueError(f"{what} must be a tensor or an ndarray, not {type(field).__name__}")
    shape = tuple(int(n) for n in field.shape)
    if _dtype_name(field) != "float32" or len(shape) != 2:
        raise ValueError(f"{what} must be float32 [n_rays, n_gates]; got {_dtype_name(field)} {list(shape)}")
    if shape[0] < 1 or shape[1] > MAX_GATES or shape[0] * shape[1] >= 2 ** 31:
        raise ValueError(f"{what}: at least one ray, at most {MAX_GATES} gates per ray and fewer than 2^31 gates in all; got "
                         f"{list(shape)}")
    return shape


def _check_texture(half_gates, min_valid) -> Tuple[int, int]:
    if not _is_int(half_gates) or not 1 <= half_gates <= MAX_HALF_GATES:
        raise ValueError(f"half_gates must be an integer in 1 .. {MAX_HALF_GATES}, not {half_gates!r}")
    if min_valid is None:
        min_valid = int(half_gates) + 1
    if not _is_int(min_valid) or not 1 <= min_valid <= 2 * MAX_HALF_GATES + 1:
        raise ValueError(f"min_valid must be an integer in 1 .. {2 * MAX_HALF_GATES + 1}, not {min_valid!r}")
    return int(half_gates), int(min_valid)


def _check_min_score(min_score) -> float:
    min_score = _finite(min_score, "min_score")
    if min_score < 0.0:
        raise ValueError(f"min_score must not be negative, got {min_score!r}")
    return min_score


def _check_variables(variables, table, per_sweep, rays_per_sweep):
    """-> (the field that gives the shape, [(array or None, is per sweep)] in the table's order, rays_per_sweep)."""
    if not isinstance(table, MembershipTable):
        raise ValueError(f"table must be a MembershipTable, not {type(table).__name__}")
    names = table.variable_names
    if isinstance(variables, dict):
        unknown = [name for name in variables if name not in names]
        if unknown:
            raise ValueError(f"variables names {unknown!r}, which the table does not have: {names!r}")
        values = [variables.get(name) for name in names]
    else:
        values = list(variables)
        if len(values) != len(names):
            raise ValueError(f"variables: one entry per variable of the table ({len(names)}: {names!r}), got {len(values)}")
    per_sweep = tuple(per_sweep)
    if any(name not in names for name in per_sweep):
        raise ValueError(f"per_sweep names a variable the table does not have: {per_sweep!r}")
    fields = [(name, v) for name, v in zip(names, values) if v is not None and name not in per_sweep]
    if not fields:
        raise ValueError("variables: at least one [n_rays, n_gates] field is needed, every variable is absent or per sweep")
    first = fields[0][1]
    R, G = _check_field(first, f"variable {fields[0][0]!r}")
    for name, v in fields[1:]:
        _check_like(v, first, f"variable {name!r}")
    if rays_per_sweep is None:
        tables = [v for name, v in zip(names, values) if v is not None and name in per_sweep]
        n_sweeps = int(tables[0].shape[0]) if tables and hasattr(tables[0], "shape") and len(tables[0].shape) == 2 else 1
        rays_per_sweep = R // n_sweeps if n_sweeps >= 1 and R % max(n_sweeps, 1) == 0 else 0
    if not _is_int(rays_per_sweep) or rays_per_sweep < 1 or R % rays_per_sweep:
        raise ValueError(f"rays_per_sweep must be an integer of at least 1 that divides the {R} rays, not {rays_per_sweep!r}")
    out = []
    for v_index, (name, v) in enumerate(zip(names, values)):
        if v is None:
            if name in table.required or v_index == table.cond_var:
                raise ValueError(f"variable {name!r} is required by the table (or is its condition variable) and is absent")
            out.append((None, True))
        elif name in per_sweep:
            want = (R // rays_per_sweep, G)
            if not hasattr(v, "shape") or tuple(int(n) for n in v.shape) != want or _dtype_name(v) != "float32":
                raise ValueError(f"variable {name!r} is per sweep: float32 {list(want)} (sweeps, gates), got "
                                 f"{_dtype_name(v) if hasattr(v, 'dtype') else type(v).__name__} {list(getattr(v, 'shape', []))}")
            out.append((v, True))
        else:
            out.append((v, False))
    return first, out, int(rays_per_sweep)


# ---- device ------------------------------------------------------------------------------------------------------------------
def _texture(lib, torch, src, m, shape, half_gates, min_valid, centre_only, want_sd, want_mean, want_count) -> Texture:
    new = lambda on, dtype: torch.empty(shape, dtype=dtype, device=src.device) if on else None          # noqa: E731
    sd, mean, count = new(want_sd, torch.float32), new(want_mean, torch.float32), new(want_count, torch.uint16)
    if shape[1]:                 # rays without gates: the empty outputs are the result (and an empty tensor has no address)
        _native.check(lib.rg_polar_texture_f32(_native.ptr(src), _native.ptr(m), shape[0], shape[1], half_gates, min_valid,
                                               1 if centre_only else 0, _native.ptr(sd), _native.ptr(mean), _native.ptr(count),
                                               _native.stream_ptr()), "rg_polar_texture_f32")
    return Texture(sd, mean, count)


def _classify(lib, torch, tensors, per_sweep_bits, table: MembershipTable, cells, m, shape, rays_per_sweep, min_score, want_score,
              want_second) -> FuzzyClasses:
    dev = cells.device
    cls = torch.empty(shape, dtype=torch.uint8, device=dev)
    score = torch.empty(shape, dtype=torch.float32, device=dev) if want_score else None
    second = torch.empty(shape, dtype=torch.uint8, device=dev) if want_second else None
    V = table.n_vars
    c_vars = (_native.c_void_p * V)(*(_native.ptr(t) for t in tensors))
    c_kinds = (_native.c_int32 * V)(*table.kinds)
    c_edges = (_native.c_double * max(len(table.edges), 1))(*table.edges)
    c_weights = (_native.c_double * (table.n_classes * V))(*table.weights.reshape(-1).tolist())
    if shape[1]:
        _native.check(lib.rg_fuzzy_classify_f32(c_vars, c_kinds, V, per_sweep_bits, table.required_bits, rays_per_sweep, _native.ptr(m),
                                                shape[0], shape[1], table.cond_var, c_edges, table.n_bins, _native.ptr(cells),
                                                table.n_classes, c_weights, min_score, _native.ptr(cls), _native.ptr(score),
                                                _native.ptr(second), _native.stream_ptr()), "rg_fuzzy_classify_f32")
    return FuzzyClasses(cls, score, second)


def _stage_variables(torch, checked, shape, rays_per_sweep, dev):
    """The variables on ``dev`` and the per-sweep bits.  An ABSENT variable is a per-sweep table of NaN: present at no gate."""
    tensors, bits, absent = [], 0, None
    for v, (value, is_per_sweep) in enumerate(checked):
        if value is None:
            if absent is None:
                absent = torch.full((shape[0] // rays_per_sweep, shape[1]), float("nan"), dtype=torch.float32, device=dev)
            tensors.append(absent)
        else:
            tensors.append(_to_device(value, dev))
        bits |= (1 << v) if is_per_sweep else 0
    return tensors, bits


def texture_device(field, *, half_gates: int, min_valid: Optional[int] = None, mask=None, centre_only: bool = False,
                   return_mean: bool = False, return_count: bool = False) -> Texture:
    """The texture of ``field`` (float32 ``[n_rays, n_gates]``) along the ray: the population standard deviation of the valid
    gates within ``half_gates`` (1 .. 63) gates on either side of every gate, a window an edge of the ray clips.  A gate is valid
    when it is finite, at most 8192 in magnitude and ``mask`` (optional; non-zero leaves the gate out) is 0 there; values are
    taken to 2^-10 of their unit (ties to even), the sums are exact.  NaN where the window holds fewer than ``min_valid`` valid
    gates (default ``half_gates + 1``: more than half the window) and, with ``centre_only``, where the gate itself is not valid.
    ``return_mean`` adds the mean of the same gates, ``return_count`` their number (uint16, written everywhere).  One launch, no
    host synchronisation.  Returns :class:`Texture`."""
    shape = _check_field(field, "field")
    half_gates, min_valid = _check_texture(half_gates, min_valid)
    _check_like(mask, field, "mask", None)
    torch = _native.torch_mod()
    lib = _native.load_library()
    dev = _device_of(field, mask)
    src = _to_device(field, dev)
    m = None if mask is None else _to_device(mask, dev, torch.uint8)
    with torch.cuda.device(dev):
        return _texture(lib, torch, src, m, shape, half_gates, min_valid, centre_only, True, return_mean, return_count)


def texture(field, **kw) -> Texture:
    """:func:`texture_device` for NumPy arrays: the field is staged through device memory, the members come back as ndarrays."""
    return Texture(*(None if o is None else o.cpu().numpy() for o in texture_device(field, **kw)))


def classify_device(variables, table: MembershipTable, *, per_sweep: Sequence[str] = (), rays_per_sweep: Optional[int] = None,
                    mask=None, min_score: float = 0.0, return_score: bool = False, return_second: bool = False) -> FuzzyClasses:
    """The class of every gate by the fuzzy logic of ``table``.  ``variables`` is a dict by the table's variable names or a
    sequence in their order, each float32 ``[n_rays, n_gates]``; the variables named in ``per_sweep`` are float32
    ``[n_sweeps, n_gates]`` instead, one row for all ``rays_per_sweep`` rays of a sweep (temperature by range; default: the rays
    divided evenly among the rows).  A variable that is ``None`` or missing from the dict is absent at every gate -- allowed
    unless the table requires it.  NaN in a variable means absent at that gate.

    Per class the memberships of the present additive variables are averaged with the table's weights and multiplied by those of
    the present multiplicative ones; the largest score wins, the lowest class among equals.  ``classes`` is 0 where ``mask`` is
    non-zero, a required or the condition variable is absent, every score is 0 or the best is below ``min_score``.  One launch,
    no host synchronisation.  Returns :class:`FuzzyClasses`."""
    first, checked, rays_per_sweep = _check_variables(variables, table, per_sweep, rays_per_sweep)
    shape = tuple(int(n) for n in first.shape)
    _check_like(mask, first, "mask", None)
    min_score = _check_min_score(min_score)
    torch = _native.torch_mod()
    lib = _native.load_library()
    dev = _device_of(*(value for value, _ in checked), mask)
    m = None if mask is None else _to_device(mask, dev, torch.uint8)
    with torch.cuda.device(dev):
        tensors, bits = _stage_variables(torch, checked, shape, rays_per_sweep, dev)
        return _classify(lib, torch, tensors, bits, table, table.device_cells(dev), m, shape, rays_per_sweep, min_score, return_score,
                         return_second)


def beam_temperature(elevations_deg, ranges_m, heights_m, temperatures_c, radar_altitude: float = 0.0) -> np.ndarray:
    """The temperature along the beam of every sweep, float32 ``[n_sweeps, n_gates]``: the per-sweep table ``temperature`` of
    :func:`classify_hydrometeors_device`.  The beam height above sea level of every range (metres along the ground) is that of
    :func:`~radar_processor_amd.grid_products.compute_beam_height` (4/3 effective earth radius) for the sweep's elevation;
    the temperature there is ``np.interp`` through the sounding ``(heights_m, temperatures_c)``, heights above sea level in
    strictly ascending order -- constant beyond either end.  Host code in float64, rounded once; needs no device."""
    el = np.atleast_1d(np.asarray(elevations_deg, dtype=np.float64))
    r = np.asarray(ranges_m, dtype=np.float64)
    h = np.asarray(heights_m, dtype=np.float64)
    t = np.asarray(temperatures_c, dtype=np.float64)
    if el.ndim != 1 or el.size < 1 or not np.isfinite(el).all():
        raise ValueError(f"elevations_deg must be finite angles, one per sweep, got shape {list(el.shape)}")
    if r.ndim != 1 or not np.isfinite(r).all():
        raise ValueError(f"ranges_m must be a 1-D array of finite ranges, got shape {list(r.shape)}")
    if h.ndim != 1 or h.size < 1 or h.shape != t.shape or not (np.isfinite(h).all() and np.isfinite(t).all()):
        raise ValueError("heights_m and temperatures_c must be 1-D, finite, of one length and not empty")
    if (np.diff(h) <= 0).any():
        raise ValueError("heights_m must strictly ascend")
    altitude = _finite(radar_altitude, "radar_altitude")
    out = np.empty((el.size, r.size), np.float32)
    for s, angle in enumerate(el):
        out[s] = np.interp(compute_beam_height(r, float(angle), altitude), h, t)
    return out


def classify_hydrometeors_device(dbz, zdr, kdp, rhohv, *, phidp=None, temperature=None, rays_per_sweep: Optional[int] = None,
                                 table: Optional[MembershipTable] = None, mask=None, texture_half_gates: Tuple[int, int] = (2, 4),
                                 texture_min_valid: Tuple[Optional[int], Optional[int]] = (None, None),
                                 min_score: float = 0.0) -> HydrometeorClasses:
    """The chain on one volume: SD(Z) over ``texture_half_gates[0]`` gates on either side and SD(PHIDP) over
    ``texture_half_gates[1]`` (both under ``mask``), then the classifier over ``(Z, ZDR, KDP, RHOHV, SD(Z), SD(PHIDP), T)`` with
    ``table`` (default :data:`HYDROMETEOR_TABLE_S_BAND`; another table must name its variables :data:`HYDROMETEOR_VARIABLES`).
    ``dbz``, ``zdr``, ``kdp`` and ``rhohv`` are float32 ``[n_rays, n_gates]`` -- ``PhaseProducts.dbz``, ``.zdr`` and ``.kdp`` as
    they come; ``zdr`` and ``kdp`` may be ``None`` where the table does not require them.  ``phidp`` (optional) is the PHIDP
    whose texture is wanted: the UNFOLDED one (``PhaseProducts.phidp_unfolded``), a fold is a step of 360 degrees.
    ``temperature`` (optional) is float32 ``[n_sweeps, n_gates]`` in the table's unit (:func:`beam_temperature`), one row per
    ``rays_per_sweep`` rays.  Three launches on the current stream, nothing returns to the host.  Returns
    :class:`HydrometeorClasses`."""
    table = HYDROMETEOR_TABLE_S_BAND if table is None else table
    if not isinstance(table, MembershipTable) or table.variable_names != HYDROMETEOR_VARIABLES:
        raise ValueError(f"table must be a MembershipTable over the variables {HYDROMETEOR_VARIABLES!r}")
    shape = _check_field(dbz, "dbz")
    if not isinstance(texture_half_gates, (tuple, list)) or len(texture_half_gates) != 2:
        raise ValueError(f"texture_half_gates must be (half_gates of SD(Z), half_gates of SD(PHIDP)), not {texture_half_gates!r}")
    if not isinstance(texture_min_valid, (tuple, list)) or len(texture_min_valid) != 2:
        raise ValueError(f"texture_min_valid must be (min_valid of SD(Z), min_valid of SD(PHIDP)), not {texture_min_valid!r}")
    tex_z = _check_texture(texture_half_gates[0], texture_min_valid[0])
    tex_p = _check_texture(texture_half_gates[1], texture_min_valid[1])
    _check_like(phidp, dbz, "phidp")
    _check_like(mask, dbz, "mask", None)
    # the two textures stand in for themselves in the check: they have the shape and type of dbz
    given = [dbz, zdr, kdp, rhohv, dbz, None if phidp is None else dbz, temperature]
    _, checked, rays_per_sweep = _check_variables(given, table, ("T",), rays_per_sweep)
    min_score = _check_min_score(min_score)
    torch = _native.torch_mod()
    lib = _native.load_library()
    dev = _device_of(dbz, zdr, kdp, rhohv, phidp, temperature, mask)
    m = None if mask is None else _to_device(mask, dev, torch.uint8)
    with torch.cuda.device(dev):
        z = _to_device(dbz, dev)
        sd_z = _texture(lib, torch, z, m, shape, tex_z[0], tex_z[1], False, True, False, False).sd
        sd_p = None if phidp is None else _texture(lib, torch, _to_device(phidp, dev), m, shape, tex_p[0], tex_p[1], False, True,
                                                   False, False).sd
        checked[0], checked[4] = (z, False), (sd_z, False)
        checked[5] = (sd_p, False) if sd_p is not None else checked[5]
        tensors, bits = _stage_variables(torch, checked, shape, rays_per_sweep, dev)
        got = _classify(lib, torch, tensors, bits, table, table.device_cells(dev), m, shape, rays_per_sweep, min_score, True, True)
    return HydrometeorClasses(got.classes, got.score, got.second, sd_z, sd_p)


def classify_hydrometeors(dbz, zdr, kdp, rhohv, **kw) -> HydrometeorClasses:
    """:func:`classify_hydrometeors_device` for NumPy arrays: the fields are staged through device memory and every member of
    the :class:`HydrometeorClasses` comes back as an ndarray."""
    return HydrometeorClasses(*(None if o is None else o.cpu().numpy() for o in classify_hydrometeors_device(dbz, zdr, kdp, rhohv, **kw)))


def class_mask_device(classes, table: MembershipTable, names: Sequence[str]):
    """uint8 of the shape of ``classes`` (uint8, tensor or ndarray), on the device: 1 where the class is one of ``names``.  For
    ``("ground clutter", "biological")`` this is the ``mask`` of ``unfold_phidp_device`` and an entry of the gridders' ``masks``.
    A 256-entry table lookup in torch: bookkeeping on one byte per gate, not a kernel of this library."""
    if not isinstance(table, MembershipTable):
        raise ValueError(f"table must be a MembershipTable, not {type(table).__name__}")
    if isinstance(names, str):
        raise ValueError(f"names must be a sequence of class names, not the string {names!r}")
    values = [table.class_value(name) for name in names]
    if not hasattr(classes, "shape") or _dtype_name(classes) != "uint8":
        raise ValueError(f"classes must be a uint8 tensor or ndarray, got {_dtype_name(classes) if hasattr(classes, 'dtype') else type(classes).__name__}")
    torch = _native.torch_mod()
    dev = _device_of(classes)
    lut = np.zeros(256, np.uint8)
    lut[values] = 1
    with torch.cuda.device(dev):
        return _to_device(lut, dev)[_to_device(classes, dev).to(torch.int64)]


# ---- the preset --------------------------------------------------------------------------------------------------------------
_Z_EDGES = tuple(float(e) for e in range(5, 70, 5))               # 13 edges: below 5 dBZ, 5 dB bins up to 65, 65 dBZ and above
_INF = math.inf


def _kdp(l_kdp: float) -> float:
    """10 log10(KDP) -> KDP in deg/km; -30 (the published floor: KDP at or below 0.001) is an open shoulder, so that zero and
    negative KDP stay inside."""
    return -_INF if l_kdp <= -30.0 else 10.0 ** (l_kdp / 10.0)


def _s_band_vertices() -> np.ndarray:
    z_centres = np.array([2.5] + [e + 2.5 for e in _Z_EDGES], np.float64)
    out = np.zeros((len(z_centres), len(HYDROMETEOR_CLASSES), len(HYDROMETEOR_VARIABLES), 4), np.float64)
    everywhere = (-_INF, -_INF, _INF, _INF)
    weather_sd_z, weather_sd_p = (0.0, 0.5, 3.0, 6.0), (0.0, 1.0, 15.0, 30.0)
    for b, z in enumerate(z_centres):
        f1 = -0.50 + 2.50e-3 * z + 7.50e-4 * z * z
        f2 = 0.68 - 4.81e-2 * z + 2.92e-3 * z * z
        f3 = 1.42 + 6.67e-2 * z + 4.85e-4 * z * z
        g1, g2 = -44.0 + 0.8 * z, -22.0 + 0.5 * z
        drops_kdp = (_kdp(g1 - 1.0), _kdp(g1), _kdp(g2), _kdp(g2 + 1.0))
        any_kdp = (-_INF, -_INF, _kdp(10.0), _kdp(20.0))                 # the published -30, -25 flank lies below any KDP there is
        #          Z                         ZDR                             KDP                                       RHOHV
        #          SD(Z)                     SD(PHIDP)                       T (degrees Celsius)
        rows = [
            ((15.0, 20.0, 70.0, 80.0), (-4.0, -2.0, 1.0, 2.0), any_kdp, (0.5, 0.6, 0.9, 0.95),
             (2.0, 4.0, 10.0, 15.0), (30.0, 40.0, 50.0, 60.0), everywhere),                                        # ground clutter
            ((5.0, 10.0, 20.0, 30.0), (0.0, 2.0, 10.0, 12.0), (-_INF, -_INF, _kdp(10.0), _kdp(10.0)), (0.3, 0.5, 0.8, 0.83),
             (1.0, 2.0, 4.0, 7.0), (8.0, 10.0, 40.0, 60.0), (-10.0, -5.0, _INF, _INF)),                           # biological
            ((5.0, 10.0, 35.0, 40.0), (-0.3, 0.0, 0.3, 0.6), any_kdp, (0.95, 0.98, 1.0, 1.01),
             weather_sd_z, weather_sd_p, (-_INF, -_INF, -1.0, 2.0)),                                              # dry snow
            ((25.0, 30.0, 40.0, 50.0), (0.5, 1.0, 2.0, 3.0), any_kdp, (0.88, 0.92, 0.95, 0.985),
             weather_sd_z, weather_sd_p, (-2.5, -0.5, 2.5, 4.5)),                                                 # wet snow
            ((0.0, 5.0, 20.0, 25.0), (0.1, 0.4, 3.0, 3.3), (_kdp(-5.0), _kdp(0.0), _kdp(10.0), _kdp(15.0)), (0.95, 0.98, 1.0, 1.01),
             weather_sd_z, weather_sd_p, (-_INF, -_INF, -10.0, -5.0)),                                            # crystals
            ((25.0, 35.0, 50.0, 55.0), (-0.3, 0.0, f1, f1 + 0.3), any_kdp, (0.90, 0.97, 1.0, 1.01),
             weather_sd_z, weather_sd_p, (-_INF, -_INF, 0.0, 8.0)),                                               # graupel
            ((20.0, 25.0, 45.0, 50.0), (f2 - 0.3, f2, f3, f3 + 1.0), drops_kdp, (0.92, 0.95, 1.0, 1.01),
             weather_sd_z, weather_sd_p, (-2.0, 2.0, _INF, _INF)),                                                # big drops
            ((5.0, 10.0, 45.0, 50.0), (f1 - 0.3, f1, f2, f2 + 0.5), drops_kdp, (0.95, 0.97, 1.0, 1.01),
             weather_sd_z, weather_sd_p, (-2.0, 2.0, _INF, _INF)),                                                # rain
            ((40.0, 45.0, 55.0, 60.0), (f1 - 0.3, f1, f2, f2 + 0.5), drops_kdp, (0.92, 0.95, 1.0, 1.01),
             weather_sd_z, weather_sd_p, (-2.0, 2.0, _INF, _INF)),                                                # heavy rain
            ((45.0, 50.0, 75.0, 80.0), (-0.3, 0.0, f1, f1 + 0.5), (_kdp(-10.0), _kdp(-4.0), _kdp(g1), _kdp(g1 + 1.0)), (0.85, 0.9, 1.0, 1.01),
             weather_sd_z, weather_sd_p, everywhere),                                                             # rain and hail
        ]
        out[b] = np.array(rows, np.float64)
    # the published curves cross where they were never meant to be read (f1 < 0 below 24 dBZ, f2 > f3 above 53 dBZ): a vertex
    # never lies below the one before it
    return np.maximum.accumulate(out, axis=-1)


_S_BAND_WEIGHTS = (            # Z and T are multiplicative: their columns are not used
    # Z    ZDR  KDP  RHOHV SD(Z) SD(PHIDP) T
    (0.0, 0.4, 0.0, 1.0, 0.6, 0.8, 0.0),       # ground clutter
    (0.0, 0.6, 0.0, 1.0, 0.8, 0.8, 0.0),       # biological
    (0.0, 0.8, 0.0, 0.6, 0.2, 0.2, 0.0),       # dry snow
    (0.0, 0.8, 0.0, 1.0, 0.2, 0.2, 0.0),       # wet snow
    (0.0, 0.6, 0.5, 0.4, 0.2, 0.2, 0.0),       # crystals
    (0.0, 1.0, 0.0, 0.4, 0.2, 0.2, 0.0),       # graupel
    (0.0, 1.0, 0.0, 0.6, 0.2, 0.2, 0.0),       # big drops
    (0.0, 0.8, 0.0, 0.6, 0.2, 0.2, 0.0),       # rain
    (0.0, 0.8, 1.0, 0.6, 0.2, 0.2, 0.0),       # heavy rain
    (0.0, 0.8, 1.0, 0.6, 0.2, 0.2, 0.0),       # rain and hail
)

#: A PRESET, not a claim of parity: the ten classes of Park, Ryzhkov, Zrnic and Kim 2009 (Wea. Forecasting 24, 730-748) for S
#: band, with vertices that are THIS AUTHOR'S RENDERING of the published scheme.  The trapezoids of ZDR and KDP that the paper
#: gives as functions of Z are tabulated at the centre of 5 dB bins of Z (the condition variable); KDP is in deg/km, not
#: 10 log10; Z enters as a multiplicative gate instead of a weighted term, and the paper's melting-layer rules are replaced by
#: a multiplicative trapezoid of temperature in degrees Celsius (absent: no constraint).  Z, ZDR and RHOHV are required.
#: Parity with the WSR-88D HCA, wradlib's ``classify`` and CSU RadarTools is unpinned -- as ``ATTENUATION_COEFFICIENTS`` and
#: the Steiner relations of ``convection`` are presets from the literature, not reproductions of a package.
HYDROMETEOR_TABLE_S_BAND = MembershipTable(
    HYDROMETEOR_CLASSES, HYDROMETEOR_VARIABLES, _s_band_vertices(), _S_BAND_WEIGHTS,
    kinds=("multiplicative", "additive", "additive", "additive", "additive", "additive", "multiplicative"),
    required=("Z", "ZDR", "RHOHV"), condition="Z", edges=_Z_EDGES)
