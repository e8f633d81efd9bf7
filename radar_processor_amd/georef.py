"""Placing radars by latitude and longitude (csrc/rg_georef.hip).

A radar's gate coordinates (``get_gate_coordinates``) lie in the azimuthal-equidistant (AEQD) plane tangent at ITS antenna.
The mosaic functions take a radar as ``(gate_x, gate_y, gate_z, origin)`` and only translate it, but two AEQD planes
centred 200 km apart are not translations of each other: a gate 240 km north of the second radar lies 4.5 km from where
translation puts it.  This module produces the 4-tuple the mosaic functions should be given:

* :func:`place_radar` / :func:`place_radars` re-project every gate from the radar's plane into the plane of the shared
  grid on the device (``rg_gates_to_frame_f32``) and return ``(x', y', gate_z, (oz, oy, ox))`` with ``(ox, oy)`` the
  antenna's position in the grid's plane and ``x'``, ``y'`` relative to it -- exactly what every mosaic function takes;
* :func:`grid_lonlat_device` gives the longitude / latitude of a grid's nodes (``rg_frame_to_lonlat_f64``);
* :func:`geographic_to_grid` / :func:`grid_to_geographic` are the same maps in host NumPy float64 for a handful of points
  (vertices, corners, radar positions), and :func:`section_path_lonlat` a section path given by geographic vertices.

The projection is the spherical AEQD of PyART's ``pyart_aeqd`` (``processor_seam.py`` names it in its packages): a sphere
of radius :data:`AEQD_EARTH_RADIUS` = 6370997 m, restated from the textbook formulas (``include/radargrid_hip.h``,
``rg_georef``).  PyART is not in the tree, so parity with it is UNPINNED, as for the antenna transform; the tests pin the
maps against a 40-digit evaluation of the same formulas.  An ellipsoidal AEQD (what the reference's ``geotiff.py`` asks
pyproj for) differs from the sphere and is not offered.

Angles are degrees at the interface and float64 radians inside; every step runs in float64 and the result is rounded once.
``gate_z`` is a height above the antenna and is not touched.
"""
from __future__ import annotations

import math
from typing import List, Optional, Sequence, Tuple

import numpy as np

from . import _native
from .geometry_builder import _as_device_f32
from .radar_adaptors import get_gate_coordinates
from .section import _length, section_path

AEQD_EARTH_RADIUS = 6370997.0          # PyART's pyart_aeqd sphere, metres
MAX_ANGULAR_DISTANCE = math.pi / 2.0 - 0.1     # radians from the origin beyond which a position is refused


def _check_radius(R) -> float:
    R = float(R)
    if not (math.isfinite(R) and R > 0.0):
        raise ValueError(f"R must be finite and positive, not {R}")
    return R


def _check_lonlat(lon, lat, what: str) -> Tuple[np.ndarray, np.ndarray]:
    lon, lat = np.asarray(lon, dtype=np.float64), np.asarray(lat, dtype=np.float64)
    if not (np.all(np.isfinite(lon)) and np.all(np.isfinite(lat))):
        raise ValueError(f"{what}: longitude and latitude must be finite")
    if np.any(np.abs(lat) > 90.0):
        raise ValueError(f"{what}: latitude outside [-90, 90]")
    return lon, lat


def _position(p, what: str, altitude: bool) -> Tuple[float, float, float]:
    """``(lon, lat[, alt])`` -> three checked floats (alt 0.0 where the position has none and none is needed)."""
    try:
        p = tuple(float(v) for v in p)
    except TypeError:
        raise ValueError(f"{what} must be (lon, lat, alt), got {p!r}") from None
    if len(p) not in ((3,) if altitude else (2, 3)):
        raise ValueError(f"{what} must be {'(lon, lat, alt)' if altitude else '(lon, lat) or (lon, lat, alt)'}, got {p!r}")
    if not all(math.isfinite(v) for v in p):
        raise ValueError(f"{what} must be finite, got {p!r}")
    _check_lonlat(p[0], p[1], what)
    return p[0], p[1], (p[2] if len(p) == 3 else 0.0)


def _forward(lon, lat, lon0, lat0, R):
    """AEQD forward map, float64 radians in, ``(x, y, c)`` out (``c``: angular distance from the centre)."""
    d = lon - lon0
    sp, cp, sd, cd = np.sin(lat), np.cos(lat), np.sin(d), np.cos(d)
    s0, c0 = np.sin(lat0), np.cos(lat0)
    a = cp * sd
    b = c0 * sp - s0 * cp * cd
    q = s0 * sp + c0 * cp * cd
    s = np.hypot(a, b)
    c = np.arctan2(s, q)             # not arccos(q): that loses half the digits near the centre
    with np.errstate(invalid="ignore", divide="ignore"):
        k = np.where(s == 0.0, 1.0, c / np.where(s == 0.0, 1.0, s))
    return R * k * a, R * k * b, c


def geographic_to_grid(lon, lat, origin_lon, origin_lat, R: float = AEQD_EARTH_RADIUS) -> Tuple[np.ndarray, np.ndarray]:
    """Longitude / latitude (degrees, scalars or arrays) -> ``(x, y)`` float64 metres in the AEQD plane tangent at
    ``(origin_lon, origin_lat)``.  Host NumPy, no device.  ``ValueError`` for a non-finite value, a latitude outside
    [-90, 90], a bad ``R``, or a point ``pi/2 - 0.1`` rad or more from the origin (the plane is meaningless there)."""
    R = _check_radius(R)
    lon, lat = _check_lonlat(lon, lat, "geographic_to_grid")
    lon0, lat0 = _check_lonlat(origin_lon, origin_lat, "geographic_to_grid: origin")
    if lon0.ndim or lat0.ndim:
        raise ValueError("geographic_to_grid: the origin is one point")
    x, y, c = _forward(np.radians(lon), np.radians(lat), float(np.radians(lon0)), float(np.radians(lat0)), R)
    if np.any(c >= MAX_ANGULAR_DISTANCE):
        raise ValueError(f"geographic_to_grid: a point lies {float(np.max(c)):.3f} rad from the origin; the limit is "
                         f"pi/2 - 0.1 = {MAX_ANGULAR_DISTANCE:.3f}")
    return x, y


def grid_to_geographic(x, y, origin_lon, origin_lat, R: float = AEQD_EARTH_RADIUS) -> Tuple[np.ndarray, np.ndarray]:
    """``(x, y)`` metres in the AEQD plane tangent at ``(origin_lon, origin_lat)`` -> ``(lon, lat)`` float64 degrees,
    ``lon`` in [-180, 180).  Host NumPy, no device.  Non-finite coordinates give NaN; beyond ``pi * R`` the plane wraps."""
    R = _check_radius(R)
    lon0, lat0 = _check_lonlat(origin_lon, origin_lat, "grid_to_geographic: origin")
    if lon0.ndim or lat0.ndim:
        raise ValueError("grid_to_geographic: the origin is one point")
    x, y = np.broadcast_arrays(np.asarray(x, dtype=np.float64), np.asarray(y, dtype=np.float64))
    lam0, phi0 = float(np.radians(lon0)), float(np.radians(lat0))
    rho = np.hypot(x, y)
    c = rho / R
    sc, cc = np.sin(c), np.cos(c)
    safe = np.where(rho == 0.0, 1.0, rho)
    with np.errstate(invalid="ignore"):
        lat = np.arcsin(np.clip(cc * math.sin(phi0) + y * sc * math.cos(phi0) / safe, -1.0, 1.0))
        lon = lam0 + np.arctan2(x * sc, rho * math.cos(phi0) * cc - y * math.sin(phi0) * sc)
    lat = np.where(rho == 0.0, phi0, lat)
    lon = np.degrees(np.where(rho == 0.0, lam0, lon))
    with np.errstate(invalid="ignore"):
        lon = lon - 360.0 * np.floor((lon + 180.0) / 360.0)
        lon = np.where(lon >= 180.0, lon - 360.0, lon)
    return lon, np.degrees(lat)


def make_georef(from_lonlat, to_lonlat, R: float = AEQD_EARTH_RADIUS) -> "_native.Georef":
    """The ``rg_georef`` of a re-projection from the plane about ``from_lonlat`` into the plane about ``to_lonlat``
    (degrees; an altitude, if given, is ignored): every constant the kernels need, in host float64.  Raises ``ValueError``
    as :func:`geographic_to_grid` does; touches no device."""
    R = _check_radius(R)
    lon_f, lat_f, _ = _position(from_lonlat, "the radar's position", altitude=False)
    lon_t, lat_t, _ = _position(to_lonlat, "the grid origin", altitude=False)
    same = lon_f == lon_t and lat_f == lat_t
    ox = oy = 0.0
    if not same:
        x, y = geographic_to_grid(lon_f, lat_f, lon_t, lat_t, R)
        ox, oy = float(x), float(y)
    phi_f, phi_t = float(np.radians(lat_f)), float(np.radians(lat_t))
    # sines and cosines by NumPy, like every other step of the host maps
    return _native.Georef(radius=R, lon_from=float(np.radians(lon_f)), lat_from=phi_f, sin_lat_from=float(np.sin(phi_f)),
                          cos_lat_from=float(np.cos(phi_f)), lon_to=float(np.radians(lon_t)), lat_to=phi_t,
                          sin_lat_to=float(np.sin(phi_t)), cos_lat_to=float(np.cos(phi_t)), ox=ox, oy=oy,
                          same_centre=int(same), reserved=0)


def place_gates_device(gate_x, gate_y, radar_lonlat, origin_lonlat, R: float = AEQD_EARTH_RADIUS, device=None, out=None):
    """Re-project a radar's gates on the device: ``gate_x``, ``gate_y`` (NumPy arrays or tensors, float32 metres in the AEQD
    plane at ``radar_lonlat``) -> two float32 device tensors ``(x', y')``: the gates in the plane at ``origin_lonlat``,
    relative to the antenna's position there (``rg_gates_to_frame_f32``).  With both positions exactly equal the
    coordinates are copied bit for bit; a gate whose x or y is not finite comes out NaN in both.

    ``out=(x_out, y_out)``: contiguous float32 tensors of the gates' length on the device to write into -- they may be
    the input tensors themselves (in place).  Every argument is validated before the device is touched."""
    georef = make_georef(radar_lonlat, origin_lonlat, R)
    n = _length(gate_x)
    if _length(gate_y) != n:
        raise ValueError(f"gate_x and gate_y differ in length ({n} and {_length(gate_y)})")
    if out is not None and (len(out) != 2 or _length(out[0]) != n or _length(out[1]) != n):
        raise ValueError(f"out must be two tensors of {n} elements")
    torch = _native.torch_mod()
    lib = _native.load_library()
    dev = _native.canonical_device(device)
    gx, gy = _as_device_f32(gate_x, dev), _as_device_f32(gate_y, dev)
    if out is None:
        out = (torch.empty_like(gx), torch.empty_like(gy))
    for t in out:
        if not (t.is_cuda and t.device == dev and t.dtype == torch.float32 and t.is_contiguous()):
            raise ValueError(f"out: expected contiguous cuda float32 tensors on {dev}")
    with torch.cuda.device(dev):
        _native.check(lib.rg_gates_to_frame_f32(_native.ptr(gx), _native.ptr(gy), n, georef, _native.ptr(out[0]),
                                                _native.ptr(out[1]), _native.stream_ptr()), "rg_gates_to_frame_f32")
    return out[0].view(-1), out[1].view(-1)


def place_radar(gate_x, gate_y, gate_z, radar_position, grid_origin, R: float = AEQD_EARTH_RADIUS, device=None):
    """One radar of a mosaic, placed by where it stands: ``radar_position`` and ``grid_origin`` are ``(lon, lat, alt)``
    (degrees, metres).  Returns ``(x', y', gate_z, (oz, oy, ox))`` -- ``x'``, ``y'`` float32 device tensors
    (:func:`place_gates_device`), ``gate_z`` the object passed in (a height above the antenna: untouched), ``(ox, oy)`` the
    antenna in the grid's plane (host float64) and ``oz = alt_radar - alt_origin``.  A radar standing exactly at the
    origin's longitude and latitude keeps its coordinates bit for bit and ``ox = oy = 0.0``."""
    lon_r, lat_r, alt_r = _position(radar_position, "radar_position", altitude=True)
    lon_0, lat_0, alt_0 = _position(grid_origin, "grid_origin", altitude=True)
    georef = make_georef((lon_r, lat_r), (lon_0, lat_0), R)         # every refusal, before any device work
    if _length(gate_z) != _length(gate_x):
        raise ValueError("gate_x, gate_y and gate_z differ in length")
    x, y = place_gates_device(gate_x, gate_y, (lon_r, lat_r), (lon_0, lat_0), R, device)
    return x, y, gate_z, (alt_r - alt_0, georef.oy, georef.ox)


def place_radars(radars: Sequence, grid_origin, R: float = AEQD_EARTH_RADIUS, device=None) -> List[tuple]:
    """(Duck-typed) PyART radars -> the list of placed 4-tuples for ``MosaicSearch`` / ``compute_mosaic_geometry``: each
    radar's ``get_gate_coordinates`` and ``longitude / latitude / altitude['data'][0]`` through :func:`place_radar`."""
    placed = []
    for radar in radars:
        position = tuple(float(getattr(radar, name)["data"][0]) for name in ("longitude", "latitude", "altitude"))
        placed.append(place_radar(*get_gate_coordinates(radar), position, grid_origin, R, device))
    return placed


def section_path_lonlat(vertices_lonlat, spacing: float, grid_origin, R: float = AEQD_EARTH_RADIUS):
    """:func:`section_path` along a polyline given by geographic vertices ``[(lon, lat), ...]``: the vertices are mapped
    into the plane of ``grid_origin`` (``(lon, lat)`` or ``(lon, lat, alt)``) and the path is sampled THERE, every
    ``spacing`` metres.  Each leg is straight in the grid's plane, not a geodesic (the two differ except through the
    origin).  Returns ``(xs float32, ys float32, s float64)``."""
    lon0, lat0, _ = _position(grid_origin, "grid_origin", altitude=False)
    v = np.asarray(vertices_lonlat, dtype=np.float64)
    if v.ndim != 2 or v.shape[1] != 2 or v.shape[0] < 2:
        raise ValueError("vertices_lonlat must be at least two (lon, lat) pairs")
    x, y = geographic_to_grid(v[:, 0], v[:, 1], lon0, lat0, R)
    return section_path(np.stack([x, y], axis=1), spacing)


def grid_lonlat_device(grid_shape, grid_limits, grid_origin, R: float = AEQD_EARTH_RADIUS, device=None):
    """Longitude and latitude of every column of a grid whose plane is tangent at ``grid_origin`` (``(lon, lat)`` or
    ``(lon, lat, alt)``): two float64 ``[ny, nx]`` device tensors in degrees, ``lon`` in [-180, 180)
    (``rg_frame_to_lonlat_f64``).  The nodes are those of the gridders: ``np.linspace(..., dtype='float32')`` of
    ``grid_limits`` (z, y, x order)."""
    georef = make_georef(grid_origin, grid_origin, R)
    shape = tuple(int(s) for s in grid_shape)
    if len(shape) != 3 or min(shape) < 1:
        raise ValueError(f"bad grid shape {grid_shape}")
    _, ny, nx = shape
    yc = np.linspace(grid_limits[1][0], grid_limits[1][1], ny, dtype="float32")
    xc = np.linspace(grid_limits[2][0], grid_limits[2][1], nx, dtype="float32")
    torch = _native.torch_mod()
    lib = _native.load_library()
    dev = _native.canonical_device(device)
    yc_t, xc_t = torch.from_numpy(yc).to(dev), torch.from_numpy(xc).to(dev)
    lon = torch.empty((ny, nx), dtype=torch.float64, device=dev)
    lat = torch.empty((ny, nx), dtype=torch.float64, device=dev)
    with torch.cuda.device(dev):
        _native.check(lib.rg_frame_to_lonlat_f64(_native.ptr(xc_t), _native.ptr(yc_t), ny, nx, georef, _native.ptr(lon),
                                                 _native.ptr(lat), _native.stream_ptr()), "rg_frame_to_lonlat_f64")
    return lon, lat
