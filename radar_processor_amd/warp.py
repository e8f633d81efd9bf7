"""Onto a web map (csrc/rg_warp.hip): a product plane, or its RGBA image, resampled north-up into a Web Mercator
(EPSG:3857) raster, and the overview pyramid of the result -- without leaving the device.

Everything up to ``colormap_rgba_device`` lies in the grid's own azimuthal-equidistant (AEQD) plane.  The reference then shells
out to ``gdalwarp`` (``radar_processor/processor.py:229-303``) and lets rasterio build the overviews (``:306-420``); its
``radar_grid/geotiff.py:238-291`` does not resample at all.  Here:

* :class:`MercatorRaster` names a north-up raster; :func:`mercator_raster_for` is the one that covers a grid,
  :func:`mercator_tile` the one of an XYZ map tile;
* :func:`warp_to_mercator_device` resamples float32 planes (nearest or bilinear) or an RGBA image (nearest) into one;
* :func:`overview_pyramid_device` builds overview levels, every level from the base image;
* :func:`web_mercator_rgba` chains warp, ``colormap_rgba_device`` and the pyramid;
* :func:`lonlat_to_mercator` / :func:`mercator_to_lonlat` are the spherical Mercator maps in host NumPy float64.

Longitude and latitude are carried UNCHANGED from the grid's 6370997 m sphere (``georef.AEQD_EARTH_RADIUS``) to the
6378137 m sphere of EPSG:3857, which is what a PROJ pipeline with no datum shift does.  GDAL, pyproj and rasterio are not in
the tree, so parity with ``gdalwarp`` is UNPINNED; the tests pin the pixel map (``include/radargrid_hip.h``,
``rg_mercator_raster``) against a 40-digit evaluation of its formulas.

``grid_shape`` and ``grid_limits`` are the gridders' ``(nz, ny, nx)`` and ``((z0, z1), (y0, y1), (x0, x1))``; only their last
two entries are read, so ``(ny, nx)`` and ``((y0, y1), (x0, x1))`` do as well.  Every argument is validated before the device
is touched.
"""
from __future__ import annotations

import math
from typing import List, NamedTuple, Optional, Tuple

import numpy as np

from . import _native
from .georef import AEQD_EARTH_RADIUS, _check_radius, _position, grid_to_geographic, make_georef

MERCATOR_RADIUS = 6378137.0                      # the EPSG:3857 sphere, metres
_HALF_WORLD = math.pi * MERCATOR_RADIUS
WARP_METHODS = {"nearest": 0, "bilinear": 1}
OVERVIEW_RESAMPLINGS = {"nearest": 0, "average": 1}
# the names radar_processor/processor.py:204-216 accepts
_REFERENCE_RESAMPLINGS = ("nearest", "bilinear", "cubic", "average", "mode", "max", "min", "med", "q1", "q3", "rms")
DEFAULT_OVERVIEW_FACTORS = [2, 4, 8, 16]
EDGE_SAMPLES = 257                               # points per edge of a grid's outline (mercator_raster_for)


class MercatorRaster(NamedTuple):
    """A north-up Web Mercator raster of square pixels: row 0 is the northernmost row, the centre of pixel ``(r, c)`` is
    ``(x_min + (c + 0.5) * pixel, y_max - (r + 0.5) * pixel)``.  ``x_min`` may lie beyond ``+-pi * MERCATOR_RADIUS``."""
    x_min: float
    y_max: float
    pixel: float
    width: int
    height: int

    @property
    def bounds(self) -> Tuple[float, float, float, float]:
        """``(west, south, east, north)``, metres."""
        return (self.x_min, self.y_max - self.height * self.pixel, self.x_min + self.width * self.pixel, self.y_max)

    @property
    def transform(self) -> Tuple[float, float, float, float, float, float]:
        """GDAL's six coefficients ``(x_min, pixel, 0, y_max, 0, -pixel)``."""
        return (self.x_min, self.pixel, 0.0, self.y_max, 0.0, -self.pixel)


def _check_raster(raster) -> MercatorRaster:
    try:
        x_min, y_max, pixel, width, height = raster
    except (TypeError, ValueError):
        raise ValueError(f"raster must be a MercatorRaster(x_min, y_max, pixel, width, height), got {raster!r}") from None
    x_min, y_max, pixel = float(x_min), float(y_max), float(pixel)
    if not (math.isfinite(x_min) and math.isfinite(y_max) and math.isfinite(pixel) and pixel > 0.0):
        raise ValueError(f"raster: x_min and y_max must be finite and pixel finite and positive, got {raster!r}")
    if width != int(width) or height != int(height) or width < 0 or height < 0 or max(width, height) >= 2 ** 31:
        raise ValueError(f"raster: width and height must be integers in 0 .. 2^31 - 1, got {width!r} and {height!r}")
    return MercatorRaster(x_min, y_max, pixel, int(width), int(height))


def lonlat_to_mercator(lon, lat) -> Tuple[np.ndarray, np.ndarray]:
    """Longitude / latitude in degrees -> EPSG:3857 ``(x, y)`` float64 metres (host NumPy).  ``|lat| = 90`` gives
    ``+-inf``; a longitude outside [-180, 180) is not wrapped."""
    lon, lat = np.asarray(lon, dtype=np.float64), np.asarray(lat, dtype=np.float64)
    with np.errstate(divide="ignore"):
        return MERCATOR_RADIUS * np.radians(lon), MERCATOR_RADIUS * np.arctanh(np.sin(np.radians(lat)))


def mercator_to_lonlat(x, y) -> Tuple[np.ndarray, np.ndarray]:
    """EPSG:3857 ``(x, y)`` metres -> longitude / latitude in float64 degrees (host NumPy); ``x`` is not wrapped."""
    x, y = np.asarray(x, dtype=np.float64), np.asarray(y, dtype=np.float64)
    return np.degrees(x / MERCATOR_RADIUS), np.degrees(np.arctan(np.sinh(y / MERCATOR_RADIUS)))


def _lattice(grid_shape, grid_limits) -> "_native.WarpSource":
    """The float64 node lattice of a plane: the ``rg_warp_source`` of ``(ny, nx)`` nodes between the y and x limits."""
    try:
        ny, nx = (int(n) for n in tuple(grid_shape)[-2:])
        (y_lo, y_hi), (x_lo, x_hi) = ((float(lo), float(hi)) for lo, hi in tuple(grid_limits)[-2:])
    except (TypeError, ValueError):
        raise ValueError(f"bad grid shape {grid_shape!r} or limits {grid_limits!r}") from None
    if ny < 2 or nx < 2:
        raise ValueError(f"a plane to warp needs at least 2 x 2 nodes, not {ny} x {nx}")
    if not all(math.isfinite(v) for v in (y_lo, y_hi, x_lo, x_hi)) or y_hi <= y_lo or x_hi <= x_lo:
        raise ValueError(f"grid limits must be finite and increasing, got {grid_limits!r}")
    return _native.WarpSource(x_lo=x_lo, y_lo=y_lo, step_x=(x_hi - x_lo) / (nx - 1), step_y=(y_hi - y_lo) / (ny - 1), ny=ny,
                              nx=nx)


def mercator_raster_for(grid_shape, grid_limits, grid_origin, pixel_size: Optional[float] = None,
                        R: float = AEQD_EARTH_RADIUS) -> MercatorRaster:
    """The raster that covers a grid whose plane is tangent at ``grid_origin`` (``(lon, lat)`` or ``(lon, lat, alt)``).

    The outline of the grid's cell footprint -- its limits widened by half a step -- is sampled at :data:`EDGE_SAMPLES`
    points per edge and mapped through :func:`grid_to_geographic`; the raster is the bounding box of those points.
    Longitudes are taken relative to the origin's, so a grid across the antimeridian gets ONE connected raster (whose
    ``x_min`` or east edge then lies beyond ``+-pi * MERCATOR_RADIUS``).  ``pixel_size`` defaults to
    ``min(step_x, step_y) / cos(lat_origin)``, the Mercator size of a grid step at the origin; ``width`` and ``height`` are
    the ceilings of extent over pixel.  Host NumPy; raises ``ValueError`` for what cannot be a grid or a raster."""
    R = _check_radius(R)
    lon0, lat0, _ = _position(grid_origin, "grid_origin", altitude=False)
    s = _lattice(grid_shape, grid_limits)
    if pixel_size is None:
        pixel_size = min(s.step_x, s.step_y) / math.cos(math.radians(lat0))
    pixel = float(pixel_size)
    if not (math.isfinite(pixel) and pixel > 0.0):
        raise ValueError(f"pixel_size must be finite and positive, not {pixel_size!r}")
    west, east = s.x_lo - 0.5 * s.step_x, s.x_lo + (s.nx - 0.5) * s.step_x
    south, north = s.y_lo - 0.5 * s.step_y, s.y_lo + (s.ny - 0.5) * s.step_y
    for pole_y in (R * (math.pi / 2.0 - math.radians(lat0)), -R * (math.pi / 2.0 + math.radians(lat0))):
        if west <= 0.0 <= east and south <= pole_y <= north:
            raise ValueError("the grid holds a pole: it has no Web Mercator raster")
    ex, ey = np.linspace(west, east, EDGE_SAMPLES), np.linspace(south, north, EDGE_SAMPLES)
    x = np.concatenate([ex, ex, np.full_like(ey, west), np.full_like(ey, east)])
    y = np.concatenate([np.full_like(ex, south), np.full_like(ex, north), ey, ey])
    lon, lat = grid_to_geographic(x, y, lon0, lat0, R)
    lon = lon0 + ((lon - lon0 + 180.0) % 360.0 - 180.0)                  # within 180 degrees of the origin's
    mx, my = lonlat_to_mercator(lon, lat)
    if not (np.all(np.isfinite(mx)) and np.all(np.isfinite(my))):
        raise ValueError("the grid reaches a pole: it has no Web Mercator raster")
    x_min, y_max = float(mx.min()), float(my.max())
    width, height = math.ceil((float(mx.max()) - x_min) / pixel), math.ceil((y_max - float(my.min())) / pixel)
    return _check_raster(MercatorRaster(x_min, y_max, pixel, max(width, 1), max(height, 1)))


def mercator_tile(z: int, x: int, y: int, size: int = 256) -> MercatorRaster:
    """The raster of XYZ map tile ``(z, x, y)`` (``y`` grows southwards, as tile servers count) at ``size`` x ``size``
    pixels.  ``ValueError`` unless ``0 <= z <= 30``, ``0 <= x, y < 2**z`` and ``size >= 1``.  Tile edges are
    ``2 * pi * a * (i / 2**z - 1/2)``, rounded once: a tile and its four children share them exactly."""
    if any(v != int(v) for v in (z, x, y, size)):
        raise ValueError(f"z, x, y and size must be integers, got {(z, x, y, size)!r}")
    z, x, y, size = int(z), int(x), int(y), int(size)
    if not 0 <= z <= 30:
        raise ValueError(f"zoom level {z} outside 0 .. 30")
    n = 1 << z
    if not (0 <= x < n and 0 <= y < n):
        raise ValueError(f"tile ({x}, {y}) outside 0 .. {n - 1} at zoom {z}")
    if not 1 <= size < 2 ** 31:
        raise ValueError(f"size must be a positive int32, not {size}")
    world = 2.0 * _HALF_WORLD
    return MercatorRaster(world * (x / n - 0.5), world * (0.5 - y / n), world / n / size, size, size)


# ---- device --------------------------------------------------------------------------------------------------------------
def _is_tensor(a) -> bool:
    return type(a).__module__.startswith("torch")


def _image_kind(a, what: str) -> Tuple[str, tuple]:
    """``("f32", (P, h, w))`` or ``("rgba", (h, w))`` of a tensor / ndarray, checked by dtype and rank only."""
    shape = tuple(int(n) for n in a.shape)
    dtype = str(a.dtype).replace("torch.", "")
    if dtype == "float32" and len(shape) in (2, 3):
        if len(shape) == 3 and shape[0] < 1:
            raise ValueError(f"{what}: no planes in shape {shape}")
        return "f32", ((1,) + shape if len(shape) == 2 else shape)
    if dtype == "uint8" and len(shape) == 3 and shape[2] == 4:
        return "rgba", shape[:2]
    raise ValueError(f"{what} must be float32 [h, w] or [P, h, w], or uint8 [h, w, 4]; got {dtype} {list(shape)}")


def _to_device(a, dev):
    torch = _native.torch_mod()
    if _is_tensor(a):
        return a.to(dev).contiguous()
    return torch.from_numpy(np.ascontiguousarray(a)).to(dev)


def _device_of(a, device):
    if device is None and _is_tensor(a) and a.is_cuda:
        return a.device
    return _native.canonical_device(device)


def warp_to_mercator_device(data, grid_limits, grid_origin, raster, method: str = "nearest", fill_value: float = float("nan"),
                            R: float = AEQD_EARTH_RADIUS, device=None, out=None):
    """Resample ``data`` -- planes on the nodes of a grid tangent at ``grid_origin`` -- into ``raster`` on the device.

    ``data``: float32 ``[ny, nx]`` or ``[P, ny, nx]`` (``rg_warp_mercator_f32``; all planes share one coordinate evaluation
    per pixel), or uint8 ``[ny, nx, 4]`` (``rg_warp_mercator_rgba8``), tensor or ndarray; row ``iy`` grows northwards.  The
    result has the matching rank: ``[height, width]``, ``[P, height, width]`` or ``[height, width, 4]``, row 0 in the north.

    ``method``: ``"nearest"`` copies the nearest node's value bit for bit; ``"bilinear"`` weights the four surrounding
    nodes, skips the NaN ones and keeps the pixel only while the present weights sum to at least 0.5 (an echo's edge stays
    where nearest keeps it).  Pixels outside the grid, or ``pi/2 - 0.1`` rad or more from its origin, get ``fill_value``
    (float32) or ``0, 0, 0, 0`` (uint8, nearest only: bilinear on uint8 is a ``ValueError``).  ``out``: a contiguous tensor of
    the result's shape and dtype on the device to write into."""
    georef = make_georef(grid_origin, grid_origin, R)
    raster = _check_raster(raster)
    if method not in WARP_METHODS:
        raise ValueError(f"method must be one of {sorted(WARP_METHODS)}, not {method!r}")
    kind, shape = _image_kind(data, "data")
    if kind == "rgba" and method != "nearest":
        raise ValueError("a uint8 RGBA image is warped with method='nearest' only")
    source = _lattice(shape[-2:], grid_limits)
    fill = float(fill_value)
    planes = shape[0] if kind == "f32" else 1
    if kind == "rgba":
        out_shape = (raster.height, raster.width, 4)
    else:
        out_shape = (raster.height, raster.width) if len(data.shape) == 2 else (planes, raster.height, raster.width)
    if out is not None and (not _is_tensor(out) or tuple(out.shape) != out_shape):
        raise ValueError(f"out must be a tensor of shape {out_shape}")
    torch = _native.torch_mod()
    lib = _native.load_library()
    dev = _device_of(data, device)
    src = _to_device(data, dev)
    dtype = torch.uint8 if kind == "rgba" else torch.float32
    if out is None:
        out = torch.empty(out_shape, dtype=dtype, device=dev)
    elif not (out.is_cuda and out.device == dev and out.dtype == dtype and out.is_contiguous()):
        raise ValueError(f"out: expected a contiguous cuda {dtype} tensor on {dev}")
    c_raster = _native.MercatorRaster(*raster)
    with torch.cuda.device(dev):
        if kind == "rgba":
            _native.check(lib.rg_warp_mercator_rgba8(_native.ptr(src), source, georef, c_raster, _native.ptr(out),
                                                     _native.stream_ptr()), "rg_warp_mercator_rgba8")
        else:
            _native.check(lib.rg_warp_mercator_f32(_native.ptr(src), planes, source, georef, c_raster, WARP_METHODS[method],
                                                   fill, _native.ptr(out), _native.stream_ptr()), "rg_warp_mercator_f32")
    return out


def _check_pyramid(factors, resampling) -> Tuple[List[int], str]:
    if factors is None:
        factors = DEFAULT_OVERVIEW_FACTORS
    if not isinstance(factors, list):
        raise TypeError(f"factors must be a list or None, got {type(factors).__name__}")
    if not isinstance(resampling, str):
        raise TypeError(f"resampling must be a string, got {type(resampling).__name__}")
    name = resampling.lower().strip()
    if name not in OVERVIEW_RESAMPLINGS:
        known = "" if name in _REFERENCE_RESAMPLINGS else "unknown "
        raise ValueError(f"{known}resampling {resampling!r}: this build implements {', '.join(sorted(OVERVIEW_RESAMPLINGS))}")
    for f in factors:
        if isinstance(f, bool) or f != int(f) or not 2 <= f <= 64:
            raise ValueError(f"an overview factor must be an integer in 2 .. 64, not {f!r}")
    return [int(f) for f in factors], name


def overview_pyramid_device(image, factors: Optional[list] = None, resampling: str = "nearest", device=None) -> list:
    """Overview levels of ``image`` (float32 ``[h, w]`` / ``[P, h, w]`` or uint8 ``[h, w, 4]``, tensor or ndarray): a list
    with one device tensor ``[.., ceil(h / f), ceil(w / f) ..]`` per factor, each computed from ``image`` itself
    (``rg_overview_f32`` / ``rg_overview_rgba8``).  ``factors``: a list of integers in 2 .. 64; ``None`` means
    ``[2, 4, 8, 16]`` and ``[]`` gives ``[]`` (``convert_to_cog``'s ``overview_factors``; a non-list is a ``TypeError``).

    ``resampling``: ``"nearest"`` takes the pixel at the middle of each block, bit for bit; ``"average"`` the mean of the
    block's finite values, accumulated in float64 (NaN where there is none) -- float32 only.  The other names the reference
    passes on to rasterio are refused with a ``ValueError``."""
    factors, name = _check_pyramid(factors, resampling)
    kind, shape = _image_kind(image, "image")
    if kind == "rgba" and name != "nearest":
        raise ValueError("a uint8 RGBA image takes resampling='nearest' only")
    if not factors:
        return []
    torch = _native.torch_mod()
    lib = _native.load_library()
    dev = _device_of(image, device)
    src = _to_device(image, dev)
    h, w = shape[-2:]
    levels = []
    with torch.cuda.device(dev):
        for f in factors:
            oh, ow = -(-h // f), -(-w // f)
            if kind == "rgba":
                out = torch.empty((oh, ow, 4), dtype=torch.uint8, device=dev)
                _native.check(lib.rg_overview_rgba8(_native.ptr(src), h, w, f, _native.ptr(out), _native.stream_ptr()),
                              "rg_overview_rgba8")
            else:
                out = torch.empty((oh, ow) if len(image.shape) == 2 else (shape[0], oh, ow), dtype=torch.float32, device=dev)
                _native.check(lib.rg_overview_f32(_native.ptr(src), shape[0], h, w, f, OVERVIEW_RESAMPLINGS[name],
                                                  _native.ptr(out), _native.stream_ptr()), "rg_overview_f32")
            levels.append(out)
    return levels


def web_mercator_rgba(plane, grid_limits, grid_origin, lut, vmin: float, vmax: float, raster=None, method: str = "nearest",
                      factors: Optional[list] = None, resampling: str = "nearest", R: float = AEQD_EARTH_RADIUS, device=None):
    """A float32 product plane ``[ny, nx]`` -> ``(raster, rgba, [overview rgba, ...])`` for a web map, on the device: the
    plane is warped (:func:`warp_to_mercator_device`, NaN fill), coloured through ``colormap_rgba_device(.., lut, vmin,
    vmax)`` and given its overviews (:func:`overview_pyramid_device`).  ``raster=None`` takes
    :func:`mercator_raster_for` of the plane.  With ``resampling="nearest"`` the overviews are levels of the RGBA image;
    with ``"average"`` they are levels of the warped FLOAT plane, each coloured afterwards (colours are not averaged).
    ``lut`` is the table of ``colormap_lut``."""
    from .raster import colormap_rgba_device
    factors, resampling = _check_pyramid(factors, resampling)
    kind, shape = _image_kind(plane, "plane")
    if kind != "f32" or len(plane.shape) != 2:
        raise ValueError("plane must be one float32 [ny, nx] plane")
    vmin, vmax = float(vmin), float(vmax)
    if not vmin <= vmax:
        raise ValueError("vmin must be less than or equal to vmax")
    lut = np.ascontiguousarray(lut, dtype=np.uint8) if not _is_tensor(lut) else lut
    if len(lut.shape) != 2 or lut.shape[1] != 4 or lut.shape[0] < 4:
        raise ValueError("lut must be the [N + 3, 4] uint8 table of colormap_lut")
    if raster is None:
        raster = mercator_raster_for(shape[-2:], grid_limits, grid_origin, R=R)
    raster = _check_raster(raster)
    warped = warp_to_mercator_device(plane, grid_limits, grid_origin, raster, method=method, R=R, device=device)
    if _is_tensor(lut):
        lut = lut.to(warped.device)
    rgba = colormap_rgba_device(warped, lut, vmin, vmax)
    if resampling == "average":
        levels = [colormap_rgba_device(level, lut, vmin, vmax)
                  for level in overview_pyramid_device(warped, factors, "average")]
    else:
        levels = overview_pyramid_device(rgba, factors, "nearest")
    return raster, rgba, levels
