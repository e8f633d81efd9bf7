"""ctypes binding of libradargrid_hip.so (declared in include/radargrid_hip.h).

There is deliberately NO CPU fallback: if the shared library is missing, does not load, or no HIP device is
visible, every product entry point raises :class:`NativeUnavailable`.  PyTorch is used by the callers only
as plumbing -- device allocations (``tensor.data_ptr()``) and the current HIP stream.
"""
from __future__ import annotations

import ctypes
import os
import threading
from ctypes import (POINTER, Structure, c_char_p, c_double, c_float, c_int32, c_int64, c_uint8, c_void_p)

HERE = os.path.dirname(os.path.abspath(__file__))
# The product loads the in-tree library and nothing else: no environment override.  Measurement scripts that want
# another build of the library (tools/exp_rowwise.py --libs) assign ``_native.LIB_PATH`` themselves before the first
# load; the ABI check below applies to them as well.
LIB_PATH = os.path.join(HERE, "csrc", "libradargrid_hip.so")
ABI_VERSION = 104          # include/radargrid_hip.h: RG_VERSION -- load_library refuses a library built from another header

RG_MAX_FIELDS = 8
RG_MAX_RADARS = 16         # radars one rg_roi_grid_mosaic_f32 / rg_roi_section_mosaic_f32 launch takes
RG_NO_RADAR = 255          # out_radar of the combine entry points: the value is the fill
RG_EXCLUDED_BITS = 0x7FD1CE5D

RG_OK, RG_EINVAL, RG_EALIGN, RG_ELAUNCH, RG_EWORKSPACE, RG_EUNSUPPORTED, RG_ENODEVICE = 0, -1, -2, -3, -4, -5, -6
GATE_OPS = {"below": 0, "above": 1, "between": 2, "outside": 3, "equal": 4, "invalid": 5}
COLUMN_OPS = {"max": 0, "min": 1, "mean": 2}
WEIGHTINGS = {"barnes2": 0, "cressman": 1, "nearest": 2, "closest": 3}
COMBINES = {"mean": 0, "max": 1, "nearest_radar": 2}     # rg_combine: how a mosaic launch combines its radars
RG_MAX_PROFILE_THRESHOLDS = 4   # thresholds one rg_column_profile_f32 launch takes
RG_MAX_PLANE_TESTS = 12
RG_TEST_LO, RG_TEST_HI, RG_TEST_LO_INCLUSIVE, RG_TEST_NONFINITE = 1, 2, 4, 8
RG_MINMAX_WORKSPACE_BYTES = 32768
RG_MAX_LUT = 4093
RG_COMPACT_LINES = 4          # grid lines (= wavefronts) per chunk of the compact CSR copy (header: RG_COMPACT_LINES)
RG_COMPACT_MAX_WINDOW = 8192
RG_COMPACT_ROTATION = 5       # block -> chunk column rotation per line group (header: RG_COMPACT_ROTATION)
RG_REC_ORDER_SEGMENT, RG_REC_ORDER_DISPATCH = 0, 1
RG_ROW_END16_MAX = 65534      # largest segment span the row-end table holds (header: RG_ROW_END16_MAX)
RG_ROW_END16_WIDE = 0xFFFF    # table entries of a segment beyond it, which reads the row pointers (header: RG_ROW_END16_WIDE)
RG_CC_TILE_H, RG_CC_TILE_W = 32, 64   # tile of the connected-component labelling (header: RG_CC_TILE_H / RG_CC_TILE_W)
RG_DENSE_MAX_DICT = 2048      # chunks with at most this many dictionary entries keep 14-byte records (header: RG_DENSE_MAX_DICT)


class NativeUnavailable(RuntimeError):
    """The HIP extension (or a HIP device) is missing; the product path refuses to run without it."""


class NativeError(RuntimeError):
    """A C-ABI entry point returned a negative rg_status."""


class CellGrid(Structure):
    _fields_ = [("x0", c_double), ("y0", c_double), ("inv_cx", c_double), ("inv_cy", c_double),
                ("z_lo", c_double), ("z_hi", c_double), ("ncx", c_int32), ("ncy", c_int32), ("levels", c_int32),
                ("level0", c_int32)]


class MosaicRadar(Structure):
    """``rg_mosaic_radar``: one radar of an ``rg_roi_grid_mosaic_f32`` launch (device pointers, host-side table)."""
    _fields_ = [("sorted_gates", c_void_p), ("cell_start", c_void_p), ("cells", CellGrid), ("xc", c_void_p),
                ("yc", c_void_p), ("zc", c_void_p), ("ix0", c_int32), ("iy0", c_int32), ("nx_win", c_int32),
                ("ny_win", c_int32), ("gate_offset", c_int64), ("n_gates", c_int64)]


class SectionRadar(Structure):
    """``rg_section_radar``: one radar of an ``rg_roi_section_mosaic_f32`` launch (device pointers, host-side table)."""
    _fields_ = [("sorted_gates", c_void_p), ("cell_start", c_void_p), ("cells", CellGrid), ("xs", c_void_p),
                ("ys", c_void_p), ("zc", c_void_p), ("gate_offset", c_int64), ("n_gates", c_int64)]


class PlaneTest(Structure):
    _fields_ = [("plane", c_void_p), ("lo", c_float), ("hi", c_float), ("flags", c_int32)]


class Georef(Structure):
    """``rg_georef``: the float64 constants of a re-projection between two AEQD planes (``georef.make_georef`` fills it)."""
    _fields_ = [("radius", c_double), ("lon_from", c_double), ("lat_from", c_double), ("sin_lat_from", c_double),
                ("cos_lat_from", c_double), ("lon_to", c_double), ("lat_to", c_double), ("sin_lat_to", c_double),
                ("cos_lat_to", c_double), ("ox", c_double), ("oy", c_double), ("same_centre", c_int32),
                ("reserved", c_int32)]


class MercatorRaster(Structure):
    """``rg_mercator_raster``: a north-up Web Mercator raster (``warp.MercatorRaster`` is the Python-side tuple)."""
    _fields_ = [("x_min", c_double), ("y_max", c_double), ("pixel", c_double), ("width", c_int32), ("height", c_int32)]


class WarpSource(Structure):
    """``rg_warp_source``: the float64 node lattice of the plane a warp samples."""
    _fields_ = [("x_lo", c_double), ("y_lo", c_double), ("step_x", c_double), ("step_y", c_double), ("ny", c_int32),
                ("nx", c_int32)]


class MotionLattice(Structure):
    """``rg_motion_lattice``: the node lattice of a motion field, in pixels; passed to ``rg_advect_f32`` BY VALUE."""
    _fields_ = [("origin_y", c_double), ("origin_x", c_double), ("step_y", c_double), ("step_x", c_double), ("ny", c_int32),
                ("nx", c_int32)]


RG_MOTION_MAX_BLOCK = 64    # largest block side of rg_block_match_u8 (header: RG_MOTION_MAX_BLOCK)
RG_MOTION_MAX_SEARCH = 32   # largest search radius (header: RG_MOTION_MAX_SEARCH)
RG_MAX_LEADS = 16           # lead times one rg_advect_f32 launch takes (header: RG_MAX_LEADS)
RG_MAX_ACC_STEPS = 64       # sub-instants one rg_accumulate_advected_f32 launch sums (header: RG_MAX_ACC_STEPS)
RG_MAX_VERIFY_THRESHOLDS = 8   # thresholds one verification launch takes (header: RG_MAX_VERIFY_THRESHOLDS)
RG_MAX_VERIFY_SCALES = 16      # window sizes one rg_fss_sums_i32 launch takes (header: RG_MAX_VERIFY_SCALES)
RG_MAX_VERIFY_SCALE = 255      # largest window size (header: RG_MAX_VERIFY_SCALE)
RG_MAX_DISK_RADIUS = 127       # largest footprint radius and half-width in pixels (header: RG_MAX_DISK_RADIUS)
RG_MAX_CONV_CLASSES = 8        # radius classes of the convective centres (header: RG_MAX_CONV_CLASSES)
RG_MAX_MEMBERS = 64            # ensemble members one rg_ensemble_exceedance_f32 launch takes (radargrid_ensemble.h: RG_MAX_MEMBERS)
RG_MAX_SEL_PLANES = 4      # level selections (constant-elevation PPIs) one planes-mode launch samples
RG_PPI_SEL_NONE = -1


class PlaneRequest(Structure):
    """``rg_plane_request``: what one ``rg_csr_compact_apply_planes_f32`` launch produces (device pointers)."""
    _fields_ = [("out", c_void_p), ("level_planes", c_void_p), ("keep_lo", c_int32), ("n_keep", c_int32),
                ("col_max", c_void_p), ("col_arg", c_void_p), ("col_min", c_void_p), ("col_mean", c_void_p),
                ("col_lo", c_int32), ("col_hi", c_int32), ("n_sel", c_int32), ("reserved", c_int32),
                ("sel_levels", c_void_p * RG_MAX_SEL_PLANES), ("sel_samples", c_void_p)]


# name -> (restype, argtypes); mirrors include/radargrid_hip.h one to one
SIGNATURES = {
    "rg_version": (c_int32, []),
    "rg_last_error": (c_char_p, []),
    "rg_device_count": (c_int32, []),
    "rg_stream_read_probe": (c_int32, [c_void_p, c_int64, c_void_p, c_void_p]),
    "rg_antenna_to_cartesian_f32": (c_int32, [c_void_p, c_int32, c_void_p, c_void_p, c_int32, c_void_p, c_void_p,
                                              c_void_p, c_void_p]),
    "rg_gate_mask_f32": (c_int32, [c_void_p, c_int64, c_int32, c_float, c_float, c_void_p, c_void_p]),
    "rg_pack_fields_f32": (c_int32, [c_int32, POINTER(c_void_p), POINTER(c_void_p), c_void_p, c_int64, c_int32,
                                     c_void_p, c_void_p]),
    "rg_csr_apply_f32": (c_int32, [c_void_p, c_int32, c_void_p, c_void_p, c_int64, c_int64, c_int64, c_void_p, c_int32,
                                   c_int32, c_int64, c_float, c_void_p, c_void_p]),
    "rg_csr_apply_f32_ex": (c_int32, [c_void_p, c_int32, c_void_p, c_void_p, c_int64, c_int64, c_int64, c_void_p,
                                      c_int32, c_int32, c_int64, c_float, c_void_p, c_int32, c_void_p]),
    "rg_column_reduce_f32": (c_int32, [c_void_p, c_int32, c_int64, c_int32, c_int32, c_int32, c_void_p, c_void_p,
                                       c_void_p]),
    "rg_column_profile_f32": (c_int32, [c_void_p, c_int32, c_int64, c_int32, c_int32, c_void_p, POINTER(c_double), c_int32,
                                        c_int32, c_void_p, c_void_p, c_double, c_void_p, c_void_p]),
    "rg_cappi_lerp_f32": (c_int32, [c_void_p, c_int64, c_int32, c_float, c_float, c_void_p, c_void_p]),
    "rg_elevation_ppi_f32": (c_int32, [c_void_p, c_void_p, c_void_p, c_int32, c_int32, c_int32, c_double, c_double,
                                       c_double, c_double, c_double, c_double, c_double, c_double, c_int32, c_int32,
                                       c_void_p, c_void_p]),
    "rg_geom_bin_workspace_bytes": (c_int64, [c_int64, c_int32, c_int32]),
    "rg_geom_bin_gates_f32": (c_int32, [c_void_p, c_void_p, c_void_p, c_int64, c_float, c_float, POINTER(CellGrid),
                                        c_void_p, c_void_p, c_void_p, c_int64, c_void_p]),
    "rg_geom_bin_levels_count": (c_int32, [c_void_p, c_void_p, c_void_p, c_int64, c_float, c_float, POINTER(CellGrid), c_void_p,
                                           c_int32, c_double, c_double, c_void_p, c_void_p]),
    "rg_geom_bin_levels_workspace_bytes": (c_int64, [c_int64, c_int64, c_int64]),
    "rg_geom_bin_gates_levels_f32": (c_int32, [c_void_p, c_void_p, c_void_p, c_int64, c_float, c_float, POINTER(CellGrid),
                                               c_void_p, c_int32, c_double, c_double, c_int64, c_void_p, c_void_p, c_void_p,
                                               c_int64, c_void_p]),
    "rg_geom_count_f32": (c_int32, [c_void_p, c_void_p, POINTER(CellGrid), c_void_p, c_void_p, c_void_p, c_int32,
                                    c_int32, c_int32, c_double, c_double, c_void_p, c_void_p]),
    "rg_csr_compact_apply_f32": (c_int32, [c_void_p, c_int32, c_void_p, c_void_p, c_void_p, c_void_p, c_int64, c_int64,
                                           c_int64, c_int64, c_void_p, c_int32, c_int32, c_int64, c_float, c_void_p,
                                           c_int32, c_int32, c_void_p]),
    "rg_csr_compact_pack": (c_int32, [c_void_p, c_int32, c_void_p, c_void_p, c_int64, c_int64, c_int64, c_void_p,
                                      c_int32, c_int64, ctypes.c_uint32, c_void_p, c_void_p, c_void_p]),
    "rg_csr_compact_pack_dense": (c_int32, [c_void_p, c_int32, c_void_p, c_void_p, c_int64, c_int64, c_int64, c_void_p,
                                            c_void_p, c_int32, c_int64, ctypes.c_uint32, c_void_p, c_void_p, c_void_p]),
    "rg_csr_compact_apply_packed_f32": (c_int32, [c_void_p, c_int32, c_void_p, c_void_p, c_int32, ctypes.c_uint32, c_void_p,
                                                  c_void_p, c_int64, c_int64, c_int64, c_int64, c_void_p, c_int32,
                                                  c_int32, c_int64, c_float, c_void_p, c_int32, c_int32, c_void_p]),
    "rg_csr_row_ends16": (c_int32, [c_void_p, c_int32, c_int64, c_int64, c_int64, c_void_p, c_void_p]),
    "rg_csr_compact_apply_packed_f32_ex": (c_int32, [c_void_p, c_int32, c_void_p, c_void_p, c_int32, ctypes.c_uint32, c_void_p,
                                                     c_void_p, c_int64, c_int64, c_int64, c_int64, c_void_p, c_int32,
                                                     c_int32, c_int64, c_float, c_void_p, c_int32, c_int32, c_void_p,
                                                     c_void_p]),
    "rg_csr_compact_apply_columns_f32_ex": (c_int32, [c_void_p, c_int32, c_void_p, c_void_p, c_int32, ctypes.c_uint32, c_void_p,
                                                      c_void_p, c_int64, c_int64, c_int64, c_int64, c_void_p, c_int32,
                                                      c_int32, c_int64, c_float, c_void_p, c_void_p, c_int32, c_int32,
                                                      c_void_p, c_void_p, c_int32, c_int32, c_int32, c_int32, c_void_p,
                                                      c_void_p, c_int64, c_int32, c_void_p, c_void_p]),
    "rg_csr_compact_apply_planes_f32_ex": (c_int32, [c_void_p, c_int32, c_void_p, c_void_p, c_int32, ctypes.c_uint32, c_void_p,
                                                     c_void_p, c_int64, c_int64, c_int64, c_int64, c_void_p, c_int32,
                                                     c_int32, c_int64, c_float, POINTER(PlaneRequest), c_int32, c_int32,
                                                     c_void_p, c_void_p, c_int64, c_int32, c_void_p, c_void_p]),
    "rg_csr_columns_workspace_bytes": (c_int64, [c_int64, c_int64, c_int32, c_int32]),
    "rg_csr_compact_apply_columns_f32": (c_int32, [c_void_p, c_int32, c_void_p, c_void_p, c_int32, ctypes.c_uint32, c_void_p,
                                                   c_void_p, c_int64, c_int64, c_int64, c_int64, c_void_p, c_int32,
                                                   c_int32, c_int64, c_float, c_void_p, c_void_p, c_int32, c_int32,
                                                   c_void_p, c_void_p, c_int32, c_int32, c_int32, c_int32, c_void_p,
                                                   c_void_p, c_int64, c_int32, c_void_p]),
    "rg_csr_planes_workspace_bytes": (c_int64, [c_int64, c_int64, c_int32, c_int32, c_int32, c_int32]),
    "rg_csr_compact_apply_planes_f32": (c_int32, [c_void_p, c_int32, c_void_p, c_void_p, c_int32, ctypes.c_uint32, c_void_p,
                                                  c_void_p, c_int64, c_int64, c_int64, c_int64, c_void_p, c_int32,
                                                  c_int32, c_int64, c_float, POINTER(PlaneRequest), c_int32, c_int32,
                                                  c_void_p, c_void_p, c_int64, c_int32, c_void_p]),
    "rg_elevation_ppi_plan_f32": (c_int32, [c_void_p, c_void_p, c_int32, c_int32, c_int32, c_double, c_double, c_double,
                                            c_double, c_double, c_double, c_double, c_double, c_int32, c_int32, c_void_p,
                                            c_void_p, c_void_p]),
    "rg_elevation_ppi_finish_f32": (c_int32, [c_void_p, c_void_p, c_void_p, c_int64, c_int32, c_void_p, c_void_p]),
    "rg_csr_compact_chunks": (c_int64, [c_int64, c_int64, c_int64]),
    "rg_csr_compact_count": (c_int32, [c_void_p, c_int32, c_void_p, c_int64, c_int64, c_int64, c_void_p, c_void_p,
                                       c_void_p]),
    "rg_csr_compact_fill": (c_int32, [c_void_p, c_int32, c_void_p, c_int64, c_int64, c_int64, c_void_p, c_void_p,
                                      c_void_p, c_void_p, c_void_p, c_void_p]),
    "rg_scan_workspace_bytes": (c_int64, [c_int64]),
    "rg_scan_counts_i64": (c_int32, [c_void_p, c_int64, c_void_p, c_void_p, c_int64, c_void_p]),
    "rg_geom_fill_f32": (c_int32, [c_void_p, c_void_p, POINTER(CellGrid), c_void_p, c_void_p, c_void_p, c_int32,
                                   c_int32, c_int32, c_double, c_double, c_int32, c_void_p, c_void_p, c_void_p,
                                   c_void_p]),
    "rg_roi_grid_f32": (c_int32, [c_void_p, c_void_p, POINTER(CellGrid), c_void_p, c_void_p, c_void_p, c_int32,
                                  c_int32, c_int32, c_double, c_double, c_int32, c_void_p, c_int32, c_int32,
                                  c_float, c_void_p, c_void_p]),
    "rg_roi_grid_mosaic_f32": (c_int32, [POINTER(MosaicRadar), c_int32, c_int32, c_int32, c_int32, c_double, c_double,
                                         c_int32, c_void_p, c_int32, c_int32, c_int64, c_float, c_void_p, c_void_p]),
    "rg_roi_grid_mosaic_combine_f32": (c_int32, [POINTER(MosaicRadar), c_int32, c_int32, c_int32, c_int32, c_double,
                                                 c_double, c_int32, c_void_p, c_int32, c_int32, c_int64, c_float, c_void_p,
                                                 c_int32, c_void_p, c_void_p]),
    "rg_roi_section_f32": (c_int32, [c_void_p, c_void_p, POINTER(CellGrid), c_void_p, c_void_p, c_void_p, c_int32,
                                     c_int32, c_double, c_double, c_int32, c_void_p, c_int32, c_int32, c_float, c_void_p,
                                     c_void_p]),
    "rg_roi_section_mosaic_f32": (c_int32, [POINTER(SectionRadar), c_int32, c_int32, c_int32, c_double, c_double, c_int32,
                                            c_void_p, c_int32, c_int32, c_int64, c_float, c_void_p, c_void_p]),
    "rg_roi_section_mosaic_combine_f32": (c_int32, [POINTER(SectionRadar), c_int32, c_int32, c_int32, c_double, c_double,
                                                    c_int32, c_void_p, c_int32, c_int32, c_int64, c_float, c_void_p,
                                                    c_int32, c_void_p, c_void_p]),
    "rg_section_count_f32": (c_int32, [c_void_p, c_void_p, POINTER(CellGrid), c_void_p, c_void_p, c_void_p, c_int32,
                                       c_int32, c_double, c_double, c_void_p, c_void_p]),
    "rg_section_fill_f32": (c_int32, [c_void_p, c_void_p, POINTER(CellGrid), c_void_p, c_void_p, c_void_p, c_int32,
                                      c_int32, c_double, c_double, c_int32, c_void_p, c_void_p, c_void_p, c_void_p]),
    "rg_collapse_ppi_f32": (c_int32, [c_void_p, c_void_p, c_void_p, c_void_p, c_int32, c_int32, c_int32, c_double,
                                      c_double, c_void_p, c_void_p, c_void_p]),
    "rg_plane_filter_f32": (c_int32, [c_void_p, c_void_p, c_int64, POINTER(PlaneTest), c_int32, c_void_p, c_void_p,
                                      c_void_p]),
    "rg_grid_filter": (c_int32, [c_void_p, c_int32, c_int64, c_int32, c_double, c_double, c_void_p, c_double, c_void_p,
                                 c_void_p]),
    "rg_nan_minmax": (c_int32, [c_void_p, c_int32, c_int64, c_int32, c_double, c_void_p, c_void_p, c_void_p]),
    "rg_colormap_rgba": (c_int32, [c_void_p, c_int32, c_int64, c_double, c_double, c_int32, c_double, c_void_p,
                                   c_int32, c_void_p, c_void_p]),
    "rg_gates_to_frame_f32": (c_int32, [c_void_p, c_void_p, c_int64, POINTER(Georef), c_void_p, c_void_p, c_void_p]),
    "rg_frame_to_lonlat_f64": (c_int32, [c_void_p, c_void_p, c_int32, c_int32, POINTER(Georef), c_void_p, c_void_p,
                                         c_void_p]),
    "rg_warp_mercator_f32": (c_int32, [c_void_p, c_int32, POINTER(WarpSource), POINTER(Georef), POINTER(MercatorRaster),
                                       c_int32, c_float, c_void_p, c_void_p]),
    "rg_warp_mercator_rgba8": (c_int32, [c_void_p, POINTER(WarpSource), POINTER(Georef), POINTER(MercatorRaster), c_void_p,
                                         c_void_p]),
    "rg_overview_f32": (c_int32, [c_void_p, c_int32, c_int32, c_int32, c_int32, c_int32, c_void_p, c_void_p]),
    "rg_overview_rgba8": (c_int32, [c_void_p, c_int32, c_int32, c_int32, c_void_p, c_void_p]),
    "rg_components_workspace_bytes": (c_int64, [c_int32, c_int32, c_int32]),
    "rg_label_components_f32": (c_int32, [c_void_p, c_void_p, c_int32, c_int32, c_int32, c_float, c_float, c_int32, c_int32,
                                          c_void_p, c_void_p, c_void_p, c_int64, c_void_p]),
    "rg_component_stats_f32": (c_int32, [c_void_p, c_void_p, c_void_p, c_int32, c_int32, c_int32, c_int32, c_void_p, c_void_p,
                                         c_void_p, c_void_p, c_void_p, c_void_p, c_void_p]),
    "rg_despeckle_select_f32": (c_int32, [c_void_p, c_void_p, c_void_p, c_void_p, c_int32, c_int32, c_int32, c_int32, c_float,
                                          c_void_p, c_void_p, c_void_p]),
    "rg_motion_quantize_f32": (c_int32, [c_void_p, c_void_p, c_int32, c_int32, c_int32, c_float, c_float, c_void_p, c_void_p]),
    "rg_block_match_u8": (c_int32, [c_void_p, c_void_p, c_int32, c_int32, c_int32, c_int32, c_int32, c_int32, c_int32,
                                    c_void_p, c_void_p, c_void_p, c_void_p]),
    "rg_advect_f32": (c_int32, [c_void_p, c_int32, c_int32, c_int32, c_void_p, MotionLattice, POINTER(c_double), c_int32,
                                c_int32, c_int32, c_float, c_void_p, c_void_p]),
    "rg_rain_rate_f32": (c_int32, [c_void_p, c_void_p, c_int32, c_int32, c_int32, c_double, c_double, c_double, c_double, c_void_p,
                                   c_void_p]),
    "rg_accumulate_advected_f32": (c_int32, [c_void_p, c_void_p, c_int32, c_int32, c_int32, c_void_p, MotionLattice, c_double,
                                             c_int32, c_int32, c_int32, c_int32, c_float, c_void_p, c_void_p, c_void_p]),
    "rg_cell_overlap_workspace_bytes": (c_int64, [c_int64]),
    "rg_cell_overlap_i32": (c_int32, [c_void_p, c_void_p, c_void_p, c_void_p, c_int32, c_int32, c_int32, c_int64, c_void_p,
                                      c_void_p, c_void_p, c_void_p, c_int64, c_void_p]),
    "rg_relabel_cells_i32": (c_int32, [c_void_p, c_void_p, c_int32, c_int32, c_int32, c_void_p, c_int32, c_void_p, c_void_p]),
    "rg_contingency_f32": (c_int32, [c_void_p, c_void_p, c_void_p, c_int32, c_int32, c_int32, POINTER(c_float), c_int32, c_void_p,
                                     c_void_p, c_void_p]),
    "rg_exceedance_sat_i32": (c_int32, [c_void_p, c_void_p, c_void_p, c_int32, c_int32, c_int32, POINTER(c_float), c_int32,
                                        c_void_p, c_void_p]),
    "rg_fss_sums_i32": (c_int32, [c_void_p, c_void_p, c_int32, c_int32, c_int32, POINTER(c_int32), c_int32, c_void_p, c_void_p]),
    "rg_box_fraction_f32": (c_int32, [c_void_p, c_int32, c_int32, c_int32, c_int32, c_void_p, c_void_p]),
    "rg_echo_table_bytes": (c_int64, [c_int32, c_int32, c_int32]),
    "rg_echo_table_f32": (c_int32, [c_void_p, c_void_p, c_int32, c_int32, c_int32, c_float, c_void_p, c_int64, c_void_p]),
    "rg_disk_background": (c_int32, [c_void_p, c_int32, c_int32, c_int32, POINTER(c_int32), c_int32, c_void_p, c_void_p, c_void_p,
                                     c_void_p]),
    "rg_convective_centres_f32": (c_int32, [c_void_p, c_void_p, c_void_p, c_int32, c_int32, c_int32, c_float, c_double, c_double,
                                            c_double, POINTER(c_double), c_int32, c_void_p, c_void_p]),
    "rg_convective_area_workspace_bytes": (c_int64, [c_int32, c_int32, c_int32, c_int32]),
    "rg_convective_area_u8": (c_int32, [c_void_p, c_void_p, c_void_p, c_int32, c_int32, c_int32, c_float, c_int32, POINTER(c_int32),
                                        POINTER(c_int32), c_void_p, c_int64, c_void_p, c_void_p]),
}

# name -> (restype, argtypes); mirrors include/radargrid_ensemble.h one to one.  A table of its own, bound after SIGNATURES from
# the same library: the probabilistic nowcasts were added without touching radargrid_hip.h or the table above.
ENSEMBLE_SIGNATURES = {
    "rg_ensemble_exceedance_f32": (c_int32, [c_void_p, c_int32, c_int32, c_void_p, MotionLattice, POINTER(c_double), c_int32, c_int32,
                                             c_int32, c_void_p, c_int32, POINTER(c_float), c_int32, c_int32, c_void_p, c_void_p,
                                             c_void_p, c_void_p, c_void_p]),
    "rg_ensemble_histogram_u8": (c_int32, [c_void_p, c_void_p, c_void_p, c_void_p, c_int32, c_int32, c_int32, c_int32,
                                           POINTER(c_float), c_int32, c_void_p, c_void_p, c_void_p]),
}

RG_PHASE_MAX_GATES = 32768         # gates of one ray (radargrid_phase.h: RG_PHASE_MAX_GATES)
RG_PHASE_MAX_CLASSES = 4           # half-window classes of rg_phidp_fit_f32 (radargrid_phase.h: RG_PHASE_MAX_CLASSES)
RG_PHASE_MAX_HALF_WINDOW = 255     # largest half-window in gates (radargrid_phase.h: RG_PHASE_MAX_HALF_WINDOW)
RG_PHASE_MAX_WORKGROUPS = 16777215 # workgroups of 256 one launch holds (radargrid_phase.h: RG_PHASE_MAX_WORKGROUPS)
RG_PHASE_MAX_ABS_PHI = 16384       # |phi| in degrees beyond which a gate is left out of a fit (radargrid_phase.h)

# name -> (restype, argtypes); mirrors include/radargrid_phase.h one to one.  The third table, bound after the other two from the
# same library: the polar-domain phase processing was added without touching either header or either table above.
PHASE_SIGNATURES = {
    "rg_phidp_unfold_f32": (c_int32, [c_void_p, c_void_p, c_int32, c_int32, c_double, c_void_p, c_void_p, c_void_p]),
    "rg_phidp_fit_f32": (c_int32, [c_void_p, c_int32, c_int32, c_void_p, POINTER(c_double), POINTER(c_int32), c_int32, c_int32,
                                   c_int32, c_double, c_void_p, c_void_p, c_void_p, c_void_p]),
    "rg_attenuation_phidp_f32": (c_int32, [c_void_p, c_void_p, c_int32, c_int32, c_double, c_double, c_double, c_void_p, c_void_p,
                                           c_void_p, c_void_p, c_void_p, c_void_p, c_void_p]),
}

RG_VELOCITY_MAX_ABS = 16384           # |v| in m/s beyond which a gate is not valid (radargrid_velocity.h: RG_VELOCITY_MAX_ABS)
RG_VELOCITY_MAX_NYQUIST = 8192        # the largest Nyquist velocity in m/s (radargrid_velocity.h: RG_VELOCITY_MAX_NYQUIST)
RG_VELOCITY_MIN_BANDS = 2             # n_bands from (radargrid_velocity.h: RG_VELOCITY_MIN_BANDS)
RG_VELOCITY_MAX_BANDS = 8             # ... to (radargrid_velocity.h: RG_VELOCITY_MAX_BANDS)
RG_VELOCITY_SWEEPS_PER_LAUNCH = 64    # Nyquist velocities one launch carries (radargrid_velocity.h)

# name -> (restype, argtypes); mirrors include/radargrid_velocity.h one to one.  The fourth table, bound after the other three
# from the same library: velocity dealiasing was added without touching a header or a table above.
VELOCITY_SIGNATURES = {
    "rg_velocity_split_f32": (c_int32, [c_void_p, c_void_p, c_int32, c_int32, c_int32, POINTER(c_double), c_int32, c_void_p,
                                        c_void_p]),
    "rg_velocity_regions_i32": (c_int32, [c_void_p, c_void_p, c_int32, c_int32, c_int32, c_int32, c_void_p, c_void_p]),
    "rg_region_edges_workspace_bytes": (c_int64, [c_int64]),
    "rg_region_edges_f32": (c_int32, [c_void_p, c_void_p, c_int32, c_int32, c_int32, c_int32, c_int64, c_void_p, c_void_p,
                                      c_void_p, c_void_p, c_void_p, c_int64, c_void_p]),
    "rg_velocity_apply_folds_f32": (c_int32, [c_void_p, c_void_p, c_void_p, c_int32, c_int32, c_int32, c_int32, POINTER(c_double),
                                              c_void_p, c_void_p, c_void_p]),
}

RG_SHEAR_MEDIAN_MAX_HALF = 2          # half-widths of the median window from 0 to (radargrid_shear.h: RG_SHEAR_MEDIAN_MAX_HALF)
RG_SHEAR_MAX_HALF_RAYS = 16           # the LLSD window: half-width in rays at most (radargrid_shear.h: RG_SHEAR_MAX_HALF_RAYS)
RG_SHEAR_MAX_HALF_GATES = 16          # ... and in gates (radargrid_shear.h: RG_SHEAR_MAX_HALF_GATES)
RG_SHEAR_MAX_WINDOW = 1089            # 33 * 33 gates: the largest count (radargrid_shear.h: RG_SHEAR_MAX_WINDOW)

# name -> (restype, argtypes); mirrors include/radargrid_shear.h one to one.  The fifth table, bound after the other four from
# the same library: the LLSD was added without touching a header or a table above.
SHEAR_SIGNATURES = {
    "rg_polar_median_f32": (c_int32, [c_void_p, c_void_p, c_int32, c_int32, c_int32, c_int32, c_int32, c_int32, c_int32, c_int32,
                                      c_void_p, c_void_p]),
    "rg_velocity_llsd_f32": (c_int32, [c_void_p, c_void_p, c_int32, c_int32, c_int32, c_void_p, c_void_p, c_int32, c_int32, c_double,
                                       c_int32, c_int32, c_int32, c_int32, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p]),
}

RG_HYDRO_TEXTURE_SHIFT = 10           # the fixed point of the texture: q = x * 2^10 (radargrid_hydro.h: RG_HYDRO_TEXTURE_SHIFT)
RG_HYDRO_MAX_ABS = 8192               # |x| beyond which a gate is not valid for the texture (radargrid_hydro.h: RG_HYDRO_MAX_ABS)
RG_HYDRO_MAX_HALF_GATES = 63          # the texture window: half-width in gates at most (radargrid_hydro.h)
RG_HYDRO_TEXTURE_TILE = 512           # gates of one ray a workgroup of the texture takes at a time (radargrid_hydro.h)
RG_HYDRO_MAX_VARS = 8                 # variables of the classifier (radargrid_hydro.h: RG_HYDRO_MAX_VARS)
RG_HYDRO_MAX_CLASSES = 16             # classes (radargrid_hydro.h: RG_HYDRO_MAX_CLASSES)
RG_HYDRO_MAX_BINS = 32                # bins of the condition variable (radargrid_hydro.h: RG_HYDRO_MAX_BINS)
RG_HYDRO_MAX_CELLS = 1024             # B * C * V at most (radargrid_hydro.h: RG_HYDRO_MAX_CELLS)
RG_HYDRO_UNCLASSIFIED = 0             # cls of a gate without a class (radargrid_hydro.h: RG_HYDRO_UNCLASSIFIED)

# name -> (restype, argtypes); mirrors include/radargrid_hydro.h one to one.  The sixth table, bound after the other five from
# the same library: the hydrometeor classification was added without touching a header or a table above.
HYDRO_SIGNATURES = {
    "rg_polar_texture_f32": (c_int32, [c_void_p, c_void_p, c_int32, c_int32, c_int32, c_int32, c_int32, c_void_p, c_void_p, c_void_p,
                                       c_void_p]),
    "rg_fuzzy_classify_f32": (c_int32, [POINTER(c_void_p), POINTER(c_int32), c_int32, c_int32, c_int32, c_int32, c_void_p, c_int32,
                                        c_int32, c_int32, POINTER(c_double), c_int32, c_void_p, c_int32, POINTER(c_double), c_double,
                                        c_void_p, c_void_p, c_void_p, c_void_p]),
}

_lock = threading.Lock()
_lib = None


def load_library(require_device: bool = True):
    """dlopen the in-tree library and bind every declared symbol.  Raises NativeUnavailable loudly."""
    global _lib
    with _lock:
        if _lib is None:
            # PyTorch-ROCm ships its own HIP runtime; it must be the one already loaded when our library is
            # dlopen-ed, so that both share ONE runtime (streams and device pointers are only meaningful within it).
            # Loading ours first would pull in the system libamdhip64 and leave torch without a usable device.
            torch_mod()
            if not os.path.exists(LIB_PATH):
                raise NativeUnavailable(
                    f"{LIB_PATH} is missing: build it with `python -m radar_processor_amd.build` "
                    "(hipcc --offload-arch=gfx950). There is no CPU fallback for the radar_grid hot path.")
            try:
                lib = ctypes.CDLL(LIB_PATH)
            except OSError as exc:  # missing ROCm runtime etc.
                raise NativeUnavailable(f"cannot load {LIB_PATH}: {exc}") from exc
            try:
                lib.rg_version.restype = c_int32
                built_for = int(lib.rg_version())
            except AttributeError:
                raise NativeUnavailable(f"{LIB_PATH} does not export rg_version") from None
            if built_for != ABI_VERSION:
                raise NativeUnavailable(
                    f"{LIB_PATH} was built from header version {built_for}, this package binds version {ABI_VERSION}: the "
                    "signatures differ, calling it would shift arguments. Rebuild it with `python -m radar_processor_amd.build`.")
            for name, (restype, argtypes) in (list(SIGNATURES.items()) + list(ENSEMBLE_SIGNATURES.items())
                                              + list(PHASE_SIGNATURES.items()) + list(VELOCITY_SIGNATURES.items())
                                              + list(SHEAR_SIGNATURES.items()) + list(HYDRO_SIGNATURES.items())):
                try:
                    fn = getattr(lib, name)
                except AttributeError:
                    raise NativeUnavailable(f"{LIB_PATH} does not export {name}") from None
                fn.restype = restype
                fn.argtypes = argtypes
            _lib = lib
    if require_device and _lib.rg_device_count() <= 0:
        raise NativeUnavailable("libradargrid_hip.so loaded but no HIP device is visible "
                                f"({_lib.rg_last_error().decode()}); the radar_grid hot path has no CPU fallback.")
    return _lib


def check(status: int, what: str) -> None:
    if status < 0:
        msg = load_library(require_device=False).rg_last_error().decode()
        raise NativeError(f"{what} failed with rg_status {status}: {msg}")


def torch_mod():
    try:
        import torch
    except Exception as exc:  # pragma: no cover
        raise NativeUnavailable(f"PyTorch-ROCm is required for device memory and streams: {exc}") from exc
    return torch


def device(index=None):
    """Return the torch device the HIP path runs on; raises when there is none."""
    torch = torch_mod()
    load_library(require_device=True)
    if not torch.cuda.is_available():
        raise NativeUnavailable("torch.cuda.is_available() is False: no MI355X visible to PyTorch-ROCm")
    if index is None:
        index = torch.cuda.current_device()
    return torch.device("cuda", index)


def canonical_device(dev):
    """``torch.device("cuda")`` / ``"cuda:1"`` / an int -> the indexed ``torch.device``: tensors report ``cuda:N``, and an
    index-less device compares unequal to it (a cache keyed on the device would otherwise never hit)."""
    torch = torch_mod()
    if dev is None:
        return device()
    dev = torch.device("cuda", dev) if isinstance(dev, int) else torch.device(dev)
    if dev.type == "cuda" and dev.index is None:
        dev = torch.device("cuda", torch.cuda.current_device())
    return dev


def stream_ptr() -> int:
    """hipStream_t of torch's current stream (0 = the null stream)."""
    torch = torch_mod()
    return int(torch.cuda.current_stream().cuda_stream)


def ptr(t) -> int:
    """Device pointer of a tensor (None -> NULL)."""
    return 0 if t is None else int(t.data_ptr())
