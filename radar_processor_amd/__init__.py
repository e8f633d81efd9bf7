"""radar_processor_amd -- MI355X-native implementation of the ``radar_grid`` hot path of
jgmarti84/radar-processor: geometry build -> CSR apply -> CAPPI / COLMAX, behind the reference's own Python
function surface (``radar_grid/__init__.py:39-82``, hot-path names only).

    from radar_processor_amd import (GridGeometry, compute_grid_geometry, apply_geometry, apply_geometry_multi,
                                     GateFilter, constant_altitude_ppi, column_max, save_geometry, load_geometry)

Host code is Python on PyTorch-ROCm tensors (allocations + streams only); the work is done by hand-written HIP
kernels for gfx950 in ``csrc/`` behind the C ABI of ``include/radargrid_hip.h``.  There is no CPU fallback:
without the built library and a HIP device every compute entry point raises ``NativeUnavailable``.

(The directory is spelled ``radar_processor_amd`` because a hyphen cannot appear in a Python package name;
``radar-processor_amd`` at the repository root is a symlink to it.)
"""
from ._native import NativeError, NativeUnavailable, load_library
from .gate_filters import GateFilter, GridFilter, create_mask_from_filter, device_gate_mask
from .geometry_builder import RoiSearch, compute_grid_geometry
from .grid_geometry import (DeviceCSR, GridGeometry, load_device_layout, load_geometry, save_device_layout, save_geometry)
from .grid_products import (EARTH_RADIUS, EFFECTIVE_RADIUS_FACTOR, column_argmax, column_max, column_mean,
                            column_min, column_profile, compute_beam_height, compute_beam_height_flat,
                            compute_beam_height_simple, constant_altitude_ppi, constant_elevation_ppi, echo_base, echo_top,
                            get_beam_height_difference, get_elevation_from_z_level, vertically_integrated_liquid)
from .gridding import PlaneProducts, apply_geometry, apply_geometry_multi, grid_fields_device
from .plane_products import grid_products_device
from .roi_grid import roi_grid_fields_device
from .mosaic import (MOSAIC_COMBINES, NO_RADAR, MosaicSearch, apply_mosaic, apply_mosaic_multi, compute_mosaic_geometry,
                     compute_mosaic_section_geometry, mosaic_fields_device, mosaic_limits, mosaic_section_fields_device,
                     mosaic_section_points, mosaic_vertical_section, path_reach, reach_window)
from .section import (compute_section_geometry, section_fields_device, section_path, section_rectangle,
                      vertical_section)
from .georef import (AEQD_EARTH_RADIUS, geographic_to_grid, grid_lonlat_device, grid_to_geographic, place_gates_device,
                     place_radar, place_radars, section_path_lonlat)
from .warp import (MercatorRaster, lonlat_to_mercator, mercator_raster_for, mercator_tile, mercator_to_lonlat,
                   overview_pyramid_device, warp_to_mercator_device, web_mercator_rgba)
from .components import (CellTable, cell_table_device, despeckle, despeckle_device, identify_cells,
                         label_components_device)
from .motion import (MotionGrid, advect_device, estimate_motion_device, fill_motion_device, motion_to_velocity, nowcast,
                     nowcast_device, quantize_planes_device)
from .tracking import (CellMatch, CellOverlap, CellTracker, TrackFrame, advect_labels_device, cell_overlap_device, match_cells,
                       relabel_cells_device)
from .accumulation import (AccumulationFrame, RainAccumulator, accumulate, accumulate_device, rain_rate_device)
from .verification import (ContingencyTable, FSSSums, NowcastVerifier, Verification, VerifierFrame, categorical_scores,
                           contingency_device, exceedance_sat_device, fss_device, neighbourhood_fraction_device, verify_nowcast)
from .convection import (ConvectiveStratiform, classify_grid, convective_stratiform, convective_stratiform_device, disk_footprint,
                         echo_background_device, rain_rate_by_class_device)
from .ensemble import (EnsembleProducts, ProbabilityTable, ensemble_exceedance_device, ensemble_histogram_device,
                       motion_perturbations, probabilistic_nowcast, probabilistic_nowcast_device, probability_scores)
from .phase import (ATTENUATION_COEFFICIENTS, AttenuationCorrection, PhaseFit, PhaseProducts, correct_attenuation_device,
                    fit_phidp_device, process_phase, process_phase_device, unfold_phidp_device)
from .velocity import (DealiasedVelocity, RegionEdges, VelocityRegions, apply_folds_device, dealias_velocity,
                       dealias_velocity_device, merge_regions, region_edges_device, split_velocity_device,
                       velocity_regions_device)
from .shear import (ShearWindow, VelocityShear, azimuthal_shear_device, llsd_window, median_filter_device, velocity_shear,
                    velocity_shear_device)
from .hydrometeor import (HYDROMETEOR_CLASSES, HYDROMETEOR_TABLE_S_BAND, HYDROMETEOR_VARIABLES, FuzzyClasses, HydrometeorClasses,
                          MembershipTable, Texture, beam_temperature, class_mask_device, classify_device, classify_hydrometeors,
                          classify_hydrometeors_device, texture, texture_device)
from .processor_seam import build_grid3d_package
from .raster import (PlaneTest, apply_colormap_to_array, apply_filter_masks, collapse_field_3d_to_2d,
                     collapse_grid_to_2d, collapse_plane_device, colormap_lut, colormap_rgba_device,
                     plane_filter_device)
from .radar_adaptors import (get_available_fields, get_field_data, get_gate_coordinates, get_radar_altitude,
                             get_radar_info)

__version__ = "0.1.0"

__all__ = [
    # reference surface (radar_grid/__init__.py:39-82), hot-path subset
    "GridGeometry", "save_geometry", "load_geometry",
    "compute_grid_geometry",
    "apply_geometry", "apply_geometry_multi",
    "get_gate_coordinates", "get_field_data", "get_available_fields", "get_radar_info", "get_radar_altitude",
    "GateFilter", "GridFilter", "create_mask_from_filter",
    "constant_altitude_ppi", "constant_elevation_ppi", "column_max", "column_min", "column_mean",
    "get_elevation_from_z_level", "get_beam_height_difference", "compute_beam_height", "compute_beam_height_flat",
    "EARTH_RADIUS", "EFFECTIVE_RADIUS_FACTOR", "apply_colormap_to_array",
    # 2-D raster stage of radar_processor (utils.py:336-387, processor.py:480-551, :802-886)
    "collapse_field_3d_to_2d", "collapse_grid_to_2d", "apply_filter_masks",
    # build-specific additions
    "save_device_layout", "load_device_layout", "column_argmax", "grid_fields_device", "grid_products_device", "PlaneProducts", "roi_grid_fields_device", "build_grid3d_package", "device_gate_mask", "RoiSearch", "DeviceCSR",
    "mosaic_limits", "reach_window", "compute_mosaic_geometry", "apply_mosaic", "apply_mosaic_multi", "MosaicSearch",
    "mosaic_fields_device", "MOSAIC_COMBINES", "NO_RADAR",
    "mosaic_section_points", "path_reach", "mosaic_section_fields_device", "compute_mosaic_section_geometry",
    "mosaic_vertical_section",
    "section_path", "section_rectangle", "section_fields_device", "compute_section_geometry", "vertical_section",
    "AEQD_EARTH_RADIUS", "geographic_to_grid", "grid_to_geographic", "place_gates_device", "place_radar", "place_radars",
    "section_path_lonlat", "grid_lonlat_device",
    "MercatorRaster", "lonlat_to_mercator", "mercator_to_lonlat", "mercator_raster_for", "mercator_tile",
    "warp_to_mercator_device", "overview_pyramid_device", "web_mercator_rgba",
    "column_profile", "echo_top", "echo_base", "vertically_integrated_liquid",
    "label_components_device", "cell_table_device", "despeckle_device", "despeckle", "identify_cells", "CellTable",
    "quantize_planes_device", "estimate_motion_device", "fill_motion_device", "advect_device", "nowcast_device", "nowcast",
    "motion_to_velocity", "MotionGrid",
    "advect_labels_device", "cell_overlap_device", "match_cells", "relabel_cells_device", "CellTracker", "CellOverlap", "CellMatch",
    "TrackFrame",
    "rain_rate_device", "accumulate_device", "accumulate", "RainAccumulator", "AccumulationFrame",
    "contingency_device", "categorical_scores", "exceedance_sat_device", "neighbourhood_fraction_device", "fss_device",
    "verify_nowcast", "NowcastVerifier", "ContingencyTable", "FSSSums", "Verification", "VerifierFrame",
    "disk_footprint", "echo_background_device", "convective_stratiform_device", "convective_stratiform", "classify_grid",
    "rain_rate_by_class_device", "ConvectiveStratiform",
    "motion_perturbations", "ensemble_exceedance_device", "probabilistic_nowcast_device", "probabilistic_nowcast",
    "ensemble_histogram_device", "probability_scores", "EnsembleProducts", "ProbabilityTable",
    "unfold_phidp_device", "fit_phidp_device", "correct_attenuation_device", "process_phase_device", "process_phase",
    "ATTENUATION_COEFFICIENTS", "PhaseFit", "AttenuationCorrection", "PhaseProducts",
    "split_velocity_device", "velocity_regions_device", "region_edges_device", "merge_regions", "apply_folds_device",
    "dealias_velocity_device", "dealias_velocity", "VelocityRegions", "RegionEdges", "DealiasedVelocity",
    "llsd_window", "median_filter_device", "velocity_shear_device", "azimuthal_shear_device", "velocity_shear", "ShearWindow",
    "VelocityShear",
    "texture_device", "texture", "MembershipTable", "classify_device", "beam_temperature", "classify_hydrometeors_device",
    "classify_hydrometeors", "class_mask_device", "HYDROMETEOR_TABLE_S_BAND", "HYDROMETEOR_CLASSES", "HYDROMETEOR_VARIABLES",
    "Texture", "FuzzyClasses", "HydrometeorClasses",
    "collapse_plane_device", "plane_filter_device", "PlaneTest", "colormap_lut", "colormap_rgba_device",
    "NativeUnavailable", "NativeError", "load_library",
]
