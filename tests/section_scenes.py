"""The scene of the vertical-section fixtures (tests/golden/g11_section_*.npz) and a brute-force float64 restatement of
a section for arbitrary points, shared by tests/golden/make_section_golden.py, tests/test_section_host.py and
tests/test_gpu_section.py.

The restatement is a loop over the points and ALL gates -- no search structure, no lattice: per point the reference's
float64 arithmetic (radar_grid/compute.py:46-47, 69-74, 82-87) over every toa-valid gate, level by level.
"""
import functools

import numpy as np

from oracle import radar_grid_oracle as oracle

VOLUME = dict(n_elev=12, n_az=180, n_gates=300, seed=31, max_range_m=120e3)
FIELDS = ("DBZH", "RHOHV")
QC = ("RHOHV", 0.8)
NZ = 21
Z_LIMITS = (0.0, 10000.0)
TOA = 17000.0
MIN_RADIUS = 250.0
BEAM_FACTOR = 0.01746
FILL = -9999.0
WEIGHTINGS = ("barnes2", "cressman", "nearest")
# name -> (vertices, spacing): a diagonal that misses the radar by ~25 km; a dog-leg THROUGH the radar (rows of 2000+
# neighbours there) whose last leg runs beyond the last gate
PATHS = {
    "diag": (((-100e3, -70e3), (90e3, 110e3)), 500.0),
    "dogleg": (((-60e3, 20e3), (0.0, 0.0), (30e3, -80e3), (125e3, -80e3)), 400.0),
}
# a lattice that holds both paths: the search structure of the GPU tests (its spacing has nothing to do with the paths')
GRID_SHAPE = (NZ, 40, 48)
GRID_LIMITS = (Z_LIMITS, (-85e3, 115e3), (-105e3, 130e3))


@functools.lru_cache(maxsize=1)
def volume():
    from radar_processor_amd import synthetic
    return synthetic.make_volume(fields=FIELDS, **VOLUME)


def path_points(name):
    import radar_processor_amd as rg
    vertices, spacing = PATHS[name]
    return rg.section_path(vertices, spacing)


def levels(z_limits=Z_LIMITS, nz=NZ):
    return oracle.axis_coords_f32(z_limits[0], z_limits[1], nz)


def brute_pairs(gate_x, gate_y, gate_z, xs, ys, zc, radar_altitude=0.0, min_radius=MIN_RADIUS, beam_factor=BEAM_FACTOR,
                toa=TOA):
    """Neighbour sets of the section at the float32 points (xs, ys) x the float32 levels zc: ``(indptr int64 [nz * n + 1],
    gate_indices int32, d2 float64, r2 float64)`` per pair, row ``k * n + i``, every row in ascending gate order.  Per
    point the horizontal part ``dx*dx + dy*dy`` is evaluated over ALL toa-valid gates; the levels then look only at the
    gates whose horizontal part is below the column's largest ``r2`` (``d2 >= dx*dx + dy*dy``: no other gate can pass
    ``d2 < r2``), with the full sum formed in compute.py:72's order."""
    z_rel, valid = oracle.gate_validity(np.asarray(gate_z), radar_altitude, toa)
    gidx = np.nonzero(valid)[0]
    gx = np.asarray(gate_x)[gidx].astype(np.float64)
    gy = np.asarray(gate_y)[gidx].astype(np.float64)
    gz = np.asarray(z_rel)[gidx].astype(np.float64)
    xs64, ys64 = np.asarray(xs, dtype=np.float32).astype(np.float64), np.asarray(ys, dtype=np.float32).astype(np.float64)
    zc64 = np.asarray(zc, dtype=np.float32).astype(np.float64)
    n, nz = len(xs64), len(zc64)
    rows = [[None] * n for _ in range(nz)]
    for i in range(n):
        x, y = xs64[i], ys64[i]
        dx, dy = gx - x, gy - y
        dxy2 = dx * dx + dy * dy                                  # over ALL valid gates
        r_col = np.maximum(min_radius, np.sqrt(x * x + y * y + zc64 * zc64) * beam_factor)    # compute.py:46-47
        near = np.nonzero(dxy2 < (r_col * r_col).max())[0]
        for k in range(nz):
            r2 = r_col[k] * r_col[k]
            dz = gz[near] - zc64[k]
            d2 = dxy2[near] + dz * dz                             # compute.py:72: (dx*dx + dy*dy) + dz*dz
            hit = np.nonzero(d2 < r2)[0]                          # compute.py:74
            rows[k][i] = (gidx[near[hit]].astype(np.int32), d2[hit], np.full(hit.size, r2))
    flat = [rows[k][i] for k in range(nz) for i in range(n)]
    indptr = np.concatenate([[0], np.cumsum([len(r[0]) for r in flat])]).astype(np.int64)
    return (indptr, np.concatenate([r[0] for r in flat]).astype(np.int32), np.concatenate([r[1] for r in flat]),
            np.concatenate([r[2] for r in flat]))


def brute_section(gate_x, gate_y, gate_z, xs, ys, zc, weighting, exact_weights=False, **kw):
    """CSR of the section: :func:`brute_pairs` with the weights of compute.py:82-87 -- their float32 roundings, or with
    ``exact_weights`` the float64 values before that rounding (the ``w`` of oracle.voxel_stats)."""
    indptr, idx, d2, r2 = brute_pairs(gate_x, gate_y, gate_z, xs, ys, zc, **kw)
    w = oracle.roi_weight_f64(d2, r2, weighting)
    return indptr, idx, w if exact_weights else w.astype(np.float32)


@functools.lru_cache(maxsize=4)
def scene_pairs(name):
    """brute_pairs of a fixture path over the fixture volume (cached: the sets do not depend on the weighting)."""
    vol = volume()
    xs, ys, _ = path_points(name)
    return brute_pairs(vol.gate_x, vol.gate_y, vol.gate_z, xs, ys, levels())


def scene_weights(name, weighting, exact=True):
    _, _, d2, r2 = scene_pairs(name)
    w = oracle.roi_weight_f64(d2, r2, weighting)
    return w if exact else w.astype(np.float32)


def fixture(weighting):
    """(meta, arrays) of g11_section_<weighting>; the non-Barnes files take gate_indices from the Barnes one."""
    from conftest import load_golden
    meta, arrays = load_golden(f"g11_section_{weighting}")
    if weighting != "barnes2":
        _, sib = load_golden("g11_section_barnes2")
        for name in PATHS:
            arrays.setdefault(f"{name}_gate_indices", sib[f"{name}_gate_indices"])
    return meta, arrays


def field_and_masks(vol, name):
    """values, plain mask, mask with the QC filter folded in"""
    data, mask = oracle.merge_masks(vol.fields[name])
    qc = oracle.gate_mask("below", np.ma.getdata(vol.fields[QC[0]]).ravel(), QC[1])
    return data, mask, mask | qc
