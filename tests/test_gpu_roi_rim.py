"""The ROI neighbour search at the rim: gates planted (oracle/roi_rim.py) where the float32 decisions of
``roi_block_kernel`` (csrc/rg_roi_grid.hip) meet the reference's float64 ``d2 < r2`` -- the 2e-6 band, the float32
Cressman weight, exact ``d2 == r2``, the band's own float32 edges -- on every position of a 4 x 4 voxel block and of a
16 x 4 patch, ragged blocks, first and last levels, grid corners and faces, the radar's vertical and the toa cut.

Both users of the kernel are checked against the float64 oracle: the geometry builder (count / fill modes) must return
the oracle's CSR (same index sets, Cressman and uniform weights bit for bit, Barnes within one ulp) and the CSR-free
gridder (grid mode) its NaN pattern and values (rtol 1e-5 with the ATOL_FRAC floor).  Every gridded value must lie
within the range of its voxel's unmasked neighbour values (a weighted mean with positive weights cannot leave it).
Each run also asserts how many planted gates of every case it covered, so a drifting generator cannot make it pass
vacuously."""
import functools

import numpy as np
import pytest

from conftest import ATOL_FRAC
from oracle import radar_grid_oracle as oracle
from oracle import roi_rim

pytestmark = pytest.mark.gpu

WEIGHTINGS = ("barnes2", "cressman", "nearest")

# Voxel spacing > 2 r_max on both: a planted gate belongs to the neighbourhood of its own voxel only.
#   minr -- min_radius dominates (r = 1000 m exactly, integer voxel centres: case D via Pythagorean offsets); nx = 37 is
#           two full 16 x 4 patches and a ragged one (5 voxels: a full 4 x 4 block and a 1-wide one), ny = 9 a 1-row block
#   beam -- r = 0.05 |v| (irrational, different for every voxel of a block; integer where |v| is), min_radius only at
#           the voxel nearest the radar; nx = 19 leaves a 3-wide block, ny = 5 a 1-row one
GEOMS = {
    "minr": dict(shape=(3, 9, 37), limits=((500.0, 5500.0), (-10e3, 10e3), (-45e3, 45e3)), min_radius=1000.0,
                 beam_factor=0.0, need=dict(A=100, B=100, C=40, D=100, E=100)),
    "beam": dict(shape=(3, 5, 19), limits=((1000.0, 9000.0), (-8e3, 8e3), (-36e3, 36e3)), min_radius=100.0,
                 beam_factor=0.05, need=dict(A=50, B=50, C=20, D=5, E=50)),
}


@pytest.fixture(scope="module")
def rg():
    import radar_processor_amd as pkg
    pkg.load_library()
    return pkg


@functools.lru_cache(maxsize=8)
def _rim(name, seed=1, outward=False):
    g = GEOMS[name]
    return roi_rim.rim_cloud(g["shape"], g["limits"], g["min_radius"], g["beam_factor"], seed=seed, outward=outward)


def _assert_coverage(cloud, need):
    counts = cloud.counts()
    print(f"rim cases covered: {counts} ({len(cloud)} planted gates)")
    assert cloud.misses == 0
    for case, n in need.items():
        assert counts[case] >= n, f"case {case}: {counts[case]} planted gates, the test needs {n} ({counts})"


def _values_and_mask(cloud_voxel, n, seed):
    """Distinct values; in about a third of the voxels with two or more planted gates one of them is masked, plus a
    sprinkle of masked gates anywhere else (n - len(cloud_voxel) background gates follow the planted ones)."""
    rng = np.random.default_rng(seed)
    val = (rng.permutation(n) * 0.37 - 40.0).astype(np.float32)
    mask = np.zeros(n, dtype=bool)
    vox = np.asarray(cloud_voxel)
    for v in np.unique(vox):
        idx = np.nonzero(vox == v)[0]
        if idx.size >= 2 and rng.random() < 0.35:
            mask[idx[rng.integers(idx.size)]] = True
    mask[len(vox):] = rng.random(n - len(vox)) < 0.15
    return val, mask


def _neighbour_range(ip, idx, val, mask):
    """Per voxel: [min, max] of the unmasked neighbour values (NaN where there is none)."""
    n_vox = ip.shape[0] - 1
    lo = np.full(n_vox, np.nan); hi = np.full(n_vox, np.nan)
    keep = ~mask[idx]
    row = np.repeat(np.arange(n_vox), np.diff(ip))[keep]
    v = val[idx][keep].astype(np.float64)
    if row.size:
        lo_r = np.full(n_vox, np.inf); hi_r = np.full(n_vox, -np.inf)
        np.minimum.at(lo_r, row, v); np.maximum.at(hi_r, row, v)
        has = np.isfinite(lo_r)
        lo[has] = lo_r[has]; hi[has] = hi_r[has]
    return lo, hi


def _check_grid(got, want, ip, idx, val, mask, label):
    """NaN pattern and values against the float64-summed oracle; every value inside its neighbours' range."""
    got = np.asarray(got, dtype=np.float32).ravel()
    want = np.asarray(want, dtype=np.float32).ravel()
    lo, hi = _neighbour_range(ip, idx, val, mask)
    nan_diff = int(np.count_nonzero(np.isnan(got) != np.isnan(want)))
    fin = np.isfinite(got) & np.isfinite(lo)
    slack = 1e-6 * np.maximum(np.abs(lo), np.abs(hi))
    out_range = int(np.count_nonzero(fin & ((got < lo - slack) | (got > hi + slack))))
    assert nan_diff == 0 and out_range == 0, (
        f"{label}: {nan_diff} voxels with a different NaN pattern ({int(np.count_nonzero(np.isnan(got) & ~np.isnan(want)))} "
        f"NaN where the oracle has a value), {out_range} values outside their neighbours' range, of {got.size} voxels "
        f"({int(np.count_nonzero(~np.isnan(want)))} with a value)")
    good = val[~mask]
    atol = ATOL_FRAC * float(np.abs(good[np.isfinite(good)]).max()) if good.size else 0.0
    np.testing.assert_allclose(got, want, rtol=1e-5, atol=atol, equal_nan=True, err_msg=label)


def _check_csr(csr, o_ip, o_idx, o_w, weighting, label):
    ip, idx, w = oracle.canonical_rows(csr.indptr.cpu().numpy(), csr.gate_indices.cpu().numpy(), csr.weights.cpu().numpy())
    np.testing.assert_array_equal(ip, o_ip, err_msg=label)
    np.testing.assert_array_equal(idx, o_idx, err_msg=label)
    if weighting == "barnes2":
        assert np.abs(w.view(np.int32).astype(np.int64) - o_w.view(np.int32).astype(np.int64)).max(initial=0) <= 1, label
    else:
        np.testing.assert_array_equal(w.view(np.int32), o_w.view(np.int32), err_msg=label)


def _run(rg, gx, gy, gz, fields, masks, shape, limits, weighting, searches, shared_mask=None, **kw):
    """Oracle vs the builder and the CSR-free gridder for every RoiSearch variant in ``searches`` (dicts of RoiSearch
    keywords).  ``fields`` / ``masks``: lists of per-gate arrays (the fused gridder grids them in one call)."""
    import torch
    dev = torch.device("cuda", 0)
    o_ip, o_idx, o_w = oracle.build_geometry(gx, gy, gz, shape, limits, weighting=weighting, **kw)
    assert o_idx.size > 0
    merged = [m | shared_mask if shared_mask is not None else m for m in masks]
    wants = [oracle.csr_apply_f64(o_ip, o_idx, o_w, v, m, shape) for v, m in zip(fields, merged)]
    f_t = [torch.from_numpy(np.ascontiguousarray(v)).to(dev) for v in fields]
    m_t = [torch.from_numpy(m.astype(np.uint8)).to(dev) for m in masks]
    s_t = None if shared_mask is None else torch.from_numpy(shared_mask.astype(np.uint8)).to(dev)
    for skw in searches:
        label = f"{weighting} {skw}"
        search = rg.RoiSearch(gx, gy, gz, shape, limits, device=dev, **kw, **skw)
        if "per_level" in skw:
            assert search.per_level == skw["per_level"]
        _check_csr(search.build_csr(weighting), o_ip, o_idx, o_w, weighting, label)
        out = rg.roi_grid_fields_device(search, f_t, m_t, shared_mask=s_t, weighting=weighting).cpu().numpy()
        for i, (want, v, m) in enumerate(zip(wants, fields, merged)):
            _check_grid(out[i], want, o_ip, o_idx, v, m, f"{label} field {i}")
    return o_ip, o_idx, o_w


SEARCHES = (dict(), dict(per_level=False), dict(per_level=True, cell_size=1.0), dict(per_level=False, cell_size=1.0))


# ---- 1. rim shells -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("weighting", WEIGHTINGS)
@pytest.mark.parametrize("geom", sorted(GEOMS))
def test_rim_shells(rg, geom, weighting):
    """Only planted rim gates (0-3 per voxel, one of them masked in some voxels), every voxel of the grid planted: the
    builder returns the oracle's CSR and the fused gridder its grid, per-level lists or one list, default or tiny cells
    (cell_size is clamped to span / 4000, about 23 m: cell boundaries everywhere along the rims)."""
    g = GEOMS[geom]
    cloud = _rim(geom)
    _assert_coverage(cloud, g["need"])
    val, mask = _values_and_mask(cloud.voxel, len(cloud), seed=3)
    o_ip, o_idx, _ = _run(rg, cloud.gx, cloud.gy, cloud.gz, [val], [mask], g["shape"], g["limits"], weighting, SEARCHES,
                          min_radius=g["min_radius"], beam_factor=g["beam_factor"])
    # the planted labels are what the oracle sees: A / B inside, C / D outside (E on either side)
    n_vox = o_ip.shape[0] - 1
    row = np.repeat(np.arange(n_vox), np.diff(o_ip))
    member = set(zip(row.tolist(), o_idx.tolist()))
    pair_in = np.array([(int(v), i) in member for i, v in enumerate(cloud.voxel)])
    assert pair_in[np.isin(cloud.case, ["A", "B"])].all()
    assert not pair_in[np.isin(cloud.case, ["C", "D"])].any()
    # voxels whose only unmasked neighbour is a case-A gate (float32 Cressman weight <= 0) exist in the run
    only = np.zeros(n_vox, dtype=np.int64)
    np.add.at(only, cloud.voxel[pair_in & ~mask], 1)
    a_only = [v for v in np.unique(cloud.voxel[(cloud.case == "A") & ~mask]) if only[v] == 1]
    assert len(a_only) >= 10


# ---- 2. the same shells in a dense random background -----------------------------------------------------------------
@pytest.mark.parametrize("weighting", WEIGHTINGS)
@pytest.mark.parametrize("geom", sorted(GEOMS))
def test_rim_shells_in_dense_background(rg, geom, weighting):
    """The rim gates share cell rings and candidate steps with ordinary gates; the block pre-filter sees 16 different
    radii in one block (beam) and survivors that are neighbours of some voxels of the block only."""
    g = GEOMS[geom]
    cloud = _rim(geom, seed=7)
    _assert_coverage(cloud, g["need"])
    rng = np.random.default_rng(11)
    (z0, z1), (y0, y1), (x0, x1) = g["limits"]
    n_bg = 30000
    bx = rng.uniform(x0 - 2e3, x1 + 2e3, n_bg).astype(np.float32)
    by = rng.uniform(y0 - 2e3, y1 + 2e3, n_bg).astype(np.float32)
    bz = rng.uniform(z0 - 2e3, z1 + 2e3, n_bg).astype(np.float32)
    gx = np.concatenate([cloud.gx, bx]); gy = np.concatenate([cloud.gy, by]); gz = np.concatenate([cloud.gz, bz])
    order = rng.permutation(gx.size)               # planted gates anywhere in the index order
    val, mask = _values_and_mask(cloud.voxel, gx.size, seed=5)
    _run(rg, gx[order], gy[order], gz[order], [val[order]], [mask[order]], g["shape"], g["limits"], weighting,
         SEARCHES[:3], min_radius=g["min_radius"], beam_factor=g["beam_factor"])


# ---- 3. edges of the search structure ------------------------------------------------------------------------------
@pytest.mark.parametrize("weighting", WEIGHTINGS)
@pytest.mark.parametrize("geom", sorted(GEOMS))
def test_rim_gates_beyond_the_grid_faces(rg, geom, weighting):
    """Voxels on a face, edge or corner of the grid get their rim gates outside the grid's x / y / z extent (the cell grid
    and its z range are padded by r_max only)."""
    g = GEOMS[geom]
    cloud = _rim(geom, seed=13, outward=True)
    _assert_coverage(cloud, {c: n // 2 for c, n in g["need"].items()})
    nz, ny, nx = g["shape"]
    zc, yc, xc = roi_rim.voxel_centres(g["shape"], g["limits"])
    outside = ((cloud.gx < xc.min()) | (cloud.gx > xc.max()) | (cloud.gy < yc.min()) | (cloud.gy > yc.max())
               | (cloud.gz < zc.min()) | (cloud.gz > zc.max()))
    assert np.count_nonzero(outside & np.isin(cloud.case, ["A", "B"])) >= 50
    val, mask = _values_and_mask(cloud.voxel, len(cloud), seed=17)
    _run(rg, cloud.gx, cloud.gy, cloud.gz, [val], [mask], g["shape"], g["limits"], weighting, SEARCHES,
         min_radius=g["min_radius"], beam_factor=g["beam_factor"])


@pytest.mark.parametrize("weighting", WEIGHTINGS)
@pytest.mark.parametrize("beam_factor", [0.05, 0.3])
def test_rim_gates_on_the_radar_vertical(rg, weighting, beam_factor):
    """Gates straight above and below voxels on the radar's vertical, just inside and just outside a beam-dominated
    rim: the gate below sits at |g| = |v| - r, where the per-level lists' reach bound R_g = bf |g| / (1 - bf) equals r."""
    shape, limits = (5, 3, 3), ((2345.6, 9876.5), (-6e3, 6e3), (-6e3, 6e3))
    vert = [iz * 9 + 4 for iz in range(shape[0])]          # (iz, 1, 1): x = y = 0
    cloud = roi_rim.vertical_cloud(shape, limits, 100.0, beam_factor, vert)
    assert np.all(cloud.gx == 0) and np.all(cloud.gy == 0)
    val, mask = _values_and_mask(np.full(len(cloud), -1), len(cloud), seed=19)
    mask[:] = False
    o_ip, o_idx, _ = _run(rg, cloud.gx, cloud.gy, cloud.gz, [val], [mask], shape, limits, weighting,
                          SEARCHES + (dict(per_level=True, cell_size=5000.0),), min_radius=100.0,
                          beam_factor=beam_factor)
    # every 'just inside' gate is a neighbour of its voxel, no 'just outside' gate is
    row = np.repeat(np.arange(o_ip.shape[0] - 1), np.diff(o_ip))
    member = set(zip(row.tolist(), o_idx.tolist()))
    inside = np.array([k % 2 == 0 for k in range(len(cloud))])           # vertical_cloud: '<' then '>' per direction
    pair_in = np.array([(int(v), i) in member for i, v in enumerate(cloud.voxel)])
    np.testing.assert_array_equal(pair_in, inside)


@pytest.mark.parametrize("weighting", WEIGHTINGS)
def test_toa_cut_at_the_float32_boundary(rg, weighting):
    """Gates whose float32 ``gate_z - radar_altitude`` is exactly ``toa`` are kept, one ulp above it are dropped
    (compute.py:182,193), with a radar altitude that is not a float32 value, next to rim gates of the top level."""
    rng = np.random.default_rng(23)
    alt, toa = 437.3, 4500.0        # toa and toa + alt in one binade: stepping gz by one ulp steps z - alt by one
    alt32, toa32 = np.float32(alt), np.float32(toa)
    shape, limits = (2, 5, 21), ((3000.0, 4000.0), (-10e3, 10e3), (-25e3, 25e3))
    n = 4000
    gx = rng.uniform(-26e3, 26e3, n).astype(np.float32)
    gy = rng.uniform(-11e3, 11e3, n).astype(np.float32)
    # absolute heights around toa + altitude: walk the float32 lattice until z - alt rounds to toa / to the next float
    base = np.float32(toa + alt)
    cand = roi_rim._ulp_steps(base, 64)
    zrel = cand - alt32
    at = cand[zrel == toa32]
    above = cand[zrel == np.nextafter(toa32, np.float32(np.inf))]
    assert at.size and above.size
    kind = rng.integers(0, 3, n)                 # 0: exactly toa, 1: one ulp above, 2: ordinary height below
    gz = np.where(kind == 0, at[rng.integers(at.size, size=n)],
                  np.where(kind == 1, above[rng.integers(above.size, size=n)],
                           rng.uniform(2000.0, 4400.0, n).astype(np.float32) + alt32)).astype(np.float32)
    val, mask = _values_and_mask(np.zeros(0, dtype=np.int64), n, seed=29)
    o_ip, o_idx, _ = _run(rg, gx, gy, gz, [val], [mask], shape, limits, weighting, SEARCHES[:3],
                          radar_altitude=alt, toa=toa, min_radius=1500.0, beam_factor=0.0)
    assert np.isin(np.nonzero(kind == 0)[0], o_idx).sum() >= 100       # gates at toa are neighbours ...
    assert not np.isin(np.nonzero(kind == 1)[0], o_idx).any()           # ... one ulp above never are


# ---- 4. several fields and a shared mask on one rim geometry ---------------------------------------------------------
@pytest.mark.parametrize("weighting", WEIGHTINGS)
@pytest.mark.parametrize("n_fields", [2, 3, 5])
def test_rim_shells_multi_field(rg, n_fields, weighting):
    """2 / 3 / 5 fields (value ring with 2 slots, gather per hit with 4 and 8 slots), field masks and a shared mask."""
    g = GEOMS["minr"]
    cloud = _rim("minr")
    _assert_coverage(cloud, g["need"])
    fields, masks = [], []
    for k in range(n_fields):
        v, m = _values_and_mask(cloud.voxel, len(cloud), seed=31 + k)
        fields.append(v); masks.append(m)
    shared = np.random.default_rng(37).random(len(cloud)) < 0.1
    _run(rg, cloud.gx, cloud.gy, cloud.gz, fields, masks, g["shape"], g["limits"], weighting, SEARCHES[:2],
         shared_mask=shared, min_radius=g["min_radius"], beam_factor=g["beam_factor"])
