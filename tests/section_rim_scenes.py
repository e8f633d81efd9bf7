"""Scenes for the section kernel (csrc/rg_roi_section.hip) at the ROI rim and on adversarial point sets, shared by
tests/test_section_rim_scenes.py (CPU) and tests/test_gpu_section_rim.py (a helper module: pytest does not collect it).

A scene is a handful of section points, a few levels, an ROI rule and the lattice of a ``RoiSearch`` whose rectangle holds
the points.  Its gates are PLANTED (oracle/roi_rim.py, ``point_cloud``): float32 gates nudged by ulps around the rim of
every sample ``(xs[i], ys[i], zc[k])`` until the kernel's float32 distance and the reference's float64 ``d2 < r2`` fall
where a labelled case (A-E) wants them.  The truth of every scene is ``section_scenes.brute_pairs``: a float64 loop over
all gates without a search structure, with ``min_radius``, ``beam_factor`` and ``toa`` passed explicitly.

What the scenes are for (one wavefront of the kernel = a BLOCK of 4 consecutive points of one level):

  sparse_minr  37 integer points 2.5 km apart, r = 1000 m exactly: a planted gate belongs to its own sample only; exact
               ``d2 == r2`` (case D); 37 mod 4 = 1
  sparse_beam  19 non-integer points 4.1 km apart, r = 0.05 |p|: the four points of a block have four irrational radii; 19 mod 4 = 3
  dense_minr   41 integer points 75 m apart, r = 1000 m: the points of a block share almost all candidates, and a gate on
               point 0's rim lies well inside or outside point 3's
  dense_beam   42 points 78 m apart at 25 km, r = 0.05 |p|; 42 mod 4 = 2
  scattered    the points of sparse_beam and dense_beam under a fixed permutation: every full block spans 20 km or more, so
               its cell box is most of the rectangle and only the sub-boxes of the pre-filter save it
  duplicates   a point of dense_minr repeated 4 times (a whole block) and 5 times (across a block seam)
  edges        points ON the corners and edge midpoints of the search's rectangle (or of a window's), their gates planted
               outward; and the point (0, 0) with gates straight above and below it
"""
import dataclasses
import functools
from typing import Optional, Tuple

import numpy as np

import section_scenes as sc
from oracle import radar_grid_oracle as oracle
from oracle import roi_rim

TOA = 17000.0
WEIGHTINGS = ("barnes2", "cressman", "nearest")
KPTS = 4                                            # points per block of the section kernel (kPts)
MAIN = ("sparse_minr", "sparse_beam", "dense_minr", "dense_beam", "scattered", "duplicates")
SPARSE = ("sparse_minr", "sparse_beam")
DENSE = ("dense_minr", "dense_beam")
EDGE_KINDS = ("whole", "window")
EDGE_BEAM_FACTORS = (0.05, 0.3)
EDGES = tuple(f"edges_{kind}_{bf}" for kind in EDGE_KINDS for bf in EDGE_BEAM_FACTORS)


@dataclasses.dataclass(frozen=True)
class Scene:
    name: str
    xs: np.ndarray                                  # float32 [n]
    ys: np.ndarray
    z_limits: Tuple[float, float]
    nz: int
    min_radius: float
    beam_factor: float
    grid_shape: Tuple[int, int, int]                # the RoiSearch's lattice: its rectangle (or its window's) holds the points
    grid_limits: tuple
    need: dict                                      # planted gates per case a run must cover (a condition, not a measurement)
    seed: int = 1
    per_sample: Tuple[int, ...] = (1, 2, 3)
    direction: Optional[tuple] = None               # per point: None or 'out:<signs>' (roi_rim.plant)
    window: Optional[Tuple[int, int, int, int]] = None
    vertical: Tuple[int, ...] = ()                  # points that also get gates straight above and below every sample

    @property
    def n(self) -> int:
        return int(self.xs.shape[0])

    @property
    def zc(self) -> np.ndarray:
        return oracle.axis_coords_f32(self.z_limits[0], self.z_limits[1], self.nz)

    @property
    def roi(self) -> dict:
        return dict(min_radius=self.min_radius, beam_factor=self.beam_factor, toa=TOA)

    def radius(self) -> np.ndarray:
        """float64 [nz, n]: every sample's radius of influence (compute.py:46-47)"""
        x, y, z = self.xs.astype(np.float64)[None, :], self.ys.astype(np.float64)[None, :], self.zc.astype(np.float64)[:, None]
        return np.maximum(self.min_radius, np.sqrt(x * x + y * y + z * z) * self.beam_factor)


def _f32(a) -> np.ndarray:
    return np.asarray(a, dtype=np.float64).astype(np.float32)


# ---- the point sets ------------------------------------------------------------------------------------------------------------
def _sparse_minr_points():
    i = np.arange(37)
    return _f32(-45000.0 + 2500.0 * i), _f32(-9000.0 + 500.0 * i)


def _sparse_beam_points():
    i = np.arange(19)
    return _f32(-36000.0 + 4000.37 * i), _f32(-8000.0 + 888.9 * i)


def _dense_minr_points():
    i = np.arange(41)
    return _f32(3000.0 + 60.0 * i), _f32(-1000.0 + 45.0 * i)           # 75 m apart


def _dense_beam_points():
    i = np.arange(42)
    return _f32(-3000.13 + 62.4 * i), _f32(24800.7 + 46.8 * i)         # 78 m apart, 25 - 26.7 km from the radar


def _scattered_order() -> np.ndarray:
    """The fixed permutation of sparse_beam's points (0 .. 18) followed by dense_beam's (19 .. 60): fifteen full blocks of
    one or two sparse points and dense ones (every dense point is 20 km or more from every sparse one), each block's points
    in an order of its own, and a last block of one dense point."""
    rng = np.random.default_rng(4)
    sparse, dense = list(range(19)), list(range(19, 61))
    blocks = []
    for b in range(15):
        # four blocks pair a sparse point far from the radar with one near it (radii 18 to 1), the others hold one
        own = [sparse.pop(0), sparse.pop(len(sparse) // 2)] if b < 4 else [sparse.pop(0)]
        own += [dense.pop(0) for _ in range(KPTS - len(own))]
        blocks.append(rng.permutation(own))
    assert not sparse and len(dense) == 1
    return np.concatenate(blocks + [np.array(dense)])


def _duplicate_points():
    """dense_minr's first points with point 5 four times in block 1 (indices 4 .. 7) and point 9 five times across the seam
    of blocks 2 and 3 (indices 10 .. 14): 18 points, 18 mod 4 = 2."""
    x, y = _dense_minr_points()
    pick = [0, 1, 2, 3, 5, 5, 5, 5, 6, 7, 9, 9, 9, 9, 9, 10, 11, 12]
    return x[pick], y[pick]


DUPLICATE_GROUPS = ((4, 5, 6, 7), (10, 11, 12, 13, 14))

_EDGE_SHAPE = (5, 7, 9)                              # 2 km columns and rows: (0, 0) is a column of the lattice
_EDGE_LIMITS = ((2345.6, 9876.5), (-6e3, 6e3), (-8e3, 8e3))
_EDGE_WINDOW = (1, 6, 2, 8)                          # y -4000 .. 4000, x -4000 .. 6000


def edge_rectangle(kind):
    """(x0, x1, y0, y1) of the edges scene's rectangle, as radar_processor_amd.section_rectangle returns it"""
    yc = np.linspace(_EDGE_LIMITS[1][0], _EDGE_LIMITS[1][1], _EDGE_SHAPE[1], dtype="float32")
    xc = np.linspace(_EDGE_LIMITS[2][0], _EDGE_LIMITS[2][1], _EDGE_SHAPE[2], dtype="float32")
    if kind == "window":
        yc, xc = yc[_EDGE_WINDOW[0]:_EDGE_WINDOW[1]], xc[_EDGE_WINDOW[2]:_EDGE_WINDOW[3]]
    return float(xc.min()), float(xc.max()), float(yc.min()), float(yc.max())


def _edge_points(kind):
    x0, x1, y0, y1 = edge_rectangle(kind)
    xm, ym = float(np.float32(0.5 * (x0 + x1))), float(np.float32(0.5 * (y0 + y1)))
    pts = [(x0, y0, "out:--."), (x1, y0, "out:+-."), (x0, y1, "out:-+."), (x1, y1, "out:++."),
           (xm, y0, "out:.-."), (xm, y1, "out:.+."), (x0, ym, "out:-.."), (x1, ym, "out:+.."), (0.0, 0.0, None)]
    return _f32([p[0] for p in pts]), _f32([p[1] for p in pts]), tuple(p[2] for p in pts)


@functools.lru_cache(maxsize=None)
def scene(name: str) -> Scene:
    # need: about half of what the committed seed yields, and at least A 20, B 20, C 10, E 20 (D 20 in the integer scenes)
    if name == "sparse_minr":
        xs, ys = _sparse_minr_points()
        return Scene(name, xs, ys, (500.0, 5500.0), 3, 1000.0, 0.0, (3, 9, 37), ((500.0, 5500.0), (-10e3, 10e3), (-45e3, 45e3)),
                     need=dict(A=22, B=25, C=10, D=21, E=26))
    if name == "sparse_beam":
        xs, ys = _sparse_beam_points()
        return Scene(name, xs, ys, (1000.0, 13000.0), 4, 100.0, 0.05, (4, 5, 19),
                     ((1000.0, 13000.0), (-9e3, 9e3), (-37e3, 37e3)), need=dict(A=31, B=38, C=14, E=32), per_sample=(2, 3, 4))
    if name == "dense_minr":
        xs, ys = _dense_minr_points()
        return Scene(name, xs, ys, (500.0, 2500.0), 3, 1000.0, 0.0, (3, 4, 5), ((500.0, 2500.0), (-2e3, 2e3), (2e3, 6e3)),
                     need=dict(A=21, B=29, C=20, D=27, E=25))
    if name == "dense_beam":
        xs, ys = _dense_beam_points()
        return Scene(name, xs, ys, (1000.0, 5000.0), 3, 100.0, 0.05, (3, 3, 4), ((1000.0, 5000.0), (24e3, 27.5e3), (-3.5e3, 0.5e3)),
                     need=dict(A=30, B=39, C=24, E=35))
    if name == "scattered":
        xs = np.concatenate([_sparse_beam_points()[0], _dense_beam_points()[0]])[_scattered_order()]
        ys = np.concatenate([_sparse_beam_points()[1], _dense_beam_points()[1]])[_scattered_order()]
        return Scene(name, xs, ys, (1000.0, 9000.0), 3, 100.0, 0.05, (3, 6, 9), ((1000.0, 9000.0), (-9e3, 27.5e3), (-37e3, 37e3)),
                     need=dict(A=45, B=43, C=27, E=57), seed=2)
    if name == "duplicates":
        xs, ys = _duplicate_points()
        return Scene(name, xs, ys, (500.0, 2500.0), 3, 1000.0, 0.0, (3, 4, 5), ((500.0, 2500.0), (-2e3, 2e3), (2e3, 6e3)),
                     need=dict(A=20, B=20, C=18, D=20, E=20), seed=3, per_sample=(2, 3, 4))
    if name in EDGES:
        _, kind, bf = name.split("_")
        xs, ys, direction = _edge_points(kind)
        return Scene(name, xs, ys, _EDGE_LIMITS[0], _EDGE_SHAPE[0], 100.0, float(bf), _EDGE_SHAPE, _EDGE_LIMITS,
                     need=dict(A=29, B=30, C=10, E=33), seed=5, per_sample=(4, 5, 6), direction=direction,
                     window=_EDGE_WINDOW if kind == "window" else None, vertical=(8,))
    raise KeyError(name)


# ---- the planted gates and the float64 truth ------------------------------------------------------------------------------------
def sample_rim(s: Scene, row: int) -> roi_rim.Rim:
    k, i = divmod(int(row), s.n)
    return roi_rim.voxel_rim(s.xs[i], s.ys[i], s.zc[k], s.min_radius, s.beam_factor)


def _vertical_gates(s: Scene):
    """As roi_rim.vertical_cloud for the lattice: per sample of the points ``s.vertical`` the innermost gate inside and
    the outermost gate outside the rim, straight above and straight below."""
    rng = np.random.default_rng(0)
    pts, rows, lab = [], [], []
    for k in range(s.nz):
        for i in s.vertical:
            rim = sample_rim(s, k * s.n + i)
            for d in ("up", "down"):
                for side in ("<", ">"):
                    g = roi_rim.plant(rim, side, rng, direction=d)
                    assert g is not None, (s.name, k, i, d, side)
                    pts.append(g); rows.append(k * s.n + i)
                    lab.append(roi_rim.classify(g[0:1], g[1:2], g[2:3], rim)[0])
    return np.array(pts, dtype=np.float32).reshape(-1, 3), np.array(rows, dtype=np.int64), np.array(lab, dtype="<U1")


@functools.lru_cache(maxsize=None)
def cloud(name: str) -> roi_rim.RimCloud:
    """The scene's gates: ``voxel`` is the row ``k * n + i`` of the sample a gate was planted for.  The vertical gates of
    an edges scene come last, four per sample (up <, up >, down <, down >)."""
    s = scene(name)
    c = roi_rim.point_cloud(s.xs, s.ys, s.zc, s.min_radius, s.beam_factor, s.seed, per_sample=s.per_sample,
                            direction=s.direction)
    if s.vertical:
        p, rows, lab = _vertical_gates(s)
        c = roi_rim.RimCloud(np.concatenate([c.gx, p[:, 0]]), np.concatenate([c.gy, p[:, 1]]), np.concatenate([c.gz, p[:, 2]]),
                             np.concatenate([c.voxel, rows]), np.concatenate([c.case, lab]), c.misses)
    return c


def n_vertical(name: str) -> int:
    s = scene(name)
    return 4 * s.nz * len(s.vertical)


@functools.lru_cache(maxsize=None)
def pairs(name: str):
    """section_scenes.brute_pairs of the scene's points over its planted gates: (indptr, gate_indices, d2, r2)"""
    s, c = scene(name), cloud(name)
    return sc.brute_pairs(c.gx, c.gy, c.gz, s.xs, s.ys, s.zc, radar_altitude=0.0, **s.roi)


def relabel(name: str) -> np.ndarray:
    """Every planted gate's label against its own sample, from scratch"""
    s, c = scene(name), cloud(name)
    return np.array([roi_rim.classify(c.gx[j:j + 1], c.gy[j:j + 1], c.gz[j:j + 1], sample_rim(s, c.voxel[j]))[0]
                     for j in range(len(c))], dtype="<U1")


def membership(indptr, gate_indices, n_gates: int) -> np.ndarray:
    """bool [rows, n_gates]: gate g is a neighbour of row v (for the tiny scenes only)"""
    indptr = np.asarray(indptr, dtype=np.int64)
    m = np.zeros((indptr.shape[0] - 1, n_gates), dtype=bool)
    m[np.repeat(np.arange(indptr.shape[0] - 1), np.diff(indptr)), np.asarray(gate_indices, dtype=np.int64)] = True
    return m


def own_membership(name: str) -> np.ndarray:
    """bool [gates]: the planted gate is a neighbour of the sample it was planted for"""
    c = cloud(name)
    ip, idx, _, _ = pairs(name)
    return membership(ip, idx, len(c))[c.voxel, np.arange(len(c))]


def split_within_block(name: str) -> int:
    """Planted gates that are neighbours of one point of their own block (at their own level) and not of another: the
    per-point decisions inside one wavefront."""
    s, c = scene(name), cloud(name)
    ip, idx, _, _ = pairs(name)
    m = membership(ip, idx, len(c))
    count = 0
    for j, row in enumerate(c.voxel):
        k, i = divmod(int(row), s.n)
        b0 = i // KPTS * KPTS
        col = m[k * s.n + b0:k * s.n + min(b0 + KPTS, s.n), j]
        count += int(col.any() and not col.all())
    return count


def a_only_samples(name: str, mask: np.ndarray) -> int:
    """Samples whose only unmasked neighbour is a case-A gate: a float32 Cressman weight would be <= 0 there"""
    c = cloud(name)
    ip, idx, _, _ = pairs(name)
    row = np.repeat(np.arange(ip.shape[0] - 1), np.diff(ip))
    live = ~np.asarray(mask, dtype=bool)[idx]
    n_live = np.bincount(row[live], minlength=ip.shape[0] - 1)
    lone = live & (n_live[row] == 1)
    return int(np.count_nonzero(c.case[idx[lone]] == "A"))


# ---- the conditions on the scattered scene -------------------------------------------------------------------------------------
def block_extents(s: Scene) -> np.ndarray:
    """float64 [blocks]: the largest distance between two points of every block of four"""
    x, y = s.xs.astype(np.float64), s.ys.astype(np.float64)
    out = []
    for b0 in range(0, s.n, KPTS):
        bx, by = x[b0:b0 + KPTS], y[b0:b0 + KPTS]
        out.append(float(np.hypot(bx[:, None] - bx[None, :], by[:, None] - by[None, :]).max()))
    return np.array(out)


def block_radius_ratios(s: Scene) -> np.ndarray:
    """float64 [nz, blocks]: largest over smallest radius of influence among the points of a block, level by level"""
    r = s.radius()
    return np.array([[r[k, b0:b0 + KPTS].max() / r[k, b0:b0 + KPTS].min() for b0 in range(0, s.n, KPTS)] for k in range(s.nz)])


def block_cell_rows(s: Scene, cell_size: float) -> np.ndarray:
    """float64 [blocks]: cell rows the kernel's box of a block covers at least (its y extent widened by the block's
    smallest radius at the lowest level), for a search with this ``cell_size``"""
    y = s.ys.astype(np.float64)
    r = s.radius()
    return np.array([(y[b0:b0 + KPTS].max() - y[b0:b0 + KPTS].min() + 2.0 * r[:, b0:b0 + KPTS].min()) / cell_size
                     for b0 in range(0, s.n, KPTS)])


# ---- a dense background ---------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def with_background(name: str, n_bg: int = 30000, seed: int = 11):
    """The scene's planted gates among ``n_bg`` uniform random ones confined to the path's bounding box padded by 2 r,
    under a permutation: ``(gx, gy, gz, where)`` with ``where[j]`` the position of planted gate j in the gate arrays."""
    s, c = scene(name), cloud(name)
    rng = np.random.default_rng(seed)
    pad = 2.0 * float(s.radius().max())
    bx = rng.uniform(float(s.xs.min()) - pad, float(s.xs.max()) + pad, n_bg).astype(np.float32)
    by = rng.uniform(float(s.ys.min()) - pad, float(s.ys.max()) + pad, n_bg).astype(np.float32)
    bz = rng.uniform(float(s.zc.min()) - pad, float(s.zc.max()) + pad, n_bg).astype(np.float32)
    gx, gy, gz = np.concatenate([c.gx, bx]), np.concatenate([c.gy, by]), np.concatenate([c.gz, bz])
    order = rng.permutation(gx.size)                                   # gate arrays = concatenation[order]
    where = np.empty(gx.size, dtype=np.int64)
    where[order] = np.arange(gx.size)
    return gx[order], gy[order], gz[order], where[:len(c)]


@functools.lru_cache(maxsize=None)
def background_pairs(name: str):
    s = scene(name)
    gx, gy, gz, _ = with_background(name)
    return sc.brute_pairs(gx, gy, gz, s.xs, s.ys, s.zc, radar_altitude=0.0, **s.roi)
