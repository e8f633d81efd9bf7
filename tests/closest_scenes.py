"""Seeded scenes for the closest-gate mode of ``rg_roi_grid_f32`` (``RG_W_CLOSEST``), shared by tests/test_closest_oracle.py
(CPU: the scenes exercise what they claim to) and tests/test_gpu_closest.py (GPU: the kernel against ``oracle.closest_gate_choice``
on every voxel).  A helper module: its name does not start with ``test_``, so pytest does not collect it.

Field values are INDEX-CODED, ``value[g] = float32(g)`` (exact below 2^24 gates), so a gridded value names the gate the
kernel chose.  Every scene is built once per process, and so is every oracle result (``Scene.choice``).

  polar_const  a polar volume on a grid centred on the radar (natural float32 ties on its symmetry lines), the constant
               ROI of the processor seam
  polar_beam   the same volume with a beam-dominated ROI that grows across the grid, a radar altitude and a toa cut
  ragged_a/b   dense random clouds on grids ragged against the kernel's 16 x 4 patch; voxels with far more than 256
               members, so the survivor ring wraps and drains many times per block
  ties         planted ties (duplicates, mirror pairs, three-way, across ring drains) and gates on voxel centres
  rim          roi_rim's planted rim gates (cases A-E) as the only gates near their voxels
"""
import dataclasses
import functools
from typing import List, Optional

import numpy as np

from oracle import radar_grid_oracle as oracle
from oracle import roi_rim
from radar_processor_amd import processor_seam, synthetic

N_MASKS = 11                       # field counts up to 11 = one full group of 8 and a group of 3
FIELD_COUNTS = (1, 2, 3, 4, 5, 8, 11)
SCENES = ("polar_const", "polar_beam", "ragged_a", "ragged_b", "ties", "rim")


@dataclasses.dataclass
class Tie:
    """One planted group of the ``ties`` scene: ``tied`` = gate indices (ascending) that share the smallest float32 d2 of
    voxel ``voxel`` (flat index); ``other`` = the runner-up of a 'centre' group (-1 otherwise)."""
    kind: str
    voxel: int
    tied: tuple
    other: int = -1


@dataclasses.dataclass
class Scene:
    name: str
    gx: np.ndarray
    gy: np.ndarray
    gz: np.ndarray                 # as handed to RoiSearch: radar_altitude is still in it
    shape: tuple
    limits: tuple
    min_radius: float
    beam_factor: float
    radar_altitude: float = 0.0
    toa: float = float("inf")
    seed: int = 0
    ties: Optional[List[Tie]] = None
    rim_voxel: Optional[np.ndarray] = None      # rim scene: the voxel every gate was planted for
    special_masks: Optional[dict] = None        # field number -> mask, where the scene plants its own

    @property
    def n_gates(self) -> int:
        return int(self.gx.shape[0])

    @property
    def n_vox(self) -> int:
        return int(np.prod(self.shape))

    def search_kw(self) -> dict:
        return dict(min_radius=self.min_radius, beam_factor=self.beam_factor, radar_altitude=self.radar_altitude, toa=self.toa)

    def values(self) -> np.ndarray:
        assert self.n_gates < 2 ** 24
        return np.arange(self.n_gates, dtype=np.float32)

    def mask(self, k: int) -> Optional[np.ndarray]:
        """Field k's exclusion mask: ``None`` for odd k, a seeded mask of its own for even k."""
        if self.special_masks and k in self.special_masks:
            return self.special_masks[k]
        if k % 2:
            return None
        return np.random.default_rng([self.seed, 7, k]).random(self.n_gates) < 0.2

    def masks(self, n: int = N_MASKS) -> list:
        return [self.mask(k) for k in range(n)]

    def shared_mask(self) -> np.ndarray:
        return np.random.default_rng([self.seed, 8]).random(self.n_gates) < 0.15

    def choice_for(self, masks, key) -> dict:
        return oracle.closest_gate_choice(self.gx, self.gy, self.gz, masks, self.shape, self.limits, self.min_radius,
                                          self.beam_factor, radar_altitude=self.radar_altitude, toa=self.toa,
                                          cache_key=("closest_scenes", self.name, key))

    def choice(self) -> dict:
        """The oracle for ``masks(N_MASKS)``: field count n uses its first n fields."""
        return self.choice_for(self.masks(), "fields")

    def choice_shared(self, n: int = 3) -> dict:
        """... for the first n masks OR-ed with ``shared_mask()``."""
        sh = self.shared_mask()
        return self.choice_for([sh if m is None else (m | sh) for m in self.masks(n)], ("shared", n))

    def real_values(self):
        """(values, specials) for the bit-transport check: normal data, and -0.0, a subnormal, +inf, -inf and NaN planted on
        gates that win somewhere in field 1 (nothing excluded).  ``specials``: {name: gate index}."""
        rng = np.random.default_rng([self.seed, 9])
        val = rng.normal(20.0, 10.0, self.n_gates).astype(np.float32)
        winners = np.unique(self.choice()["idx32"][1])
        winners = winners[winners >= 0]
        assert winners.size >= 5, self.name
        pick = winners[np.linspace(0, winners.size - 1, 5).astype(int)]
        names = ("neg_zero", "subnormal", "pos_inf", "neg_inf", "nan")
        planted = np.array([-0.0, 1e-40, np.inf, -np.inf, np.nan], dtype=np.float32)
        val[pick] = planted
        return val, dict(zip(names, (int(p) for p in pick)))


# ---- polar volumes --------------------------------------------------------------------------------------------------------
POLAR = dict(n_elev=6, n_az=120, n_gates=200)
POLAR_RES = 1000.0
POLAR_Z, POLAR_Y, POLAR_X = (0.0, 4000.0), (-11500.0, 11500.0), (-18500.0, 18500.0)     # the seam's (5, 23, 37) grid
POLAR_MAX_RANGE = 30000.0


@functools.lru_cache(maxsize=None)
def _polar_gates():
    elev, az, rng_m = synthetic.sweep_geometry(POLAR["n_elev"], POLAR["n_az"], POLAR["n_gates"], max_range_m=POLAR_MAX_RANGE)
    return synthetic.gate_coordinates(elev, az, rng_m)


def _polar_const() -> Scene:
    gx, gy, gz = _polar_gates()
    shape = processor_seam.grid3d_shape(POLAR_Z, POLAR_Y, POLAR_X, POLAR_RES)
    return Scene("polar_const", gx, gy, gz, shape, (POLAR_Z, POLAR_Y, POLAR_X),
                 min_radius=processor_seam.constant_roi_for(POLAR_RES, POLAR_Y), beam_factor=0.0, seed=101)


def _polar_beam() -> Scene:
    gx, gy, gz = _polar_gates()
    alt = 137.3
    return Scene("polar_beam", gx, gy, (gz + np.float32(alt)).astype(np.float32), (4, 21, 38),
                 ((200.0, 2600.0), (-12e3, 12e3), (-20e3, 17e3)), min_radius=120.0, beam_factor=0.06, radar_altitude=alt,
                 toa=900.0, seed=102)


# ---- dense clouds on ragged grids ---------------------------------------------------------------------------------------
def _ragged(name, shape, limits, n, box, min_radius, beam_factor, seed) -> Scene:
    rng = np.random.default_rng(seed)
    (x0, x1), (y0, y1), (z0, z1) = box
    gx = rng.uniform(x0, x1, n).astype(np.float32)
    gy = rng.uniform(y0, y1, n).astype(np.float32)
    gz = rng.uniform(z0, z1, n).astype(np.float32)
    return Scene(name, gx, gy, gz, shape, limits, min_radius=min_radius, beam_factor=beam_factor, seed=seed)


def _ragged_a() -> Scene:       # the cloud ends at x = 4 km: the columns beyond its reach stay empty
    return _ragged("ragged_a", (3, 9, 70), ((500.0, 6000.0), (-3e3, 9e3), (-15e3, 15e3)), 40000,
                   ((-19e3, 4e3), (-6e3, 12e3), (-2e3, 8.5e3)), 2500.0, 0.0, 103)


def _ragged_b() -> Scene:       # one level, beam-dominated radii from 0.9 to 2.3 km
    return _ragged("ragged_b", (1, 7, 63), ((1500.0, 1500.0), (-4e3, 8e3), (-15e3, 15e3)), 45000,
                   ((-3e3, 18e3), (-7e3, 11e3), (-1e3, 4e3)), 900.0, 0.15, 104)


# ---- planted ties -------------------------------------------------------------------------------------------------------
TIE_KINDS = ("dup", "mirror_y", "mirror_x", "three", "centre", "dup_centre")
TIES_FAR_VOXELS = {45: +1, 131: -1, 214: +1, 307: -1}      # voxel -> side (sign of y) of the LOWER tied index
TIES_FAR_FILLERS = 300


def _ties() -> Scene:
    """Integer voxel centres 1 km apart and a constant 600 m ROI: a planted gate (at most 350 m from its voxel) is a member of
    that voxel only.  Every voxel gets one group; inside a group the gate that must get the lowest index comes first."""
    shape, limits = (2, 8, 20), ((1000.0, 2000.0), (-3500.0, 3500.0), (-9500.0, 9500.0))
    rng = np.random.default_rng(105)
    zc, yc, xc = roi_rim.voxel_centres(shape, limits)
    nz, ny, nx = shape
    pts, group_of, rank = [], [], []
    groups = []                                    # (kind, voxel, number of tied gates, has_other)
    for v in range(nz * ny * nx):
        iz, rem = divmod(v, ny * nx)
        iy, ix = divmod(rem, nx)
        c = np.array([xc[ix], yc[iy], zc[iz]], dtype=np.float64)
        a, b, d = (int(t) for t in rng.integers(20, 200, 3))
        if v in TIES_FAR_VOXELS:
            side = TIES_FAR_VOXELS[v]
            # lowest index on `side`, highest on the other; TIES_FAR_FILLERS farther members with indices and y in between
            offs = [(0, 300 * side, 0)]
            offs += [(int(rng.integers(-150, 150)), int(rng.integers(-150, 150)), int(rng.integers(400, 450)))
                     for _ in range(TIES_FAR_FILLERS)]
            offs += [(0, -300 * side, 0)]
            kind, n_tied = "far", 2
        else:
            kind = TIE_KINDS[int(rng.integers(len(TIE_KINDS)))]
            if kind == "dup":
                offs, n_tied = [(a, -b, d), (a, -b, d)], 2
            elif kind == "mirror_y":                # the lower index in the LATER cell row (larger y)
                offs, n_tied = [(a, b, d), (a, -b, d)], 2
            elif kind == "mirror_x":
                offs, n_tied = [(a, b, -d), (-a, b, -d)], 2
            elif kind == "three":
                offs, n_tied = [(a, b, d), (-b, d, a), (d, -a, -b)], 3
            elif kind == "centre":                  # a gate exactly on the voxel centre and a runner-up
                offs, n_tied = [(0, 0, 0), (a, 0, 0)], 1
            else:                                   # two gates exactly on the voxel centre
                offs, n_tied = [(0, 0, 0), (0, 0, 0)], 2
        for r, o in enumerate(offs):
            pts.append(c + np.array(o, dtype=np.float64)); group_of.append(len(groups)); rank.append(r)
        groups.append((kind, v, n_tied, len(offs)))
    pts = np.array(pts)
    group_of, rank = np.array(group_of), np.array(rank)
    n = len(pts)
    # scatter the gates over the index range, then hand every group's indices out in rank order
    where = rng.permutation(n)
    index = np.empty(n, dtype=np.int64)
    for g in range(len(groups)):
        sel = np.nonzero(group_of == g)[0]
        index[sel[np.argsort(rank[sel])]] = np.sort(where[sel])
    order = np.argsort(index)
    gx, gy, gz = (pts[order, k].astype(np.float32) for k in range(3))
    assert np.array_equal(gx.astype(np.float64), pts[order, 0])          # integer coordinates: exact in float32
    ties = []
    for g, (kind, v, n_tied, n_offs) in enumerate(groups):
        sel = np.nonzero(group_of == g)[0]
        by_rank = index[sel[np.argsort(rank[sel])]]
        if kind == "far":
            ties.append(Tie(kind, v, (int(by_rank[0]), int(by_rank[-1]))))
        elif kind == "centre":
            ties.append(Tie(kind, v, (int(by_rank[0]),), other=int(by_rank[1])))
        else:
            ties.append(Tie(kind, v, tuple(int(i) for i in by_rank[:n_tied])))
    tied_lo = np.zeros(n, dtype=bool); tied_hi = np.zeros(n, dtype=bool); two_lo = np.zeros(n, dtype=bool)
    for t in ties:
        tied_lo[t.tied[0]] = True
        tied_hi[t.tied[-1]] = len(t.tied) > 1
        two_lo[list(t.tied[:2])] = len(t.tied) > 2
    bg = np.random.default_rng([105, 4]).random(n) < 0.3
    # field 0: every group's lowest tied index excluded; field 2: its highest; field 4: the two lowest of a three-way tie
    # and 30 % of the gates that are not tied; fields 1 and 3: nothing (Scene.mask)
    special = {0: tied_lo, 2: tied_hi, 4: two_lo | (bg & ~tied_lo & ~tied_hi)}
    return Scene("ties", gx, gy, gz, shape, limits, min_radius=600.0, beam_factor=0.0, seed=105, ties=ties,
                 special_masks=special)


# ---- rim ------------------------------------------------------------------------------------------------------------------
RIM = dict(shape=(3, 9, 37), limits=((500.0, 5500.0), (-10e3, 10e3), (-45e3, 45e3)), min_radius=1000.0, beam_factor=0.0)


def _rim() -> Scene:
    """tests/test_gpu_roi_rim.py's 'minr' geometry (r = 1000 m exactly, integer voxel centres 2.5 km apart: a planted gate
    belongs to its own voxel only) with roi_rim's shells on every voxel and the vertical gates on the radar's axis."""
    g = RIM
    cloud = roi_rim.rim_cloud(g["shape"], g["limits"], g["min_radius"], g["beam_factor"], seed=1)
    nz, ny, nx = g["shape"]
    vert = [iz * ny * nx + 4 * nx + 18 for iz in range(nz)]                # x = y = 0
    vc = roi_rim.vertical_cloud(g["shape"], g["limits"], g["min_radius"], g["beam_factor"], vert)
    assert cloud.misses == 0 and np.all(vc.gx == 0) and np.all(vc.gy == 0)
    gx, gy, gz = (np.concatenate([getattr(cloud, k), getattr(vc, k)]) for k in ("gx", "gy", "gz"))
    order = np.random.default_rng(106).permutation(gx.size)
    return Scene("rim", gx[order], gy[order], gz[order], g["shape"], g["limits"], g["min_radius"], g["beam_factor"], seed=106,
                 rim_voxel=np.concatenate([cloud.voxel, vc.voxel])[order])


_BUILDERS = dict(polar_const=_polar_const, polar_beam=_polar_beam, ragged_a=_ragged_a, ragged_b=_ragged_b, ties=_ties,
                 rim=_rim)


@functools.lru_cache(maxsize=None)
def scene(name: str) -> Scene:
    return _BUILDERS[name]()


def rim_labels(s: Scene) -> np.ndarray:
    """The case label of every gate of the rim scene against the voxel it was planted for, recomputed from scratch."""
    cloud = roi_rim.RimCloud(s.gx, s.gy, s.gz, s.rim_voxel, np.full(s.n_gates, "", dtype="<U1"))
    return roi_rim.relabel(cloud, s.shape, s.limits, s.min_radius, s.beam_factor)


def summary(s: Scene) -> dict:
    """Reference-side numbers of a scene (field 1: nothing excluded), as profiles/closest_bounds.json records them."""
    ch = s.choice()
    i32, i64 = ch["idx32"][1], ch["idx64"][1]
    filled = i32 >= 0
    pos = filled & (ch["d2_min64"][1] > 0)
    worst = float((ch["d2_win64"][1][pos] / ch["d2_min64"][1][pos] - 1.0).max(initial=0.0))
    return dict(voxels=int(i32.size), filled_share=float(filled.mean()), float32_ties=int((ch["n_tied"][1] > 1).sum()),
                idx32_ne_idx64=int((i32 != i64).sum()), worst_d2_ratio_minus_1=worst,
                bound_minus_1=float(oracle.CLOSEST_D2_BOUND - 1.0), max_members=int(ch["n_members"].max()))
