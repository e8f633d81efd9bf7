"""Seeded many-radar mosaic scenes for tests/test_mosaic_host.py and tests/test_gpu_mosaic_many.py (a helper module: its
name does not start with ``test_``, so pytest does not collect it).

``scene16`` is a mosaic of RG_MAX_RADARS = 16 radars, the most one CSR-free launch takes, on a grid that is ragged against
the K2 kernel's 16 x 4 voxel patch (25 rows, 37 columns).  Twelve radars are live; four are inert:

  slot 0   far outside the grid (its reach window is empty)
  slot 3   no gates at all
  slot 7   gates in reach whose values are masked in every field (its window is visited, nothing is added)
  slot 11  antenna above ``toa``: every gate is cut

Eight live radars stand in a cluster so that some voxels are reached by eight radars or more; the others sit near and
beyond the grid's faces, one with grid levels below its antenna and one high enough that its gates cross the ``toa`` cut.
Slot 15 is live.  ``scene20`` is ``scene16`` plus four live radars: more than one launch takes, for the geometry route.

The oracle CSR of every radar (``oracle.build_geometry`` on the radar's shifted limits, float64 weights) is built once per
process and cached; the weights of any weighting come from ``Scene.weights_f64`` / ``Scene.weights_f32``."""
import dataclasses
import functools
from typing import List, Tuple

import numpy as np

import radar_processor_amd as rg
from oracle import radar_grid_oracle as oracle
from radar_processor_amd import synthetic

SHAPE = (5, 25, 37)                                  # 25 = 6 * 4 + 1 rows, 37 = 2 * 16 + 5 columns
LIMITS = ((0.0, 10000.0), (-36e3, 36e3), (-54e3, 54e3))       # 2.5 km levels, 3 km columns
TOA = 9000.0                                         # between the two top levels in every radar's frame
MIN_RADIUS = 1500.0                                  # sparse scans: the default 250 m leaves most voxels without pairs
BEAM_FACTOR = 0.01746
FIELDS = ("DBZH", "ZDR", "RHOHV")
INERT = {0: "far", 3: "no_gates", 7: "masked", 11: "above_toa"}


@dataclasses.dataclass(frozen=True)
class RadarSpec:
    seed: int
    max_range_m: float
    origin: Tuple[float, float, float]               # (oz, oy, ox) in the grid frame
    kind: str = "live"                               # or one of INERT's values


@dataclasses.dataclass
class Scene:
    name: str
    specs: List[RadarSpec]
    vols: list                                       # synthetic.SyntheticVolume per radar
    origins: List[Tuple[float, float, float]]
    shape: tuple = SHAPE
    limits: tuple = LIMITS
    toa: float = TOA
    min_radius: float = MIN_RADIUS
    beam_factor: float = BEAM_FACTOR

    @property
    def n_radars(self) -> int:
        return len(self.vols)

    @property
    def kinds(self) -> List[str]:
        return [s.kind for s in self.specs]

    def radars(self, sel=None):
        """``[(gate_x, gate_y, gate_z, origin), ...]`` of the radars ``sel`` (default: all), as the mosaic API takes them."""
        sel = range(self.n_radars) if sel is None else sel
        return [(self.vols[r].gate_x, self.vols[r].gate_y, self.vols[r].gate_z, self.origins[r]) for r in sel]

    def offsets(self, sel=None) -> np.ndarray:
        sel = range(self.n_radars) if sel is None else sel
        return np.concatenate([[0], np.cumsum([len(self.vols[r].gate_x) for r in sel])]).astype(np.int64)

    def window(self, r, beam_factor=None, min_radius=None):
        v = self.vols[r]
        return rg.reach_window(v.gate_x, v.gate_y, v.gate_z, self.shape, self.limits, self.origins[r],
                               self.min_radius if min_radius is None else min_radius,
                               self.beam_factor if beam_factor is None else beam_factor, self.toa)

    def csr(self, r):
        """Radar r's oracle CSR on its shifted limits: (indptr int64, gate_indices int32, float64 weights of barnes2)."""
        return _radar_csr(self.specs[r], self.shape, self.limits, self.toa, self.min_radius, self.beam_factor)

    def weights_f64(self, r, weighting):
        ip, idx, w = self.csr(r)
        if weighting == "barnes2":
            return w
        return _weights(self.specs[r], self.shape, self.limits, self.toa, self.min_radius, self.beam_factor, weighting)

    def weights_f32(self, r, weighting):
        """The reference's float32 weights (compute.py:82-87 rounded once) -- what oracle.build_geometry returns."""
        return self.weights_f64(r, weighting).astype(np.float32)

    def mosaic_csr(self, weighting, sel=None, exact=True):
        """The oracle's mosaic CSR of the radars ``sel`` (concat_rows of their CSRs): float64 weights, or float32 ones."""
        sel = list(range(self.n_radars)) if sel is None else list(sel)
        csrs = [(self.csr(r)[0], self.csr(r)[1], self.weights_f64(r, weighting) if exact else self.weights_f32(r, weighting))
                for r in sel]
        return concat_rows(csrs, self.offsets(sel))

    def reached(self) -> np.ndarray:
        """Per voxel: how many radars have at least one oracle neighbour there."""
        return np.sum([np.diff(self.csr(r)[0]) > 0 for r in range(self.n_radars)], axis=0)


def concat_rows(csrs, offsets):
    """Row v: radar 0's row v, then radar 1's, ... with gate numbers shifted by the radar's offset."""
    counts = [np.diff(np.asarray(ip, dtype=np.int64)) for ip, _, _ in csrs]
    indptr = np.concatenate([[0], np.cumsum(np.sum(counts, axis=0))]).astype(np.int64)
    idx = np.empty(int(indptr[-1]), dtype=np.int32)
    w = np.empty(int(indptr[-1]), dtype=csrs[0][2].dtype)
    base = indptr[:-1].copy()
    for r, (ip, gi, wt) in enumerate(csrs):
        ip = np.asarray(ip, dtype=np.int64)
        rows = np.repeat(np.arange(len(ip) - 1), counts[r])
        dest = base[rows] + (np.arange(len(gi)) - ip[rows])
        idx[dest] = np.asarray(gi, dtype=np.int64) + offsets[r]
        w[dest] = wt
        base += counts[r]
    return indptr, idx, w


# ---- the radars -------------------------------------------------------------------------------------------------------------
def _specs16() -> List[RadarSpec]:
    rng = np.random.default_rng(2024)
    rad = lambda: float(rng.uniform(18e3, 28e3))
    jitter = lambda s: float(rng.uniform(-s, s))
    cluster = [(oz, -5.3e3 + jitter(4e3), 7.1e3 + jitter(9e3))     # eight radars within 10 km of one point,
               for oz in (0.0, 180.0, 420.0, 610.0, 830.0, 990.0, 1240.0, 1400.0)]     # antennas over 0 .. 1.4 km
    rim = [
        (2750.0, 24.1e3 + jitter(1e3), -47.3e3 + jitter(1e3)),    # levels 0 and 1 below its antenna; near x-min / y-max
        (7130.0, -31.7e3 + jitter(1e3), 49.9e3 + jitter(1e3)),   # gates above its toa - oz cut; near x-max / y-min
        (350.0, 44.2e3 + jitter(1e3), 30.3e3 + jitter(1e3)),     # beyond the y-max face
        (-420.0, -3.9e3 + jitter(1e3), -63.4e3 + jitter(1e3)),   # below the grid bottom, beyond the x-min face
    ]
    live = iter([cluster[0], rim[0], cluster[1], cluster[2], rim[1], cluster[3], cluster[4], rim[2], cluster[5],
                 cluster[6], rim[3], cluster[7]])                  # slots 1, 2, 4, 5, 6, 8, 9, 10, 12, 13, 14, 15
    inert = {"far": (100.0, 410e3, -380e3), "no_gates": (0.0, 1.3e3, -2.2e3),
             "masked": (300.0, -8.2e3 + jitter(1e3), -19.7e3 + jitter(1e3)),     # overlapping the cluster
             "above_toa": (TOA + 460.0, 12.7e3, -14.1e3)}
    specs = []
    for slot in range(16):
        kind = INERT.get(slot, "live")
        origin = next(live) if kind == "live" else inert[kind]
        specs.append(RadarSpec(seed=100 + slot, max_range_m=rad(), origin=tuple(float(o) for o in origin), kind=kind))
    return specs


def _specs_extra() -> List[RadarSpec]:
    rng = np.random.default_rng(2025)
    origins = [(1900.0, 31.5e3, 36.8e3), (60.0, -38.9e3, -20.6e3), (5200.0, 2.7e3, 28.4e3), (800.0, -6.1e3, 9.4e3)]
    return [RadarSpec(seed=200 + k, max_range_m=float(rng.uniform(18e3, 28e3)), origin=o) for k, o in enumerate(origins)]


@functools.lru_cache(maxsize=None)
def volume(spec: RadarSpec):
    vol = synthetic.make_volume(n_elev=8, n_az=48, n_gates=32, seed=spec.seed, fields=FIELDS, max_range_m=spec.max_range_m)
    if spec.kind == "no_gates":
        vol = dataclasses.replace(vol, n_az=0, gate_x=vol.gate_x[:0], gate_y=vol.gate_y[:0], gate_z=vol.gate_z[:0],
                                  fields={k: f[:0] for k, f in vol.fields.items()})
    elif spec.kind == "masked":
        vol = dataclasses.replace(vol, fields={k: np.ma.array(np.ma.getdata(f), mask=np.ones(f.shape, dtype=bool))
                                               for k, f in vol.fields.items()})
    return vol


@functools.lru_cache(maxsize=None)
def _radar_csr(spec, shape, limits, toa, min_radius, beam_factor):
    v = volume(spec)
    return oracle.build_geometry(v.gate_x, v.gate_y, v.gate_z, shape, rg.mosaic_limits(limits, spec.origin),
                                 radar_altitude=0.0, min_radius=min_radius, beam_factor=beam_factor, weighting="barnes2",
                                 toa=toa - spec.origin[0], exact_weights=True)


@functools.lru_cache(maxsize=None)
def _weights(spec, shape, limits, toa, min_radius, beam_factor, weighting):
    v = volume(spec)
    ip, idx, _ = _radar_csr(spec, shape, limits, toa, min_radius, beam_factor)
    return oracle.pair_weights_f64(ip, idx, v.gate_x, v.gate_y, v.gate_z, shape, rg.mosaic_limits(limits, spec.origin),
                                   min_radius=min_radius, beam_factor=beam_factor, weighting=weighting)


def _scene(name, specs) -> Scene:
    return Scene(name, specs, [volume(s) for s in specs], [s.origin for s in specs])


@functools.lru_cache(maxsize=None)
def scene16() -> Scene:
    return _scene("scene16", _specs16())


@functools.lru_cache(maxsize=None)
def scene20() -> Scene:
    return _scene("scene20", _specs16() + _specs_extra())


# ---- what the scenes must exercise (asserted by tests/test_mosaic_host.py) -------------------------------------------------
def level_coords_in_radar_frame(scene: Scene, r) -> np.ndarray:
    return oracle.axis_coords_f32(scene.limits[0][0], scene.limits[0][1], scene.shape[0]).astype(np.float64) - scene.origins[r][0]


def check_properties(scene: Scene) -> dict:
    """Assert what the scene is built to exercise; returns the measured quantities (for a report)."""
    nz, ny, nx = scene.shape
    kinds = scene.kinds
    live = [r for r, k in enumerate(kinds) if k == "live"]
    pairs = [int(scene.csr(r)[0][-1]) for r in range(scene.n_radars)]
    windows = [scene.window(r) for r in range(scene.n_radars)]
    reached = scene.reached()
    # the inert radars are what they claim to be
    for r, kind in enumerate(kinds):
        v, w = scene.vols[r], windows[r]
        if kind == "far":
            assert w == (0, 0, 0, 0) and pairs[r] == 0 and len(v.gate_x) > 0
        elif kind == "no_gates":
            assert len(v.gate_x) == 0 and w == (0, 0, 0, 0) and pairs[r] == 0
        elif kind == "above_toa":
            assert scene.origins[r][0] > scene.toa and w == (0, 0, 0, 0) and pairs[r] == 0 and len(v.gate_x) > 0
            assert np.all(v.gate_z > np.float32(scene.toa - scene.origins[r][0]))
        elif kind == "masked":
            assert w != (0, 0, 0, 0) and pairs[r] >= 100
            assert all(np.ma.getmaskarray(f).all() for f in v.fields.values())
    # every live radar contributes; some voxel is reached by at least eight radars
    assert all(pairs[r] >= 100 for r in live), [(r, pairs[r]) for r in live]
    assert int(reached.max()) >= 8, int(reached.max())
    # the windows' left edges fall on many positions of the kernel's 16 x 4 patch, and every grid face is touched
    ix0 = {windows[r][2] % 16 for r in range(scene.n_radars) if windows[r] != (0, 0, 0, 0)}
    iy0 = {windows[r][0] % 4 for r in range(scene.n_radars) if windows[r] != (0, 0, 0, 0)}
    assert len(ix0) >= 8 and iy0 == {0, 1, 2, 3}, (sorted(ix0), sorted(iy0))
    wins = [w for w in windows if w != (0, 0, 0, 0)]
    assert any(w[0] == 0 for w in wins) and any(w[1] == ny for w in wins), wins
    assert any(w[2] == 0 for w in wins) and any(w[3] == nx for w in wins), wins
    assert any(w[1] - w[0] < ny or w[3] - w[2] < nx for w in wins)
    # antennas: one with grid levels below it, one whose toa - oz cut lies strictly between two of its levels with gates
    # on both sides of the cut
    below = [r for r in live
             if np.diff(scene.csr(r)[0]).reshape(scene.shape)[level_coords_in_radar_frame(scene, r) < 0].sum() > 0]
    assert below, "no live radar reaches a grid level below its antenna"
    cut = []
    for r in live:
        zl, c = level_coords_in_radar_frame(scene, r), scene.toa - scene.origins[r][0]
        gz = scene.vols[r].gate_z
        if np.any((zl[:-1] < c) & (zl[1:] > c)) and np.any(gz > np.float32(c)) and np.any(gz <= np.float32(c)) \
                and np.diff(scene.csr(r)[0]).reshape(scene.shape)[-1].sum() > 0:
            cut.append(r)
    assert cut, "no live radar with gates across its toa - oz cut that reaches the top level"
    assert kinds[0] != "live" and kinds[7] != "live" and kinds[15] == "live"
    return dict(pairs=pairs, max_reached=int(reached.max()), ix0_residues=sorted(ix0), below=below, cut=cut)
