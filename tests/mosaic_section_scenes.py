"""The scenes of the mosaic-section tests (tests/test_mosaic_section_host.py, tests/test_gpu_mosaic_section.py) and of the
fixtures tests/golden/g12_mosaic_section_*.npz (a helper module: pytest does not collect it).

``PATH`` is a dog-leg across ``mosaic_scenes.scene16()``: from the rim radar near the x-min / y-max corner through the
cluster of eight radars to the rim radar near the x-max / y-min corner, sampled every 650 m -- 193 points (193 mod 4 = 1:
the section kernel's last block of a level is ragged) times the scene's 5 levels.

The oracle of a mosaic section is ``section_scenes.brute_pairs`` per radar IN THAT RADAR'S FRAME -- the points at
``fl32(f64(xs) - ox)``, ``fl32(f64(ys) - oy)``, the levels of ``mosaic_limits(...)[0]``, ``toa - oz`` -- over ALL points (no
window, no NaN marking: the marking is checked against it), joined with ``mosaic_scenes.concat_rows``.

``scene3`` has three radars whose origins are whole metres on ``mosaic_scenes.LIMITS`` (3 km columns and rows at whole
metres): shared lattice coordinates minus origins are exact in float32, so a section along a lattice row sees every radar's
gates from exactly the coordinates the lattice mosaic's voxels have."""
import functools

import numpy as np

import mosaic_scenes as ms
import radar_processor_amd as rg
import section_scenes as sc
from oracle import radar_grid_oracle as oracle

VERTICES = ((-54e3, 30e3), (7.1e3, -5.3e3), (54e3, -33e3))
SPACING = 650.0
N_POINTS = 193
FILL = -9999.0
QC = ("RHOHV", 0.8)
WEIGHTINGS = ("barnes2", "cressman", "nearest")
FIELDS = ("DBZH", "RHOHV")                         # the fields of the fixtures


@functools.lru_cache(maxsize=None)
def scene3() -> ms.Scene:
    specs = [ms.RadarSpec(seed=301, max_range_m=26e3, origin=(0.0, -4000.0, 5000.0)),
             ms.RadarSpec(seed=302, max_range_m=24e3, origin=(350.0, 9000.0, -21000.0)),
             ms.RadarSpec(seed=303, max_range_m=22e3, origin=(1200.0, -15000.0, 30000.0))]
    return ms._scene("scene3", specs)


def scene(name: str) -> ms.Scene:
    return {"scene16": ms.scene16, "scene20": ms.scene20, "scene3": scene3}[name]()


@functools.lru_cache(maxsize=1)
def path():
    """(xs float32, ys float32, s float64) of PATH"""
    return rg.section_path(VERTICES, SPACING)


def frame(v, o):
    """float32 grid-frame coordinates in the frame of a radar at ``o``: fl32(f64(v) - o)"""
    return (np.asarray(v, dtype=np.float32).astype(np.float64) - float(o)).astype(np.float32)


def levels(s: ms.Scene, r) -> np.ndarray:
    lo, hi = rg.mosaic_limits(s.limits, s.origins[r])[0]
    return oracle.axis_coords_f32(lo, hi, s.shape[0])


def radar_points(s: ms.Scene, r, xs, ys):
    return frame(xs, s.origins[r][2]), frame(ys, s.origins[r][1])


_PAIRS = {}


def radar_pairs(s: ms.Scene, r, xs=None, ys=None, key="path"):
    """brute_pairs of radar r at the points (default: PATH) in its frame: (indptr, gate_indices, d2, r2).  Cached per
    (scene, radar, key): pass a ``key`` of your own with points of your own."""
    k = (s.name, r, key)
    if k not in _PAIRS:
        if xs is None:
            xs, ys, _ = path()
        v = s.vols[r]
        x_r, y_r = radar_points(s, r, xs, ys)
        _PAIRS[k] = sc.brute_pairs(v.gate_x, v.gate_y, v.gate_z, x_r, y_r, levels(s, r), radar_altitude=0.0,
                                   min_radius=s.min_radius, beam_factor=s.beam_factor, toa=s.toa - s.origins[r][0])
    return _PAIRS[k]


def mosaic_csr(s: ms.Scene, weighting, sel=None, exact=True, xs=None, ys=None, key="path"):
    """The oracle's CSR of the section through the radars ``sel`` (default: all): float64 weights, or their float32
    roundings; gate numbers carry the offsets of ``sel``'s own concatenation."""
    sel = list(range(s.n_radars)) if sel is None else list(sel)
    csrs = []
    for r in sel:
        ip, idx, d2, r2 = radar_pairs(s, r, xs, ys, key)
        w = oracle.roi_weight_f64(d2, r2, weighting)
        csrs.append((ip, idx, w if exact else w.astype(np.float32)))
    return ms.concat_rows(csrs, s.offsets(sel))


def concat_field(s: ms.Scene, name, sel=None, qc=False):
    """(values float32, mask bool) of field ``name`` over the concatenated gates of ``sel``; ``qc``: with the QC filter."""
    sel = list(range(s.n_radars)) if sel is None else list(sel)
    values, masks = [], []
    for r in sel:
        data, mask = oracle.merge_masks(s.vols[r].fields[name])
        if qc:
            mask = mask | oracle.gate_mask("below", np.ma.getdata(s.vols[r].fields[QC[0]]).ravel(), QC[1])
        values.append(data)
        masks.append(mask)
    return np.concatenate(values), np.concatenate(masks)


def check_properties() -> dict:
    """Assert what scene16 + PATH are built to exercise; returns the measured quantities."""
    s = ms.scene16()
    xs, ys, _ = path()
    nz, n = s.shape[0], len(xs)
    assert n == N_POINTS and n % 4 == 1
    lengths = [np.diff(radar_pairs(s, r)[0]) for r in range(s.n_radars)]
    pairs = int(sum(int(l.sum()) for l in lengths))
    reached = np.sum([l > 0 for l in lengths], axis=0)
    filled = float((reached > 0).mean())
    longest = int(max(int(l.max(initial=0)) for l in lengths))
    # what mosaic_section_points marks dead on the scene's lattice search, against the oracle's reach
    dead, outside_reached = 0, 0
    kinds_without_points = set()
    for r in range(s.n_radars):
        w = s.window(r)
        reaches = lengths[r].reshape(nz, n).sum(axis=0) > 0
        if w == (0, 0, 0, 0):                           # no search at all: not counted among the dead (point, radar) pairs
            assert not reaches.any() or s.kinds[r] == "live", (r, s.kinds[r])
            outside_reached += int(reaches.sum())
            kinds_without_points.add(s.kinds[r])
            continue
        lim = rg.mosaic_limits(s.limits, s.origins[r])
        yc = np.linspace(lim[1][0], lim[1][1], s.shape[1], dtype="float32")[w[0]:w[1]]
        xc = np.linspace(lim[2][0], lim[2][1], s.shape[2], dtype="float32")[w[2]:w[3]]
        x_r, y_r = radar_points(s, r, xs, ys)
        out = (x_r < xc.min()) | (x_r > xc.max()) | (y_r < yc.min()) | (y_r > yc.max())
        dead += int(out.sum())
        outside_reached += int((out & reaches).sum())
        if s.kinds[r] != "live":
            kinds_without_points.add(s.kinds[r])
    idle_live = [r for r in range(s.n_radars) if s.kinds[r] == "live" and lengths[r].sum() == 0]
    assert filled >= 0.25, filled
    assert int((reached >= 8).sum()) >= 30, int((reached >= 8).sum())
    assert longest > 256, longest                       # one radar's row alone wraps the kernel's ring of 128
    assert dead >= 1000, dead
    assert set(ms.INERT.values()) <= kinds_without_points | {"masked"} and "masked" in s.kinds
    assert outside_reached == 0, outside_reached
    return dict(pairs=pairs, filled=filled, eight=int((reached >= 8).sum()), longest=longest, dead=dead,
                idle_live=idle_live, outside_reached=outside_reached)


def fixture(weighting):
    """(meta, arrays) of g12_mosaic_section_<weighting>; the non-Barnes files take gate_indices from the Barnes one."""
    from conftest import load_golden
    meta, arrays = load_golden(f"g12_mosaic_section_{weighting}")
    if weighting != "barnes2":
        _, sib = load_golden("g12_mosaic_section_barnes2")
        arrays.setdefault("gate_indices", sib["gate_indices"])
    return meta, arrays
