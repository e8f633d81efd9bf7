"""Frozen scenes for the texture and the fuzzy-logic classifier (include/radargrid_hydro.h), shared by the CPU and GPU tests.  Every
array is read-only; a reference is computed once with the vectorised restatement (tests/hydro_oracle.py) and cached.
tests/test_hydro_scenes.py asserts on the CPU, through the oracle alone, that the scenes hold what they are said to hold."""
import functools
import itertools

import numpy as np

import hydro_oracle as ho

TILE = 512                                   # RG_HYDRO_TEXTURE_TILE: the shapes straddle it
TEXTURE_G = (1, 2, 64, 65, 126, 127, 128, 513, TILE - 1, TILE, TILE + 1, TILE + 63, TILE + 64)
TEXTURE_R = (1, 3, 5)
TEXTURE_L = (1, 2, 63)
NAN = np.float32(np.nan)


def _freeze(scene):
    for a in scene.values():
        if isinstance(a, np.ndarray):
            a.setflags(write=False)
        elif isinstance(a, (list, tuple)):
            for b in a:
                if isinstance(b, np.ndarray):
                    b.setflags(write=False)
    return scene


# ---- texture -----------------------------------------------------------------------------------------------------------------
def _field(rng, R, G, sigma=4.0, holes=0.15, masked=0.1):
    x = rng.normal(20.0, sigma, (R, G)).astype(np.float32)
    x[rng.random((R, G)) < holes] = NAN
    mask = (rng.random((R, G)) < masked).astype(np.uint8) * np.uint8(3)
    return x, mask


@functools.lru_cache(maxsize=None)
def texture_scenes():
    """name -> dict(x, mask, half_gates, min_valid, centre_only)."""
    out = {}
    for k, (G, R, L) in enumerate(itertools.product(sorted(set(TEXTURE_G)), TEXTURE_R, TEXTURE_L)):
        rng = np.random.default_rng(1000 + k)
        x, mask = _field(rng, R, G)
        out[f"shape_{R}x{G}_L{L}"] = dict(x=x, mask=mask if k % 3 else None, half_gates=L, min_valid=1 + k % min(2 * L + 1, max(G, 1), 9),
                                          centre_only=k & 1)
    rng = np.random.default_rng(77)
    x, mask = _field(rng, 5, 200, holes=0.3, masked=0.2)
    out["holes_mask"] = dict(x=x, mask=mask, half_gates=4, min_valid=5, centre_only=0)
    x, mask = _field(rng, 4, 150)
    x[1] = NAN                                                          # no valid gate: nothing finite
    mask = mask.copy()
    mask[2] = 1                                                         # no valid gate: all masked
    out["empty_rays"] = dict(x=x, mask=mask, half_gates=3, min_valid=1, centre_only=0)
    big, beyond = np.float32(8192.0), np.nextafter(np.float32(8192.0), np.float32(np.inf))
    x = np.where(np.arange(200) % 2 == 0, big, -big).astype(np.float32)[None, :].repeat(3, axis=0)   # the largest D there is
    x[1, 50:60] = [beyond, -beyond, np.inf, -np.inf, NAN, big, -big, beyond, 1e30, -1e30]
    x[2] = rng.uniform(-8192.0, 8192.0, 200).astype(np.float32)
    out["limits"] = dict(x=x, mask=None, half_gates=63, min_valid=2, centre_only=0)
    x = np.full((2, 90), np.float32(3.7))
    x[1] = np.float32(-8191.9995)
    out["constant"] = dict(x=x, mask=None, half_gates=5, min_valid=1, centre_only=1)
    x = rng.normal(0.0, 30.0, (2, 40)).astype(np.float32)               # every gate valid: N = 7 inside, fewer at the ends
    out["min_valid_at_n"] = dict(x=x, mask=None, half_gates=3, min_valid=7, centre_only=0)
    out["min_valid_above_n"] = dict(x=x.copy(), mask=None, half_gates=3, min_valid=8, centre_only=0)
    x = np.zeros(((1 << 20) + 3, 2), np.float32)                         # more tiles than one launch has workgroups: they stride
    x[:, 1] = (np.arange(x.shape[0]) % 251).astype(np.float32)
    x[5::7, 0] = NAN
    out["many_rays"] = dict(x=x, mask=None, half_gates=1, min_valid=2, centre_only=0)
    return {name: _freeze(s) for name, s in out.items()}


def texture_args(s):
    return s["x"], s["mask"], s["half_gates"], s["min_valid"], s["centre_only"]


@functools.lru_cache(maxsize=None)
def texture_reference(name):
    ref = ho.texture(*texture_args(texture_scenes()[name]))
    for a in ref:
        a.setflags(write=False)
    return ref


# ---- classifier --------------------------------------------------------------------------------------------------------------
def _table(rng, B, C, V, cond_var, tie_bin0=True):
    """Class c has its trapezoids centred at 10 c + (a shift per bin and variable): a gate drawn near the centres of a class is
    that class's.  Some shoulders are open, some flanks are steps; the condition variable, which walks through the bins whatever
    the class, is a member of every class everywhere.  With tie_bin0 the last two classes are THE SAME in bin 0."""
    centre = 10.0 * np.arange(C)[None, :, None] + rng.uniform(-2.0, 2.0, (B, 1, V))
    inner, outer = rng.uniform(1.0, 3.0, (B, C, V)), rng.uniform(0.0, 4.0, (B, C, V))
    outer[rng.random((B, C, V)) < 0.15] = 0.0                            # a step: x1 == x2, r = 0
    vert = np.stack([centre - inner - outer, centre - inner, centre + inner, centre + inner + outer], axis=-1)
    left, right = rng.random((B, C, V)) < 0.1, rng.random((B, C, V)) < 0.1
    vert[left, 0] = vert[left, 1] = -np.inf
    vert[right, 2] = vert[right, 3] = np.inf
    if cond_var >= 0:
        vert[:, :, cond_var] = (-np.inf, -np.inf, np.inf, np.inf)
    if tie_bin0 and C >= 2:
        vert[0, C - 1] = vert[0, C - 2]
    return vert.astype(np.float32).astype(np.float64)


def _weights(rng, C, V, tie=True):
    w = np.round(rng.uniform(0.1, 1.0, (C, V)), 2)
    w[rng.random((C, V)) < 0.1] = 0.0
    w[:, 0] = np.maximum(w[:, 0], 0.25)                                   # variable 0 is additive everywhere: W > 0 where it is present
    if tie and C >= 2:
        w[C - 1] = w[C - 2]
    return w


def _gates(rng, vert, edges, cond_var, kinds, R, G, S, per_sweep_var):
    """Values near the centres of a class chosen per gate, then the planted ones: exactly ON every edge, and exactly ON EVERY finite
    vertex of every cell of every variable but the condition variable -- one gate per (bin, class, variable, vertex), with the
    condition variable of that gate inside the bin where the cell is read.  -> (fields, keep [R][G], keep_sweep [S][G]): the gates,
    and the entries of the per-sweep rows, that holes and the mask must leave alone."""
    B, C, V = vert.shape[:3]
    rps = R // S
    owner = np.repeat(rng.integers(0, C, (S, G)), rps, axis=0)            # the rays of a sweep agree, as its per-sweep row must
    fields = []
    for v in range(V):
        with np.errstate(invalid="ignore"):                               # the last bin: the classes of bin 0 are not all different
            mid = 0.5 * (vert[B - 1, :, v, 1] + vert[B - 1, :, v, 2])
        mid = np.where(np.isfinite(mid), mid, 10.0 * np.arange(C))
        fields.append((mid[owner] + rng.normal(0.0, 1.5, (R, G))).astype(np.float32))
    keep, keep_sweep = np.zeros((R, G), bool), np.zeros((S, G), bool)
    head = 2 * len(edges) + 3                                             # the first gates of ray 0: the edges
    assert head < G
    keep[0, :head] = True
    if cond_var >= 0 and B > 1:                                           # the condition variable walks through every bin
        lo, hi = edges[0] - 3.0, edges[-1] + 3.0
        fields[cond_var] = (lo + (hi - lo) * rng.random((R, G))).astype(np.float32)
        fields[cond_var][0, :len(edges)] = np.asarray(edges, np.float32)  # exactly ON every edge, and one float32 below
        fields[cond_var][0, len(edges):2 * len(edges)] = np.nextafter(np.asarray(edges, np.float32), np.float32(-np.inf))
    centres = [edges[0] - 1.0] + [0.5 * (a + b) for a, b in zip(edges, edges[1:])] + [edges[-1] + 1.0] if len(edges) else [0.0]
    # a vertex of the per-sweep variable goes to the FIRST ray of a sweep (the row that is kept), one (sweep, gate) each; every
    # other vertex to a gate of its own among the other rays
    first_of_sweep = np.arange(R) % rps == 0 if per_sweep_var is not None else np.zeros(R, bool)
    free = iter(np.flatnonzero(np.repeat(~first_of_sweep, G) & (np.arange(R * G) >= head)).tolist())
    n_sweep_slots = 0
    for b, c, v, k in itertools.product(range(B), range(C), range(V), range(4)):
        x = vert[b, c, v, k]
        if not np.isfinite(x) or v == cond_var:
            continue
        if v == per_sweep_var:
            ray, g = (n_sweep_slots % S) * rps, head + n_sweep_slots // S
            n_sweep_slots += 1
            assert g < G, "the scene has too few gates for the vertices of its per-sweep variable"
            keep_sweep[ray // rps, g] = True
        else:
            ray, g = divmod(next(free), G)                                # StopIteration: too few gates for the vertices
        fields[v][ray, g] = np.float32(x)
        if cond_var >= 0 and B > 1:
            fields[cond_var][ray, g] = np.float32(centres[b])
        keep[ray, g] = True
    if per_sweep_var is not None:                                         # one row per sweep
        fields[per_sweep_var] = np.ascontiguousarray(fields[per_sweep_var][::rps][:S])
    return fields, keep, keep_sweep


def _classifier_scene(seed, B, C, V, R, G, S, *, zero_weight_class=None, min_score=0.0):
    rng = np.random.default_rng(seed)
    cond_var = 1 % V if B > 1 else -1
    kinds = tuple(1 if (v % 3 == 2) else 0 for v in range(V))             # variables 2, 5 are multiplicative; 0 never is
    edges = tuple(np.round(np.cumsum(rng.uniform(0.5, 2.0, B - 1)), 1).tolist())        # strictly ascending: no bin is empty
    vert = _table(rng, B, C, V, cond_var)
    weights = _weights(rng, C, V)
    if zero_weight_class is not None:
        weights[zero_weight_class] = 0.0
    per_sweep_var = V - 1 if V >= 3 else None
    fields, keep, keep_sweep = _gates(rng, vert, edges, cond_var, kinds, R, G, S, per_sweep_var)
    required = [0] + ([3] if V > 3 else [])
    optional = [v for v in range(V) if v not in required and v != cond_var and v != per_sweep_var]
    for v, share in [(v, 0.04) for v in required] + [(v, 0.1) for v in optional] + ([(cond_var, 0.04)] if cond_var >= 0 else []):
        holes = (rng.random((R, G)) < share) & ~keep                      # a planted gate keeps every variable it has
        fields[v][holes] = [NAN, np.float32(np.inf), np.float32(-np.inf)][v % 3]
    if per_sweep_var is not None:
        fields[per_sweep_var][(np.arange(G) % 11 == 0)[None, :] & ~keep_sweep] = NAN
    mask = ((rng.random((R, G)) < 0.05) & ~keep).astype(np.uint8) * np.uint8(255)
    spec = ho.Spec(kinds, sum(1 << v for v in required), cond_var, edges, ho.compile_cells(vert), weights)
    return _freeze(dict(fields=fields, per_sweep_bits=0 if per_sweep_var is None else 1 << per_sweep_var, rays_per_sweep=R // S,
                        mask=mask, spec=spec, min_score=min_score, vertices=vert, B=B, C=C, V=V, R=R, G=G, S=S))


def vertices_met(s, ref):
    """-> (met, there): of the ``there`` finite vertices of the cells of every variable but the condition variable, ``met`` are
    the value of that variable at a SCORED gate (not masked, nothing required missing, a score computed) of the cell's own bin."""
    full = ho.expand(s["fields"], s["per_sweep_bits"], s["rays_per_sweep"])
    spec = s["spec"]
    scored = ref.best >= 0.0
    bins = np.zeros(scored.shape, np.int64)
    if spec.cond_var >= 0:
        with np.errstate(invalid="ignore"):
            for e in spec.edges:
                bins += full[spec.cond_var] >= np.float32(e)
    met = there = 0
    for b in range(s["B"]):
        here = scored & (bins == b)
        for v in range(s["V"]):
            if v == spec.cond_var:
                continue
            x = s["vertices"][b, :, v, :]
            x = x[np.isfinite(x)]
            there += x.size
            met += int(np.isin(x, full[v][here].astype(np.float64)).sum())
    return met, there


CLASSIFIER_SHAPES = {                        # name -> (seed, B, C, V, R, G, S)
    "one_cell": (1, 1, 1, 1, 3, 70, 1),
    "small": (2, 2, 2, 3, 6, 131, 3),
    "bins32": (3, 32, 4, 8, 6, 700, 1),          # about 3200 finite vertices: a gate for each
    "bins32_sweeps": (4, 32, 4, 8, 9, 700, 3),
    "cap1024": (5, 8, 16, 8, 9, 700, 3),
    "cap1024_one_sweep": (6, 8, 16, 8, 6, 701, 1),
}


@functools.lru_cache(maxsize=None)
def classifier_scenes():
    out = {name: _classifier_scene(*shape) for name, shape in CLASSIFIER_SHAPES.items()}
    out["zero_weights"] = _classifier_scene(7, 2, 3, 3, 6, 131, 3, zero_weight_class=1)
    out["strides"] = _classifier_scene(8, 32, 4, 8, 9, 23000, 3)         # more gates than one launch has lanes: they stride
    # min_score above, at and below the best score of one gate of "small"
    base = out["small"]
    ref = ho.classify(*classifier_args(base))
    at = int(np.flatnonzero((ref.cls.reshape(-1) != 0) & (ref.best.reshape(-1) < 0.9))[0])
    pivot = float(ref.best.reshape(-1)[at])
    for name, value in (("min_score_above", np.nextafter(pivot, np.inf)), ("min_score_at", pivot),
                        ("min_score_below", np.nextafter(pivot, 0.0))):
        out[name] = _freeze(dict(base, min_score=float(value), pivot_gate=at, pivot=pivot))
    return out


def classifier_args(s):
    return s["fields"], s["per_sweep_bits"], s["rays_per_sweep"], s["mask"], s["spec"], s["min_score"]


@functools.lru_cache(maxsize=None)
def classifier_reference(name):
    ref = ho.classify(*classifier_args(classifier_scenes()[name]))
    for a in ref:
        a.setflags(write=False)
    return ref


def tiny(s, rays, gates):
    """The first ``gates`` gates of the first ``rays`` sweeps' first ray each: small enough for the naive restatement."""
    rps = s["rays_per_sweep"]
    rows = [k * rps for k in range(rays) if k * rps < s["R"]]
    fields = [np.ascontiguousarray(a[:len(rows), :gates] if (s["per_sweep_bits"] >> v) & 1 else a[rows][:, :gates])
              for v, a in enumerate(s["fields"])]
    return dict(s, fields=fields, mask=np.ascontiguousarray(s["mask"][rows][:, :gates]), rays_per_sweep=1, R=len(rows), G=gates)
