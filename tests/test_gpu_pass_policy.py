"""The kernel, window and pass size ``pass_policy`` chooses on real geometries (the decisions themselves are held against a
frozen restatement on the CPU, test_pass_policy_host.py; here: that ``CsrGridder`` and ``fields_per_pass`` gather the right
facts from a device geometry and that ``apply()`` reaches the entry point the choice names).

The two scenes of slab_scenes.py: on the wide scene (6 x 10 x 150) 68 % of the pairs sit in two over-wide chunks (4224 and
7023 distinct gates, in the first and the second line group of the lowest level), so a ``layout="csr"`` geometry turns its
compact copy down.  Its first eight lines (``WIDE_WINDOW``, 6 x 8 x 150) hold both of those chunks, so the copy is turned
down there as well, for every field count; the two scenes differ in nothing the policy looks at.  The scene's last two
lines (``TAIL_WINDOW``, 6 x 2 x 150: its third line group, at most 1663 gates per chunk) are therefore taken as a third
scene, on which a ``layout="csr"`` geometry keeps its copy -- up to the field count at which the tile kernel's window
passes 24 KiB, where the weights are not codable.  Barnes weights are codable in the packed records, Cressman weights are
not.
"""
import numpy as np
import pytest

import slab_scenes as scenes

pytestmark = pytest.mark.gpu

TAIL_WINDOW = (8, 10, 0, 150)
SCENES = {"wide": (None, scenes.WIDE_SHAPE), "window": (scenes.WIDE_WINDOW, scenes.WINDOW_SHAPE),
          "tail": (TAIL_WINDOW, (6, 2, 150))}                                  # RoiSearch(window=), its grid shape
WEIGHTINGS = ("barnes2", "cressman")
LAYOUTS = ("csr", "compact", "packed")
FIELD_COUNTS = (1, 3, 4, 5, 8)
FLAGS = ((False, False), (False, True), (True, False), (True, True))          # CsrGridder(compact=, packed=)

# (scene, weighting, layout) -> (fields_per_pass, {n_fields: one (compact is None, packed_stream, window) per pair of FLAGS}).
# Recorded, not derived (see test_gridder_choices_on_the_slab_scenes); the window scene gave the wide scene's rows.
_DOWN = [(True, False, 0), (True, False, 0), (True, False, 0), (True, False, 0)]
_WIDE = {
    ('barnes2', 'csr'): (4, {1: _DOWN, 3: _DOWN, 4: _DOWN, 5: _DOWN, 8: _DOWN}),
    ('barnes2', 'compact'): (4, {
        1: [(False, False, 4096), (False, True, 4096), (False, False, 4096), (False, True, 4096)],
        3: [(False, False, 2688), (False, True, 3072), (False, False, 2688), (False, True, 3072)],
        4: [(False, False, 2048), (False, True, 2432), (False, False, 2048), (False, True, 2432)],
        5: [(False, False, 1024), (False, True, 1216), (False, False, 1024), (False, True, 1216)],
        8: [(False, False, 1024), (False, True, 1216), (False, False, 1024), (False, True, 1216)],
    }),
    ('barnes2', 'packed'): (4, {
        1: [(False, True, 4096), (False, True, 4096), (False, True, 4096), (False, True, 4096)],
        3: [(False, True, 3072), (False, True, 3072), (False, True, 3072), (False, True, 3072)],
        4: [(False, True, 2432), (False, True, 2432), (False, True, 2432), (False, True, 2432)],
        5: [(False, True, 1216), (False, True, 1216), (False, True, 1216), (False, True, 1216)],
        8: [(False, True, 1216), (False, True, 1216), (False, True, 1216), (False, True, 1216)],
    }),
    ('cressman', 'csr'): (8, {1: _DOWN, 3: _DOWN, 4: _DOWN, 5: _DOWN, 8: _DOWN}),
    ('cressman', 'compact'): (8, {
        1: [(False, False, 4096), (False, False, 4096), (False, False, 4096), (False, False, 4096)],
        3: [(False, False, 2688), (False, False, 2688), (False, False, 2688), (False, False, 2688)],
        4: [(False, False, 2048), (False, False, 2048), (False, False, 2048), (False, False, 2048)],
        5: [(False, False, 1024), (False, False, 1024), (False, False, 1024), (False, False, 1024)],
        8: [(False, False, 1024), (False, False, 1024), (False, False, 1024), (False, False, 1024)],
    }),
}
TABLE = {(scene,) + key: rows for scene in ("wide", "window") for key, rows in _WIDE.items()}
TABLE.update({
    ('tail', 'barnes2', 'csr'): (4, {
        1: [(True, False, 0), (True, False, 0), (False, False, 1792), (False, True, 1792)],
        3: [(True, False, 0), (True, False, 0), (False, False, 1792), (False, True, 1792)],
        4: [(True, False, 0), (True, False, 0), (True, False, 0), (False, True, 1792)],     # tile window 28 KiB; records: kept
        5: _DOWN,                                                                           # 1024 entries: > 2 % fall back
        8: _DOWN,
    }),
    ('tail', 'barnes2', 'compact'): (4, {
        1: [(False, False, 1792), (False, True, 1792), (False, False, 1792), (False, True, 1792)],
        3: [(False, False, 1792), (False, True, 1792), (False, False, 1792), (False, True, 1792)],
        4: [(False, False, 1792), (False, True, 1792), (False, False, 1792), (False, True, 1792)],
        5: [(False, False, 1024), (False, True, 1216), (False, False, 1024), (False, True, 1216)],
        8: [(False, False, 1024), (False, True, 1216), (False, False, 1024), (False, True, 1216)],
    }),
    ('tail', 'barnes2', 'packed'): (4, {
        1: [(False, True, 1792), (False, True, 1792), (False, True, 1792), (False, True, 1792)],
        3: [(False, True, 1792), (False, True, 1792), (False, True, 1792), (False, True, 1792)],
        4: [(False, True, 1792), (False, True, 1792), (False, True, 1792), (False, True, 1792)],
        5: [(False, True, 1216), (False, True, 1216), (False, True, 1216), (False, True, 1216)],
        8: [(False, True, 1216), (False, True, 1216), (False, True, 1216), (False, True, 1216)],
    }),
    ('tail', 'cressman', 'csr'): (8, {
        1: [(True, False, 0), (True, False, 0), (False, False, 1792), (False, False, 1792)],
        3: [(True, False, 0), (True, False, 0), (False, False, 1792), (False, False, 1792)],
        4: _DOWN,
        5: _DOWN,
        8: _DOWN,
    }),
    ('tail', 'cressman', 'compact'): (8, {
        1: [(False, False, 1792), (False, False, 1792), (False, False, 1792), (False, False, 1792)],
        3: [(False, False, 1792), (False, False, 1792), (False, False, 1792), (False, False, 1792)],
        4: [(False, False, 1792), (False, False, 1792), (False, False, 1792), (False, False, 1792)],
        5: [(False, False, 1024), (False, False, 1024), (False, False, 1024), (False, False, 1024)],
        8: [(False, False, 1024), (False, False, 1024), (False, False, 1024), (False, False, 1024)],
    }),
})


@pytest.fixture(scope="module")
def rg():
    import radar_processor_amd as pkg
    pkg.load_library()
    return pkg


def _geometry(rg, scene, weighting, layout):
    """The scene's geometry in ``layout``, built fresh (the compact copy and the records of a ``"csr"`` geometry are built
    by the gridders that ask for them, in the order of :func:`observe`)."""
    from radar_processor_amd import geometry_builder
    from radar_processor_amd.grid_geometry import GridGeometry
    v = scenes.wide_volume()
    search = rg.RoiSearch(v.gate_x, v.gate_y, v.gate_z, scenes.WIDE_SHAPE, scenes.WIDE_LIMITS, window=SCENES[scene][0],
                          **scenes.WIDE_KW)
    assert search.grid_shape == SCENES[scene][1]
    if layout == "csr":
        csr, compact = search.build_csr(weighting), None
    else:
        csr, compact = geometry_builder._build_compact_only(search, weighting, packed=layout == "packed")
    return GridGeometry.from_device(search.grid_shape, scenes.WIDE_LIMITS, csr, search.toa, compact=compact)


def cases():
    return [(scene, weighting, layout) for scene in SCENES for weighting in WEIGHTINGS for layout in LAYOUTS
            if not (layout == "packed" and weighting == "cressman")]


def observe(rg, case):
    """``(fields_per_pass, {n_fields: [(compact is None, packed_stream, window), ...]}, geometry)`` of one case: a
    ``CsrGridder`` per field count and pair of flags, in this order, then ``fields_per_pass``."""
    from radar_processor_amd.gridding import CsrGridder, fields_per_pass
    geom = _geometry(rg, *case)
    n_gates = scenes.wide_volume().n_total_gates
    rows = {}
    for nf in FIELD_COUNTS:
        rows[nf] = []
        for compact, packed in FLAGS:
            g = CsrGridder(geom, n_gates, nf, compact=compact, packed=packed)
            rows[nf].append((g.compact is None, bool(g.packed_stream), int(g.window)))
    return int(fields_per_pass(geom)), rows, geom


@pytest.mark.parametrize("case", cases(), ids="-".join)
def test_gridder_choices_on_the_slab_scenes(rg, case):
    """``(gridder.compact is None, gridder.packed_stream, gridder.window)`` for 1, 3, 4, 5 and 8 fields and the four
    ``(compact, packed)`` flag pairs, and ``fields_per_pass(geometry)``, equal ``TABLE``.  The table was recorded by running
    this very loop (:func:`observe`) on the commit before ``pass_policy`` existed, where ``CsrGridder.__init__`` and
    ``gridding._fields_per_pass`` spelled the conditions out themselves.  (``fields_per_pass`` is asked after the gridders
    have built the copy, which then decides: 4 for Barnes, whose 8192- and 1792-entry windows do not hold 40-byte entries
    in 32 KiB.)"""
    per_pass, rows, _ = observe(rg, case)
    print(case, per_pass, rows)
    want_per_pass, want_rows = TABLE[case]
    assert per_pass == want_per_pass
    assert rows == want_rows


ENTRY_POINTS = ("rg_csr_apply_f32_ex", "rg_csr_compact_apply_f32", "rg_csr_compact_apply_packed_f32_ex")


@pytest.mark.parametrize("weighting", WEIGHTINGS)
@pytest.mark.parametrize("scene", ["wide", "tail"], ids=["turned_down", "accepted"])
def test_apply_reaches_the_entry_point_the_table_names(rg, scene, weighting, monkeypatch):
    """``CsrGridder(compact=True).apply()`` of three fields on the ``layout="csr"`` geometry calls exactly one of the three
    CSR entry points: the standard kernel's where the table says the copy was turned down (wide scene), the row-wise
    kernel's over the records where it says they are streamed (the scene's tail, Barnes), the tile kernel's otherwise (the
    tail, Cressman)."""
    import torch
    from radar_processor_amd.gridding import CsrGridder
    nf = 3
    no_copy, stream, window = TABLE[scene, weighting, "csr"][1][nf][FLAGS.index((True, True))]
    assert no_copy == (scene == "wide") and stream == (scene == "tail" and weighting == "barnes2")
    want = ENTRY_POINTS[0] if no_copy else ENTRY_POINTS[2] if stream else ENTRY_POINTS[1]
    geom = _geometry(rg, scene, weighting, "csr")
    v = scenes.wide_volume()
    g = CsrGridder(geom, v.n_total_gates, nf, compact=True)
    assert (g.compact is None, bool(g.packed_stream), int(g.window)) == (no_copy, stream, window)
    calls = []
    for name in ENTRY_POINTS:
        def spy(*a, _orig=getattr(g.lib, name), _name=name):
            calls.append(_name)
            return _orig(*a)
        monkeypatch.setattr(g.lib, name, spy)
    rng = np.random.default_rng(5)
    fields = [torch.from_numpy(rng.normal(0.0, 10.0, v.n_total_gates).astype(np.float32)).to(g.dev) for _ in range(nf)]
    g.pack(fields)
    out = torch.empty((nf, g.n_vox), dtype=torch.float32, device=g.dev)
    g.apply(out)
    torch.cuda.synchronize(g.dev)
    assert calls == [want], calls
    assert bool(torch.isfinite(out).any())
