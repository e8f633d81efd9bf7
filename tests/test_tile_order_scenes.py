"""``oracle.csr_apply_tile_order`` -- the NumPy restatement of the tile kernels' order of float32 additions
(``csrc/rg_row_phase.hpp``) -- and the hand-made geometries of ``tile_order_scenes`` it is run on.  CPU only: that the
restatement computes a weighted mean, that its order is the documented one and no other, and that the scenes reach every lane
split and tell one tile from another.  ``test_gpu_tile_order.py`` then holds the kernels to it bit for bit.
"""
import numpy as np
import pytest

import tile_order_scenes as scenes
from oracle import radar_grid_oracle as oracle


@pytest.fixture(scope="module")
def rest():
    return scenes.Restatements()


def _restate(c, nf, tile, fill=np.nan, used=None):
    return oracle.csr_apply_tile_order(c["indptr"], c["gidx"], c["wts"], c["fields"][:nf], c["masks"][:nf], c["shape"],
                                       tile=tile, fill_value=fill, used=used).reshape(nf, -1)


def _mask(c, f):
    return np.zeros(c["n_gates"], dtype=bool) if c["masks"][f] is None else c["masks"][f]


# ---- the scenes hold what their description says --------------------------------------------------------------------------------
def test_scene_inventory(rest):
    assert set(scenes.TILES) == {t for nf in range(1, 9) for t in scenes.tiles_for(nf)}
    for nf in range(1, 9):
        assert oracle.TILE_ORDER_DEFAULT[nf] in scenes.tiles_for(nf)
    assert [scenes.LANES_OF_SPAN[s] for s in scenes.SPANS] == [64, 32, 16, 16, 8, 8, 4, 4, 2, 2, 1, 1]
    line_lengths, seg_rows = set(), set()
    for name in scenes.SCENES:
        c = rest.scene(name)
        segs = scenes.segments(c["shape"])
        line_lengths.add(c["shape"][2])
        seg_rows |= {s[3] for s in segs}
        assert c["indptr"].dtype == np.int64 and len(c["fields"]) == len(c["masks"]) == 8
        assert c["lengths"].size <= 4000 and c["n_pairs"] <= 40000, name
        if name == "empty":
            assert c["n_pairs"] == 0
            continue
        assert int(c["gidx"][-1]) == c["n_gates"] - 1 and int(c["gidx"].max()) == c["n_gates"] - 1
        assert [m is None for m in c["masks"]] == [True, False] * 4
        w = c["wts"]
        assert w.dtype == np.float32 and float(w.min()) >= np.float32(np.exp(-4.0)) and float(w.max()) <= 1.00002
        spans = [int(c["indptr"][r0 + n] - c["indptr"][r0]) for (_, _, r0, n) in segs]
        if name != "line1":
            assert 0 in spans, name                                       # a segment without a pair
            assert any(sp and c["lengths"][r0] == 0 and c["lengths"][r0 + n - 1] == 0 for sp, (_, _, r0, n) in zip(spans, segs))
            assert any(sp % t and nxt for t in scenes.TILES for sp, nxt in zip(spans[:-1], spans[1:]))   # pairs follow a part tile
            assert {"nan", "pinf", "minf", "pminf", "negzero", "denorm", "excl", "masked"} <= set(c["kinds"].values())
        for f in range(8):
            v = c["fields"][f]
            assert np.isnan(v[scenes.G_NAN]) and v[scenes.G_PINF] == np.inf and v[scenes.G_MINF] == -np.inf
            assert v[scenes.G_NEGZERO] == 0 and np.signbit(v[scenes.G_NEGZERO]) and 0 < v[scenes.G_DENORM] < np.finfo(np.float32).tiny
            assert int(v.view(np.uint32)[scenes.G_EXCL]) == scenes.EXCLUDED_BITS
            assert not _mask(c, f)[488:494].any()
            assert _mask(c, f)[scenes.MASKED_GATES].all() == (f in scenes.MASKED_FIELDS)
            ordinary = v[scenes.ORDINARY]
            assert (ordinary > 0).any() and (ordinary < 0).any() and np.abs(ordinary).max() / np.abs(ordinary).min() > 2.0 ** 16
    assert {1, 63, 64, 65, 130} <= line_lengths and {1, 63, 64, 33, 32, 44, 43} <= seg_rows
    c = rest.scene("line130")
    assert c["shape"][0] * c["shape"][1] >= 5 and len(scenes.segments(c["shape"])) % 4 != 0
    for T in scenes.TILES:
        c = rest.scene(f"seams{T}")
        segs = scenes.segments(c["shape"])
        assert c["tile"] == T and len(segs) % 4 != 0
        starts = {}
        for cname, n in zip(scenes.LENGTH_CLASSES, (T - 1, T, T + 1, 2 * T, 2 * T + 1, 3 * T + 5)):
            rows = c["classes"]["len " + cname]
            assert (c["lengths"][rows] == n).all()
            starts[cname] = sorted(int(c["indptr"][r] - c["indptr"][r // 64 * 64]) for r in rows)
            assert starts[cname] == [0, 1, T - 1], (T, cname)
        for r in c["classes"]["ends at a boundary"]:
            assert int(c["indptr"][r + 1] - c["indptr"][r // 64 * 64]) % T == 0 and c["lengths"][r] >= 64
        for r in c["classes"]["starts at a boundary"]:
            off = int(c["indptr"][r] - c["indptr"][r // 64 * 64])
            assert off and off % T == 0 and c["lengths"][r] >= 32
        for r in c["classes"]["long between short"]:
            off0, off1 = (int(c["indptr"][r + k] - c["indptr"][r // 64 * 64]) for k in (0, 1))
            assert (off1 - 1) // T - off0 // T >= 2 and 0 < c["lengths"][r - 1] < 10 and 0 < c["lengths"][r + 1] < 10
        for s in scenes.SPANS:
            rows = c["classes"][f"span {s}"]
            assert rows.size == s and rows[0] % 64 == 0 and (np.diff(rows) == 1).all() and c["lengths"][rows].sum() <= T
            assert c["lengths"][rows[-1] + 1:rows[0] + 64].sum() == 0
        a, b = c["classes"]["gap apart"], c["classes"]["gap adjacent"]
        assert b[1] - b[0] == 1 and a[1] - a[0] == 41 and c["lengths"][a[0] + 1:a[1]].sum() == 0
        for ra, rb in zip(a, b):
            pa, pb = (slice(int(c["indptr"][r]), int(c["indptr"][r + 1])) for r in (ra, rb))
            assert np.array_equal(c["gidx"][pa], c["gidx"][pb]) and np.array_equal(c["wts"][pa], c["wts"][pb])
        last = int(c["classes"]["last row"][0])
        assert c["indptr"][last + 1] == c["n_pairs"] and (c["n_pairs"] - 1 - int(c["indptr"][last])) % T == 0


# ---- 1. it is a mean -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", scenes.DATA_SCENES)
def test_restatement_is_a_weighted_mean(rest, name):
    """Every finite voxel within the float64 mean bound (``oracle.mean_error_bound``, which holds for any order of the adds),
    NaN and fill patterns those of ``oracle.csr_apply_f64``: 1, 3 and 8 fields, every tile their table accepts.  The wide
    runs the GPU test reuses for narrower field counts hold the same bits."""
    c = rest.scene(name)
    stats = [oracle.voxel_stats(c["indptr"], c["gidx"], c["wts"], c["fields"][f], _mask(c, f)) for f in range(8)]
    f64 = [oracle.csr_apply_f64(c["indptr"], c["gidx"], c["wts"], c["fields"][f], _mask(c, f), c["shape"],
                                fill_value=-9999.0).ravel() for f in range(8)]
    worst = 0.0
    for nf in (1, 3, 8):
        for tile in scenes.tiles_for(nf):
            got = _restate(c, nf, tile, fill=-9999.0)
            assert np.array_equal(scenes.same_bits(got, rest.get(name, nf, tile, fill=-9999.0)), np.ones(got.shape, dtype=bool))
            for f in range(nf):
                assert np.array_equal(np.isnan(got[f]), np.isnan(f64[f])), (name, nf, tile, f)
                assert np.array_equal(got[f] == -9999.0, f64[f] == -9999.0), (name, nf, tile, f)
                assert np.array_equal(np.isinf(got[f]), np.isinf(f64[f])), (name, nf, tile, f)
                fin = np.isfinite(got[f]) & (got[f] != -9999.0)
                assert fin.sum() > 0
                # the bound's error model has no underflow: a product in the denormal range is rounded to a multiple of
                # 2^-149 (error <= 2^-150, at most e^4 times that after the division by a weight >= e^-4) and so is the mean
                tiny = fin & (np.abs(stats[f]["m"]) < np.finfo(np.float32).tiny) & (stats[f]["m"] != 0)
                assert (np.abs(got[f][tiny].astype(np.float64) - stats[f]["m"][tiny]) <= 2.0 ** -150 * (np.exp(4.0) + 1)).all()
                assert tiny.sum() == sum(k == "denorm" for k in c["kinds"].values())
                fin &= ~tiny
                ratio = oracle.bound_ratio(got[f][fin], {k: v[fin] for k, v in stats[f].items()}, oracle.DELTA_CSR["barnes2"])
                worst = max(worst, float(ratio.max()))
                assert (ratio <= 1).all(), (name, nf, tile, f, float(ratio.max()))
    print(f"{name}: worst |restatement - m| / bound = {worst:.3f}")
    if name != "line1":
        k = scenes.MASKED_FIELDS[0]                        # all gates masked in field k, none in field k + 1
        got = _restate(c, 8, 128)
        rows = [r for r, kind in c["kinds"].items() if kind == "masked"]
        assert rows and np.isnan(got[k][rows]).all() and np.isfinite(got[k + 1][rows]).all()
        excl = [r for r, kind in c["kinds"].items() if kind in ("excl", "nan")]
        assert np.isnan(got[:, excl]).all()                # an unmasked value with the sentinel's bits is a data NaN
        zero = [r for r, kind in c["kinds"].items() if kind == "negzero"]
        assert (got[:, zero] == 0).all() and not np.signbit(got[:, zero]).any()
        den = [r for r, kind in c["kinds"].items() if kind == "denorm"]
        assert (got[:, den] > 0).all() and (got[:, den] < np.finfo(np.float32).tiny).all()      # (w * d) / w: still a denormal


def test_tile_argument():
    c = scenes.line_scene(1)
    for nf, bad in ((1, 192), (1, 320), (2, 192), (3, 512), (4, 192), (4, 512), (5, 256), (8, 384), (1, 64), (3, 100)):
        with pytest.raises(ValueError):
            _restate(c, nf, bad)
    for nf in range(1, 9):
        default = _restate(c, nf, 0)
        assert scenes.same_bits(default, _restate(c, nf, 384 if nf <= 4 else 128)).all()


def test_geometry_without_a_pair():
    c = scenes.empty_scene()
    for nf in (1, 3, 8):
        for fill in (np.nan, -3.0):
            got = _restate(c, nf, 0, fill=fill)
            assert got.shape == (nf, 210) and scenes.same_bits(got, np.full_like(got, fill)).all()


# ---- 2. it is this order and no other --------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", scenes.DATA_SCENES)
def test_rows_of_one_or_two_pairs_equal_the_reference_sum(rest, name):
    """One pair is no sum; two pairs are one addition, commutative, whether they share a tile or not."""
    c = rest.scene(name)
    rows = np.nonzero((c["lengths"] >= 1) & (c["lengths"] <= 2))[0]
    assert rows.size >= 2
    for f in range(8):
        with np.errstate(invalid="ignore"):
            ref = oracle.csr_apply(c["indptr"], c["gidx"], c["wts"], c["fields"][f], _mask(c, f), c["shape"]).ravel()
        for tile in scenes.TILES:
            if f < scenes.WIDEST[tile]:
                want = np.where(rest.filled(name, f + 1)[f], rest.FILL, ref)
                assert scenes.same_bits(rest.wide(name, tile)[f][rows], want[rows]).all(), (name, f, tile)


def _hand_case(lead, tile):
    """One row of five pairs 1e8, 1, -1e8, 1, 1 with unit weights behind a row of ``lead`` pairs of value 0."""
    lengths = np.array([lead, 5] if lead else [5, 0])
    indptr = np.concatenate([[0], np.cumsum(lengths)]).astype(np.int64)
    gidx = np.concatenate([np.full(lead, 5), np.arange(5)]).astype(np.int32)
    values = np.array([1e8, 1.0, -1e8, 1.0, 1.0, 0.0], dtype=np.float32)
    nf = 1 if tile in scenes.tiles_for(1) else 3                  # 192 and 320 pairs are tiles of three fields
    got = oracle.csr_apply_tile_order(indptr, gidx, np.ones(lead + 5, dtype=np.float32), [values] * nf, [None] * nf, (1, 1, 2),
                                      tile=tile)
    assert scenes.same_bits(got[0], got[-1]).all()
    return got[0].ravel()[1 if lead else 0]


def test_hand_worked_sums():
    """float32: 1e8 + 1 = 1e8 and -1e8 + 1 = -1e8 (the spacing at 1e8 is 8).
    Inside one tile, the only active row: L = 64, lanes 0..4 hold one value each.  Fold by 1: lane 0 = 1e8 + 1 = 1e8, lane 2 =
    -1e8 + 1 = -1e8, lane 4 = 1 + 0 = 1.  By 2: lane 0 = 1e8 + -1e8 = 0, lane 4 = 1.  By 4: lane 0 = 0 + 1 = 1.  Mean 1 / 5.
    Straddling a boundary after its second pair, behind a row that fills the first tile: there two rows are active, L = 32,
    the part (1e8, 1) folds to 1e8 + 1 = 1e8; in the next tile the row is alone, L = 64, lanes 0..2 hold -1e8, 1, 1: by 1 lane 0
    = -1e8 + 1 = -1e8, lane 2 = 1; by 2 lane 0 = -1e8 + 1 = -1e8.  Running sum 1e8 + -1e8 = 0.  Mean 0 / 5.
    (The exact mean is 3 / 5, plain left-to-right summation gives 2 / 5.)"""
    for tile in scenes.TILES:
        inside = _hand_case(0, tile)
        assert inside.dtype == np.float32 and inside == np.float32(0.2) and inside == np.float32(np.float64(1.0) / 5.0)
        assert _hand_case(7, tile) == np.float32(0.2)                       # two active rows, L = 32: the same folds
        straddling = _hand_case(tile - 2, tile)
        assert straddling == np.float32(0.0) and not np.signbit(straddling)
        assert _hand_case(2 * tile - 2, tile) == np.float32(0.0)            # the same at the second boundary


# ---- 3. the scenes discriminate --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", scenes.DATA_SCENES)
def test_order_differs_from_left_to_right_summation(rest, name):
    """At least a quarter of the rows with 8 or more pairs hold other bits than plain left-to-right float32 sums give, for every
    tile (a seam scene: above all for the tile it was built for) and for an unmasked and a masked field."""
    c = rest.scene(name)
    rows = np.nonzero(c["lengths"] >= 8)[0]
    assert rows.size >= (2 if name == "line1" else 40)
    for f in (0, 1):
        seq = scenes.sequential_mean(c, f)
        for tile in scenes.TILES:
            if f >= scenes.WIDEST[tile]:
                continue
            got = np.where(rest.filled(name, f + 1)[f], np.float32(np.nan), rest.wide(name, tile)[f])
            differ = ~scenes.same_bits(got[rows], seq[rows])
            print(f"{name} field {f} tile {tile}: {differ.sum()} of {rows.size} rows differ from left-to-right sums")
            assert differ.sum() * 4 >= rows.size, (name, f, tile)


@pytest.mark.parametrize("T", scenes.TILES)
def test_seam_classes_tell_the_tiles_apart(rest, T):
    """For every field count and every other tile its table accepts next to T: in every seam class at least one row of the
    scene built for T holds other bits at the other tile (some field of the pass differs)."""
    name = f"seams{T}"
    c = rest.scene(name)
    checked = 0
    for nf in range(1, 5):
        if T not in scenes.tiles_for(nf):
            continue
        mine = rest.get(name, nf, T)
        for other in scenes.tiles_for(nf):
            if other == T:
                continue
            theirs = rest.get(name, nf, other)
            for cls in scenes.SEAM_CLASSES:
                rows = c["classes"][cls]
                assert rows.size >= 3
                assert (~scenes.same_bits(mine[:, rows], theirs[:, rows])).any(), (T, nf, other, cls)
                checked += 1
    assert checked >= 9 * 3


@pytest.mark.parametrize("T", scenes.TILES)
def test_gaps_count(rest, T):
    """Two rows 40 empty rows apart share a tile one lane per row (span 42); the same pairs in adjacent rows get 32 lanes each:
    other bits, in the unmasked field 0, at every tile (both segments fit the smallest tile)."""
    name = f"seams{T}"
    c = rest.scene(name)
    for tile in scenes.TILES:
        got = rest.wide(name, tile)[0]
        apart, adjacent = got[c["classes"]["gap apart"]], got[c["classes"]["gap adjacent"]]
        assert np.isfinite(apart).all() and not scenes.same_bits(apart, adjacent).any(), (T, tile)


# ---- 4. coverage -----------------------------------------------------------------------------------------------------------------
def test_every_lane_split_at_every_tile(rest):
    """Over all scenes the restatement meets every L in 1 .. 64 at every tile; the span segments meet the L their span
    dictates; and the kernel's loop over groups of 64 / L rows makes one trip, always (64 / L >= nact by the choice of L), with
    groups that are full (1, 2, 4 ... rows) and groups whose last lanes have no row (3, 5, 9, 17, 33 rows)."""
    used = set()
    for name in scenes.DATA_SCENES:
        c = rest.scene(name)
        for nf, tile in ((8, 128), (3, 192), (4, 256), (4, 320), (4, 384), (2, 512)):
            _restate(c, nf, tile, used=used)
    assert {(t, lanes) for (t, lanes, _) in used} == {(t, 1 << k) for t in scenes.TILES for k in range(7)}
    assert {rounds for (_, _, rounds) in used} == {1}
    for T in scenes.TILES:
        c = rest.scene(f"seams{T}")
        for s in scenes.SPANS:
            rows = c["classes"][f"span {s}"]
            seg = slice(int(rows[0]), int(rows[0]) + 64)
            lengths = c["lengths"][seg]
            indptr = np.concatenate([[0], np.cumsum(lengths)])
            n = int(indptr[-1])
            only = set()
            nf = 1 if T in scenes.tiles_for(1) else 3
            oracle.csr_apply_tile_order(indptr, np.zeros(n, dtype=np.int32), np.ones(n, dtype=np.float32),
                                        [np.ones(1, dtype=np.float32)] * nf, [None] * nf, (1, 1, 64), tile=T, used=only)
            assert {lanes for (_, lanes, _) in only} == {scenes.LANES_OF_SPAN[s]}, (T, s, only)
