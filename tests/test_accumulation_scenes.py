"""The accumulation scenes (tests/accumulation_scenes.py) through the NumPy restatement (tests/accumulation_oracle.py), on the
CPU: that the scenes reach every branch of the contract, so that no GPU test built on them is vacuous, and that the
definition itself behaves as rainfall should."""
import numpy as np
import pytest

import accumulation_oracle as ao
import accumulation_scenes as sc
import motion_oracle as mo


def test_the_scenes_cover_what_the_issue_lists():
    scenes = [sc.scene(n) for n in sc.SCENES]
    shapes = {s.prev.shape[-2:] for s in scenes}
    assert {(1, 1), (3, 5), (37, 53)} <= shapes
    th, tw = sc.TILE
    assert any(h > th and w > tw and h % th and w % tw and h <= 70 and w <= 200 for h, w in shapes)
    assert any(w % 4 and w % 64 for _, w in shapes) and any(h * w < 64 for h, w in shapes)
    assert {s.n_steps for s in scenes} >= {1, 3, 7, 64} and {s.substeps for s in scenes} >= {1, 3}
    assert {s.method for s in scenes} == {"nearest", "bilinear"} and {s.prev.shape[0] for s in scenes} >= {1, 3, 6}
    for n_steps in (7, 64):                               # min_steps: 1, about half, all
        assert {s.min_steps for s in scenes if s.n_steps == n_steps} & {1, n_steps // 2, (n_steps + 1) // 2}
    assert any(s.min_steps == 1 < s.n_steps for s in scenes) and any(s.min_steps == s.n_steps > 1 for s in scenes)
    assert any(1 < s.min_steps < s.n_steps for s in scenes)
    kinds = {"one" if s.lattice.ny * s.lattice.nx == 1 else "dense" if (s.lattice.ny, s.lattice.nx) == s.prev.shape[-2:]
             else "block" for s in scenes}
    assert kinds == {"one", "dense", "block"}
    assert any(not s.motion.any() for s in scenes)                                            # zero
    assert any(s.motion.any() and (s.motion == np.round(s.motion)).all() and s.motion.size == 2 for s in scenes)   # uniform integer
    assert any((s.motion != np.round(s.motion)).any() and np.abs(s.motion).max() <= 6.0 for s in scenes)           # fractional
    assert any(np.isnan(s.prev).any() and np.isposinf(s.prev).any() for s in scenes)
    for s in scenes:
        assert np.isfinite(s.motion).all() and not np.isneginf(s.prev).any() and not np.isneginf(s.next).any()
        assert not s.prev.flags.writeable and not s.motion.flags.writeable


def test_the_outside_scenes_leave_the_plane_on_every_side():
    for name in ("outside_bilinear", "outside_nearest"):
        s = sc.scene(name)
        h, w = s.prev.shape[-2:]
        # the later plane is sampled beyond every side; in one substep so is the earlier one, beyond the opposite side
        for lead in (0.5 / s.n_steps - 1.0,) + ((1.0 - 0.5 / s.n_steps,) if s.substeps == 1 else ()):
            fy, fx = mo.source_position((h, w), s.motion, s.lattice, lead, s.substeps)
            assert (fy < -1.0).any() and (fy > h).any() and (fx < -1.0).any() and (fx > w).any(), (name, lead)


def test_every_branch_and_every_kind_of_count_is_reached():
    taken = np.zeros(4, dtype=np.int64)
    zero = between = full = False
    for name in sc.SCENES:
        s, want = sc.scene(name), sc.expected(name)
        taken += (want.both, want.only_prev, want.only_next, want.neither)
        assert want.both + want.only_prev + want.only_next + want.neither == s.prev.size * s.n_steps
        zero |= bool((want.steps == 0).any())
        between |= bool(((want.steps > 0) & (want.steps < s.n_steps)).any())
        full |= bool((want.steps == s.n_steps).any())
        assert np.array_equal(sc.is_fill(want.out, s.fill), want.steps < s.min_steps), name
        # a NaN that is not the fill would carry a payload no two machines agree on: there is none
        assert not (np.isnan(want.out) & ~sc.is_fill(want.out, s.fill)).any(), name
        if s.holes:
            share = sc.is_fill(want.out, s.fill).mean()
            assert 0.0 < share < 0.5, (name, share)
    assert (taken > 0).all(), taken
    assert zero and between and full
    for name in sc.COMPOSED:
        want = sc.expected(name)
        assert min(want.both, want.only_prev, want.only_next, want.neither) > 0, name


def test_a_moving_pixel_leaves_a_swath_and_keeps_its_total():
    prev, nxt, motion, lat = sc.moving_pixel()
    still, still_lat = sc.one_node((0.0, 0.0))
    none = ao.accumulate(prev, nxt, still, still_lat, sc.MOVING_HOURS, 8, 1, "nearest").out[0]
    assert sorted(zip(*np.nonzero(none))) == [(2, 5), (2, 13)]                     # without motion: one deposit per scan
    for n_steps, columns in ((8, range(5, 13)), (16, range(5, 14))):
        out = ao.accumulate(prev, nxt, motion, lat, sc.MOVING_HOURS, n_steps, 1, "nearest").out[0]
        assert sorted(zip(*np.nonzero(out))) == [(2, x) for x in columns], n_steps
    out = ao.accumulate(prev, nxt, motion, lat, sc.MOVING_HOURS, 8, 1, "nearest").out[0]
    assert (out[2, 5:13] == out[2, 5]).all() and out[2, 5] == np.float32(sc.MOVING_RATE * sc.MOVING_HOURS / 8.0)
    for n_steps in (1, 4, 8, 16):
        out = ao.accumulate(prev, nxt, motion, lat, sc.MOVING_HOURS, n_steps, 1, "nearest").out[0]
        assert out.astype(np.float64).sum() == sc.MOVING_RATE * sc.MOVING_HOURS, n_steps
        assert none.astype(np.float64).sum() == sc.MOVING_RATE * sc.MOVING_HOURS


def test_zero_motion_is_the_trapezoid_rule():
    s, want = sc.scene("zero_motion"), sc.expected("zero_motion")
    assert (want.steps == s.n_steps).all()
    trapezoid = ao.trapezoid(s.prev, s.next, s.hours)
    np.testing.assert_allclose(want.out.astype(np.float64), trapezoid, rtol=1e-6, atol=0.0)
    for method in ("nearest", "bilinear"):
        for n_steps in (1, 3, 64):
            out = ao.accumulate(s.prev, s.next, s.motion, s.lattice, s.hours, n_steps, 3, method).out
            np.testing.assert_allclose(out.astype(np.float64), trapezoid, rtol=1e-6, atol=0.0)


def test_one_step_without_motion_on_a_steady_plane_is_hours_times_rate():
    s, want = sc.scene("steady"), sc.expected("steady")
    assert s.prev is s.next and s.n_steps == 1 and not s.motion.any()
    assert np.array_equal(want.out, (s.hours * s.prev.astype(np.float64)).astype(np.float32))
    assert (want.steps == 1).all() and want.both == s.prev.size


@pytest.mark.parametrize("name", sc.SCENES)
def test_the_restatement_is_the_composition_of_the_advection_restatement(name):
    """Sample by sample the restatement is ``motion_oracle.advect`` at the leads ``s`` and ``s - 1`` with a NaN fill: the
    first sub-instant of every scene, every plane."""
    s = sc.scene(name)
    lead = 0.5 / s.n_steps
    a = mo.advect(s.prev, s.motion, s.lattice, (lead,), s.substeps, s.method, np.nan)[0]
    b = mo.advect(s.next, s.motion, s.lattice, (lead - 1.0,), s.substeps, s.method, np.nan)[0]
    one = ao.accumulate(s.prev, s.next, s.motion, s.lattice, 1.0, s.n_steps, s.substeps, s.method, 1, np.nan)
    if s.n_steps == 1:
        has_a, has_b = ~np.isnan(a), ~np.isnan(b)
        with np.errstate(invalid="ignore"):
            r = np.where(has_a & has_b, 0.5 * a.astype(np.float64) + 0.5 * b.astype(np.float64),
                         np.where(has_a, a, b).astype(np.float64))
        assert np.array_equal(one.out, r.astype(np.float32), equal_nan=True)
    assert np.array_equal(one.steps == 0, (one.steps == 0) & np.isnan(a) & np.isnan(b))
