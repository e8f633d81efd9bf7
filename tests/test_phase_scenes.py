"""Every scene of tests/phase_scenes.py reaches what it was built for -- asserted on the CPU, through the oracle alone."""
import numpy as np
import pytest

import phase_oracle as po
import phase_scenes as ps


def test_shapes_and_read_only_arrays():
    assert {G for _, G in ps.SHAPES} == {1, 2, 63, 64, 65, 128, 129, 200} and {R for R, _ in ps.SHAPES} == {1, 5, 9}
    for scenes, prefix in ((ps.unfold_scenes(), "ramp"), (ps.fit_scenes(), "fit"), (ps.attenuation_scenes(), "att")):
        for R, G in ps.SHAPES:
            assert scenes[f"{prefix}_{R}x{G}"][0].shape == (R, G)
        for scene in scenes.values():
            for a in scene:
                if isinstance(a, np.ndarray):
                    assert not a.flags.writeable
                    with pytest.raises(ValueError):
                        a[...] = 0


# ---- unfold --------------------------------------------------------------------------------------------------------------------
def test_unfold_ramps_fold_and_hold_invalid_gates():
    scenes = ps.unfold_scenes()
    for R, G in ps.SHAPES:
        s = scenes[f"ramp_{R}x{G}"]
        out, folds = po.unfold(*s)
        invalid = ~np.isfinite(s.phidp) | (s.mask != 0)
        assert np.isnan(out[invalid]).all() and not folds[invalid].any() and not np.isnan(out[~invalid]).any()
        if G >= 128:
            assert folds.max() >= 1 and invalid.any() and (s.mask != 0).any() and np.isnan(s.phidp).any()


@pytest.mark.parametrize("name,wrap", [("seams", 360.0), ("seams_180", 180.0)])
def test_unfold_seam_rows(name, wrap):
    s = ps.unfold_scenes()[name]
    assert s.wrap == wrap and s.phidp.shape == (7, 200)
    out, K = po.unfold(*s)
    # 0: the folds sit across the seams
    assert K[0, 63] == 0 and K[0, 64] == 1 and K[0, 127] == 1 and K[0, 128] == 2
    # 1: the previous valid gate is gate 60, the whole trip 64 .. 127 is invalid
    assert np.isnan(s.phidp[1, 61:131]).all() and K[1, 60] == 0 and K[1, 131] == 1 and np.isnan(out[1, 64:128]).all()
    # 2, 3
    assert np.isnan(out[2]).all() and not K[2].any() and np.isinf(s.phidp[2]).sum() == 2 and s.mask[2, 150]
    assert np.isnan(out[3, :-1]).all() and out[3, -1] == s.phidp[3, -1] and not K[3].any()
    # 4: exactly half is no fold, one ulp beyond is
    half = np.float32(0.5 * wrap)
    assert s.phidp[4, 5] == half and s.phidp[4, 7] == -half
    assert K[4, 5] == 0 and K[4, 6] == 0 and K[4, 7] == 0 and K[4, 8] == 0
    assert K[4, 9] == -1 and K[4, 10] == 0 and K[4, 11] == 1 and K[4, 12] == 0
    # 5: up, back through 0, negative
    assert K[5, 2] == 1 and K[5, 3] == 0 and K[5, 8] == -1 and K[5].min() <= -2
    # 6: the fold is found across +-inf and a masked gate; the masked gate 128 changes nothing
    assert np.isinf(s.phidp[6, 60:62]).all() and s.mask[6, 62] and K[6, 59] == 0 and K[6, 63] == 1
    assert np.isnan(out[6, 60:63]).all() and K[6, 127] == 1 and K[6, 128] == 0 and K[6, 129] == 1 and np.isnan(out[6, 128])


def test_the_halved_rows_are_exact_halves():
    a, b = ps.unfold_scenes()["seams"], ps.unfold_scenes()["seams_180"]
    same = np.isnan(a.phidp) == np.isnan(b.phidp)
    assert same.all() and np.array_equal(b.phidp[~np.isnan(b.phidp)] * np.float32(2.0), a.phidp[~np.isnan(a.phidp)])
    assert np.array_equal(po.unfold(*a)[1], po.unfold(*b)[1])


# ---- fit -----------------------------------------------------------------------------------------------------------------------
def _fit(s, **kw):
    args = dict(half_window=s.half_window, min_valid=s.min_valid, dbz=s.dbz, edges=s.edges, centre_only=s.centre_only)
    args.update(kw)
    return po.fit(s.phi, 500.0 / (65536.0 * s.spacing), **args)


def test_fit_shape_scenes_reach_every_class_edge_and_nan():
    scenes = ps.fit_scenes()
    assert {scenes[f"fit_{R}x{G}"].centre_only for R, G in ps.SHAPES} == {False, True}
    for R, G in ps.SHAPES:
        s = scenes[f"fit_{R}x{G}"]
        L = po.half_windows(s.dbz, s.phi.shape, s.edges, s.half_window)
        if R * G >= 63:
            assert set(np.unique(L)) == set(ps.HALF4) and np.isnan(s.dbz).any()
            assert all((s.dbz == np.float32(e)).any() for e in s.edges)
        on_edge = s.dbz == np.float32(s.edges[1])
        assert (L[on_edge] == ps.HALF4[2]).all() and (L[np.isnan(s.dbz)] == ps.HALF4[0]).all()
        if G < 200:
            assert G <= max(ps.HALF4)                                     # G < L: the window is the whole ray


def test_fit_long_windows_are_clipped_at_both_ends_and_span_four_trips():
    s1, s255 = ps.fit_scenes()["l1"], ps.fit_scenes()["l255"]
    assert s1.half_window == (1,) and s255.half_window == (255,) and s255.phi.shape == (2, 200)
    n_valid = (~np.isnan(s255.phi)).sum(axis=1)
    count = _fit(s255).count
    assert (count == n_valid[:, None]).all()                              # every window is the whole ray: gates 0 .. 199
    assert _fit(s1).count.max() == 3 and _fit(s1).count[:, 0].max() <= 2


def test_fit_sparse_rows():
    s = ps.fit_scenes()["sparse"]
    f = _fit(s)
    assert s.min_valid == 3 and s.half_window == (5,)
    # row 0: N = min_valid is fitted, N = min_valid - 1 is not, side by side
    assert f.count[0, 11] == 4 and f.count[0, 10] == 3 and f.count[0, 9] == 2 and f.count[0, 5] == 1
    assert not np.isnan(f.kdp[0, 10]) and np.isnan(f.kdp[0, 9]) and np.isnan(f.phi_s[0, 5])
    # row 3: every valid gate of the window lies on one side of the centre
    assert f.count[3, 12] == 3 and np.isnan(s.phi[3, 12]) and not np.isnan(f.kdp[3, 12])
    assert abs(f.kdp[3, 12] - 0.37 * 500.0 / 125.0) < 1e-3
    p = _fit(ps.fit_scenes()["pairs"])
    # two valid gates: den = 2 * (j1^2 + j2^2) - (j1 + j2)^2 = (j1 - j2)^2 > 0; one: den = 0
    assert p.count[1, 30] == 2 and not np.isnan(p.kdp[1, 30]) and p.count[2, 30] == 1 and np.isnan(p.kdp[2, 30])
    assert p.count[4, 63] == 2 and not np.isnan(p.kdp[4, 63])
    assert np.isnan(p.kdp[2]).all() and (p.count[2, :61] == 1).all() and p.count[2, 61:].max() == 0


def test_fit_limits():
    s = ps.fit_scenes()["limits"]
    f = _fit(s)
    assert abs(s.phi[0, 20]) == 2.0 ** 14 and abs(s.phi[0, 40]) > 2.0 ** 14 and abs(s.phi[1, 40]) > 2.0 ** 14
    assert (f.count[:, 20] == 9).all() or f.count[2, 20] == 8
    assert f.count[0, 20] == 9 and f.count[0, 40] == 8 and f.count[1, 20] == 9 and f.count[1, 40] == 8
    assert f.count[2, 20] == 8 and f.count[2, 40] == 8


def test_fit_gaps_are_filled_unless_centre_only():
    a, b = ps.fit_scenes()["gaps"], ps.fit_scenes()["gaps_centre"]
    assert np.array_equal(a.phi, b.phi, equal_nan=True) and not a.centre_only and b.centre_only
    fa, fb = _fit(a), _fit(b)
    hole = np.isnan(a.phi)
    assert (~np.isnan(fa.kdp[hole])).sum() > 50 and np.isnan(fb.kdp[hole]).all()
    assert np.array_equal(po.bits(fa.kdp)[~hole], po.bits(fb.kdp)[~hole]) and np.array_equal(fa.count, fb.count)


# ---- attenuation ---------------------------------------------------------------------------------------------------------------
def _att(s):
    return po.attenuation(s.phi_s, s.dbz, alpha=s.alpha, beta=s.beta, max_dphi=s.max_dphi, zdr=s.zdr, phi0=s.phi0)


def test_attenuation_paths():
    s = ps.attenuation_scenes()["paths"]
    a = _att(s)
    m = a.dphi
    assert s.phi0 is None and s.max_dphi == 100.0
    assert np.isnan(s.phi_s[0, :130]).all() and not m[0, :131].any() and m[0, 131] == 0.5 and m[0, -1] == 34.5   # 0
    assert np.isnan(s.phi_s[1, 58:70]).all() and (m[1, 58:70] == m[1, 57]).all() and (m[1, 120:136] == m[1, 119]).all()
    assert m[1, 136] >= m[1, 119] > m[1, 70] >= m[1, 57] > 0                                                      # 1
    assert not m[2, :40].any() and (m[2, 40:] == 5.0).all()                                                       # 2
    assert not m[3].any()                                                                                         # 3
    assert m[4, 66] == 99.0 and (m[4, 67:] == 100.0).all()                                                        # 4
    assert not m[5].any() and np.array_equal(po.bits(a.dbz[5]), po.bits(s.dbz[5]))                                # 5
    assert np.isnan(a.dbz[6, ::3]).all() and not np.isnan(a.dbz[6, 1::3]).any()                                   # 6
    assert m[7, 70] == m[7, 69] and (m[7, 150:] == 100.0).all() and m[7, 149] < 100.0                             # 7
    assert (np.diff(m, axis=1) >= 0).all() and not np.signbit(m).any()


def test_attenuation_paths_with_origins_given():
    s = ps.attenuation_scenes()["paths_phi0"]
    free = ps.attenuation_scenes()["paths"]
    a, b = _att(s), _att(free._replace(zdr=None, alpha=s.alpha, beta=s.beta))
    assert np.isnan(s.phi0[[0, 2, 6]]).all() and a.zdr is None
    for r in (0, 2, 6):                                                   # NaN: the ray's own first value
        assert np.array_equal(a.dphi[r], b.dphi[r])
    assert not a.dphi[3].any() and s.phi0[3] > np.nanmax(s.phi_s[3])      # e < 0 everywhere
    assert a.dphi[4, 0] == 10.0 and a.dphi[5].max() == 0.0                # an origin below the first gate; no phi_s at all
    assert a.dphi[1, 0] == 0.0 and a.dphi[1, -1] > 40.0


def test_attenuation_shape_scenes_have_leading_nan_runs():
    scenes = ps.attenuation_scenes()
    for R, G in ps.SHAPES:
        s = scenes[f"att_{R}x{G}"]
        a = _att(s)
        assert (np.diff(a.dphi, axis=1) >= 0).all() and a.zdr is not None
        if R > 1 and G >= 2:
            assert np.isnan(s.phi_s[1, :G // 2]).all()


# ---- weather -------------------------------------------------------------------------------------------------------------------
def test_weather_scene():
    """The figures the scene was specified with: it folds once; the unfolded field is within 1.2e-5 degrees of the unwrapped
    truth; L = 15 gives 2.02 +- 0.11 deg/km in the first block; the end-of-ray dphi is 134.1 .. 137.0 degrees for a true 134.4.
    The last figure is the path above the scene's system offset, so the offset goes in as ``phi0``: the origin then carries no
    noise and the running maximum over the plateau can only sit above the truth.  With the origin left to the ray's first fitted
    value (sigma / sqrt(16) = 0.75 degrees of noise at the clipped window of gate 0, and it enters with its sign) the same rays
    end 133.55 .. 135.57: below the stated range, so that use gets a bound of its own, derived, not fitted -- origin and maximum
    each off by less than 2.5 degrees."""
    w = ps.weather()
    assert w.phidp.shape == (9, 300) and w.spacing == 240.0 and w.offset == 100.0
    assert abs((w.clean[0, -1] - w.clean[0, 0]) - 134.4) < 1e-9 and abs(w.clean[0, 0] - w.offset) < 1e-9
    hole = np.isnan(w.phidp)
    assert 0.03 < hole.mean() < 0.07
    out, K = po.unfold(w.phidp, None, 360.0)
    assert K.max() == 1 and K.min() == 0 and (K[:, -40:][~hole[:, -40:]] == 1).all()          # it folds once
    assert not K[:, :150].any()                     # (around 180 degrees the noise crosses the wrap back and forth: K is 0 or 1)
    assert np.abs(out[~hole].astype(np.float64) - w.truth[~hole]).max() <= 1.2e-5
    f = po.fit(out, 500.0 / (65536.0 * w.spacing), half_window=(15,), min_valid=8)
    lo, hi, kdp = w.blocks[0]
    inside = f.kdp[:, lo + 15:hi - 15]                                                        # windows wholly inside the block
    assert kdp == 2.0 and inside.shape == (9, 20) and abs(float(inside.mean()) - 2.02) <= 0.11
    known = po.attenuation(f.phi_s, w.dbz, alpha=0.08, beta=0.02, max_dphi=360.0, zdr=w.zdr, phi0=np.full(9, w.offset, np.float32))
    assert (known.dphi[:, -1] >= 134.1).all() and (known.dphi[:, -1] <= 137.0).all()
    a = po.attenuation(f.phi_s, w.dbz, alpha=0.08, beta=0.02, max_dphi=360.0, zdr=w.zdr)
    assert (np.abs(a.dphi[:, -1] - 134.4) < 5.0).all()                                        # the origin found on the ray
    # the correction puts back most of the 10.75 dB lost behind the second block
    behind = slice(200, 300)
    assert np.abs((w.dbz_true - w.dbz)[:, behind].mean() - 0.08 * 134.4) < 1e-3
    assert np.abs((a.dbz - w.dbz_true)[:, behind]).mean() < 0.3
    assert np.abs((known.dbz - w.dbz_true)[:, behind]).mean() < 0.3
