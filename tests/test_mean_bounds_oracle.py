"""The per-voxel error bound of oracle.mean_error_bound, checked on the CPU against the reference's fixtures.

The bound ``|got - m| <= gamma_{n+1} (S + |m|) + 2u |m| + delta D (1 + 2 delta)`` compares a float32 gridder with the
float64 mean ``m`` of its voxel, whatever the order of its float32 additions (derivation: the docstring of
oracle.mean_error_bound).  Here it is shown to be

 * sound: the reference's own float32 grids meet it on every g2 / g3 / g4 / g6 fixture, every field, with and without the
   QC mask, with delta = u (its weights are float32 roundings of the float64 ones);
 * not vacuous: the median of |ref - m| / bound is reported and bounded below; the CSR-free gridder's float32 weights,
   emulated (oracle.roi_rim.k2_weights_f32), stay within the budgets rg_roi_grid.hip states, and grids made with them meet
   the bound with those budgets;
 * sharp enough to matter: one weight scaled by 1 + 1e-4, Barnes weights without their ``+ 1e-5`` and the all-float32
   Cressman weight the CSR-free gridder once used each break it on some fixture voxel.
"""
import functools

import numpy as np
import pytest

from conftest import builder_kwargs, golden_names, grid_spec, load_golden, reference_indices, volume_for
from oracle import radar_grid_oracle as oracle
from oracle import roi_rim

FIXTURES = golden_names("g2_") + golden_names("g3_") + golden_names("g4_") + golden_names("g6_")
WITH_PAIRS = [n for n in FIXTURES if n != "g3_c2_corner_barnes2"]       # the corner window has no neighbours


@functools.lru_cache(maxsize=None)
def _fixture(name):
    """meta, reference arrays, volume, the reference CSR's pair geometry and its float64 weights."""
    meta, ref = load_golden(name)
    vol = volume_for(meta)
    shape, limits = grid_spec(meta)
    kw = builder_kwargs(meta)
    weighting = kw.pop("weighting")
    kw.pop("toa")
    idx = reference_indices(name, meta, ref)
    pairs = oracle.pair_geometry(ref["indptr"], idx, vol.gate_x, vol.gate_y, vol.gate_z, shape, limits, **kw)
    return meta, ref, vol, idx, pairs, oracle.roi_weight_f64(pairs["d2"], pairs["r2"], weighting)


def _cases(name):
    """(field, reference grid key, data, mask) for every field, with and without the QC mask."""
    meta, ref, vol, *_ = _fixture(name)
    qc = None
    if "qc" in meta:
        qc = oracle.gate_mask("below", np.ma.getdata(vol.fields[meta["qc"][0]]), meta["qc"][1])
    for fname in meta["fields"]:
        data, mask = oracle.merge_masks(vol.fields[fname])
        yield fname, f"grid_{fname}", data, mask
        if qc is not None:
            data, mask = oracle.merge_masks(vol.fields[fname], [qc])
            yield fname, f"grid_{fname}_qc", data, mask


def _stats(name, mask, data):
    meta, ref, _, idx, _, w64 = _fixture(name)
    return oracle.voxel_stats(ref["indptr"], idx, w64, data, mask)


# ---- the model's inputs ------------------------------------------------------------------------------------------------
def test_bound_formula_known_values():
    """One live neighbour: m = v exactly, D = 0; two equal weights: m = (a + b) / 2 and D = |a - b| / 2."""
    ip = np.array([0, 1, 3, 3])
    idx = np.array([0, 1, 2])
    w = np.array([0.7, 0.25, 0.25])
    v = np.array([3.0, -1.0, 5.0], dtype=np.float32)
    st = oracle.voxel_stats(ip, idx, w, v, np.zeros(3, dtype=bool))
    np.testing.assert_array_equal(st["n"], [1, 2, 0])
    np.testing.assert_allclose(st["m"][:2], [3.0, 2.0]); np.testing.assert_allclose(st["S"][:2], [3.0, 3.0])
    np.testing.assert_allclose(st["D"][:2], [0.0, 3.0], atol=1e-12)
    assert np.isnan(st["m"][2])
    u = oracle.U32
    b = oracle.mean_error_bound(st, 1e-6)
    np.testing.assert_allclose(b[:2], [oracle.gamma(2) * 6 + 2 * u * 3, oracle.gamma(3) * 5 + 2 * u * 2 + 1e-6 * 3 * (1 + 2e-6)])
    # the masked neighbour is gone: voxel 1 keeps one live value, m = 5
    st = oracle.voxel_stats(ip, idx, w, v, np.array([False, True, False]))
    assert st["n"][1] == 1 and st["m"][1] == 5.0 and st["D"][1] == 0.0
    # NaN patterns: a value where m is NaN (or the reverse) is an infinite violation
    r = oracle.bound_ratio(np.array([3.0, np.nan, 1.0], dtype=np.float32), oracle.voxel_stats(ip, idx, w, v, np.zeros(3, bool)), 0.0)
    assert r[0] <= 1.0 and np.isinf(r[1]) and np.isinf(r[2])
    # thousands of neighbours: the second-order form takes over, the bound never shrinks below it
    big = dict(m=np.array([1.0]), S=np.array([1.0]), D=np.array([1.0]), n=np.array([100_000]))
    assert oracle.mean_error_bound(big, 2e-6)[0] >= oracle.gamma(100_001) * 2


@pytest.mark.parametrize("name", WITH_PAIRS)
def test_exact_weights_are_what_the_reference_rounds(name):
    """delta = u for the CSR paths: every reference weight is within u (relative) of the float64 weight recomputed from
    its pair -- a float32 rounding of it."""
    meta, ref, _, _, _, w64 = _fixture(name)
    rel = np.abs(ref["weights"].astype(np.float64) - w64) / w64
    assert rel.max() <= oracle.DELTA_CSR[meta["weighting"]] * (1 + 1e-9), rel.max() / oracle.U32


def test_build_geometry_exact_weights_round_to_its_float32_weights():
    meta, ref = load_golden("g2_c1_near")
    vol = volume_for(meta)
    shape, limits = grid_spec(meta)
    ip, idx, w = oracle.build_geometry(vol.gate_x, vol.gate_y, vol.gate_z, shape, limits, **builder_kwargs(meta))
    ip64, idx64, w64 = oracle.build_geometry(vol.gate_x, vol.gate_y, vol.gate_z, shape, limits, exact_weights=True,
                                             **builder_kwargs(meta))
    assert w64.dtype == np.float64 and np.array_equal(ip, ip64) and np.array_equal(idx, idx64)
    np.testing.assert_array_equal(w64.astype(np.float32), w)
    kw = builder_kwargs(meta)
    kw.pop("toa")
    np.testing.assert_array_equal(oracle.pair_weights_f64(ip, idx, vol.gate_x, vol.gate_y, vol.gate_z, shape, limits, **kw),
                                  w64)


# ---- 1. sound ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", FIXTURES)
def test_reference_grids_meet_the_bound(name):
    meta, ref, *_ = _fixture(name)
    delta = oracle.DELTA_CSR[meta["weighting"]]
    report = []
    for fname, key, data, mask in _cases(name):
        r = oracle.bound_ratio(ref[key], _stats(name, mask, data), delta)
        assert r.max(initial=0) <= 1.0, (key, r.max())
        nz = r[r > 0]
        med = float(np.median(nz)) if nz.size else 0.0
        report.append(f"{key}: worst {r.max(initial=0):.3f} median {med:.4f}")
        # not vacuous: the typical error is a sizeable fraction of the bound, not a thousandth of it
        assert nz.size == 0 or med >= 1e-3, (key, med)
    print(name, "; ".join(report))


# ---- 2. the CSR-free gridder's weights, emulated -----------------------------------------------------------------------
@pytest.mark.parametrize("name", WITH_PAIRS)
def test_k2_weights_within_the_stated_budget_and_their_grids_meet_the_bound(name):
    meta, ref, _, idx, pairs, w64 = _fixture(name)
    weighting = meta["weighting"]
    k2 = roi_rim.k2_weights_f32(pairs, weighting)
    rel = np.abs(k2.astype(np.float64) - w64) / w64
    print(f"{name}: K2 {weighting} weights, worst relative error {rel.max():.3g} "
          f"({rel.max() / oracle.U32:.1f} u, budget {oracle.K2_WEIGHT_BUDGET[weighting]:.0e})")
    assert rel.max() <= oracle.K2_WEIGHT_BUDGET[weighting]
    shape, _ = grid_spec(meta)
    for fname, key, data, mask in _cases(name):
        got = oracle.csr_apply(ref["indptr"], idx, k2, data, mask, shape)
        r = oracle.bound_ratio(got, _stats(name, mask, data), oracle.DELTA_K2[weighting])
        assert r.max(initial=0) <= 1.0, (key, r.max())


# ---- 3. mutations the bound must catch ---------------------------------------------------------------------------------
@pytest.mark.parametrize("name", WITH_PAIRS)
def test_one_weight_scaled_by_1e_4_breaks_the_bound(name):
    """The pair whose weight moves its voxel's mean the most, w_i |v_i - m| / sum w, scaled by 1 + 1e-4."""
    meta, ref, _, idx, _, w64 = _fixture(name)
    shape, _ = grid_spec(meta)
    ip = ref["indptr"]
    fname, key, data, mask = next(_cases(name))
    st = _stats(name, mask, data)
    row = np.repeat(np.arange(ip.shape[0] - 1), np.diff(ip))
    live = ~mask[idx]
    W = np.bincount(row[live], weights=w64[live], minlength=ip.shape[0] - 1)
    with np.errstate(invalid="ignore", divide="ignore"):
        sens = np.nan_to_num(np.where(live, w64 * np.abs(data[idx] - st["m"][row]) / W[row], 0.0))
    w = ref["weights"].copy()
    k = int(np.argmax(sens))
    w[k] = np.float32(np.float64(w[k]) * (1 + 1e-4))
    r = oracle.bound_ratio(oracle.csr_apply(ip, idx, w, data, mask, shape), st, oracle.DELTA_CSR[meta["weighting"]])
    assert (r > 1).sum() >= 1 and r[row[k]] > 1, (key, r.max())


@pytest.mark.parametrize("name", [n for n in WITH_PAIRS if "cressman" not in n and "nearest" not in n])
def test_barnes_weight_without_its_floor_breaks_the_bound(name):
    """exp(-d2 / (r2 / 4)) without the ``+ 1e-5`` of compute.py:83, held to the K2 Barnes budget."""
    meta, ref, _, idx, pairs, _ = _fixture(name)
    shape, _ = grid_spec(meta)
    w = np.exp(-pairs["d2"] / (pairs["r2"] / 4)).astype(np.float32)
    broken = 0
    for fname, key, data, mask in _cases(name):
        r = oracle.bound_ratio(oracle.csr_apply(ref["indptr"], idx, w, data, mask, shape), _stats(name, mask, data),
                               oracle.DELTA_K2["barnes2"])
        broken += int((r > 1).sum())
    assert broken >= 1


def test_float32_cressman_numerator_breaks_the_bound_at_the_rim():
    """The all-float32 Cressman weight (r2f - d2f) / (r2f + d2f) on gates planted at the rim (oracle.roi_rim): it breaks
    the bound (and the NaN pattern, where a voxel's only live gate weighs <= 0); the kernel's float64 numerator meets it."""
    shape, limits = (2, 5, 9), ((500.0, 5500.0), (-10e3, 10e3), (-20e3, 20e3))
    cloud = roi_rim.rim_cloud(shape, limits, 1000.0, 0.0, seed=1, per_voxel=(2, 3))
    assert cloud.counts()["A"] >= 10
    ip, idx, w64 = oracle.build_geometry(cloud.gx, cloud.gy, cloud.gz, shape, limits, min_radius=1000.0, beam_factor=0.0,
                                         weighting="cressman", exact_weights=True)
    pairs = oracle.pair_geometry(ip, idx, cloud.gx, cloud.gy, cloud.gz, shape, limits, min_radius=1000.0, beam_factor=0.0)
    val = (np.arange(len(cloud)) * 0.37 - 4.0).astype(np.float32)
    mask = np.zeros(len(cloud), dtype=bool)
    st = oracle.voxel_stats(ip, idx, w64, val, mask)
    ratios = {}
    for numerator in ("f64", "f32"):
        w = roi_rim.k2_weights_f32(pairs, "cressman", cressman_numerator=numerator)
        ratios[numerator] = oracle.bound_ratio(oracle.csr_apply(ip, idx, w, val, mask, shape), st, oracle.DELTA_K2["cressman"])
    assert ratios["f64"].max() <= 1.0
    assert (ratios["f32"] > 1).sum() >= 5 and np.isinf(ratios["f32"]).sum() >= 1
