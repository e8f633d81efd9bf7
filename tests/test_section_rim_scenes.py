"""The scenes of tests/section_rim_scenes.py hold what they promise, checked with the float64 reference alone (no GPU): the
planted cases are covered, their labels are what ``roi_rim.classify`` says from scratch and what ``brute_pairs`` sees, the
float32 emulation the planting rests on agrees with exact rational arithmetic around non-lattice points, and the sparse,
dense, scattered and duplicate point sets have the properties the GPU tests rely on."""
import numpy as np
import pytest

import section_rim_scenes as srs
from oracle import roi_rim
from test_gpu_roi_rim import _values_and_mask

ALL = srs.MAIN + srs.EDGES


@pytest.mark.parametrize("name", ALL)
def test_planted_cases_are_covered_and_labelled(name):
    s, c = srs.scene(name), srs.cloud(name)
    counts = c.counts()
    print(f"{name}: {counts} ({len(c)} planted gates)")
    assert c.misses == 0
    for case, n in s.need.items():
        assert counts[case] >= n, (name, case, counts)
    assert s.need["A"] >= 20 and s.need["B"] >= 20 and s.need["C"] >= 10 and s.need["E"] >= 20
    assert np.all((c.voxel >= 0) & (c.voxel < s.nz * s.n))
    np.testing.assert_array_equal(srs.relabel(name), c.case)
    own = srs.own_membership(name)
    assert own[np.isin(c.case, ["A", "B"])].all()
    assert not own[np.isin(c.case, ["C", "D"])].any()


@pytest.mark.parametrize("name", ["sparse_minr", "dense_minr", "duplicates"])
def test_integer_scenes_hold_exact_rim_gates(name):
    s, c = srs.scene(name), srs.cloud(name)
    assert s.need["D"] >= 20
    d = np.nonzero(c.case == "D")[0]
    for j in d:
        rim = srs.sample_rim(s, c.voxel[j])
        assert roi_rim.d2_f64(c.gx[j:j + 1], c.gy[j:j + 1], c.gz[j:j + 1], rim.x, rim.y, rim.z)[0] == rim.r2


def test_float32_emulation_is_exact_around_non_lattice_points():
    """d2f_kernel (round-to-odd through float64) against d2f_exact (rationals) on planted gates of the beam scenes, whose
    points are not integers"""
    checked = 0
    for name in ("sparse_beam", "dense_beam"):
        s, c = srs.scene(name), srs.cloud(name)
        assert np.any(s.xs != np.round(s.xs)) and np.any(s.ys != np.round(s.ys))
        for j in range(0, len(c), 2):
            rim = srs.sample_rim(s, c.voxel[j])
            fast = roi_rim.d2f_kernel(c.gx[j:j + 1], c.gy[j:j + 1], c.gz[j:j + 1], rim.x, rim.y, rim.z)[0]
            assert fast == roi_rim.d2f_exact(c.gx[j], c.gy[j], c.gz[j], rim.x, rim.y, rim.z), (name, j)
            checked += 1
    assert checked >= 200


@pytest.mark.parametrize("name", srs.SPARSE)
def test_sparse_scenes_keep_every_gate_to_its_own_sample(name):
    s, c = srs.scene(name), srs.cloud(name)
    ip, idx, _, _ = srs.pairs(name)
    m = srs.membership(ip, idx, len(c))
    m[c.voxel, np.arange(len(c))] = False
    assert not m.any()
    assert s.n % srs.KPTS == (1 if name == "sparse_minr" else 3)
    # the four points of a block of sparse_beam have four different radii at every level
    if name == "sparse_beam":
        r = s.radius()
        assert all(len(set(r[k, b0:b0 + srs.KPTS])) == min(srs.KPTS, s.n - b0) for k in range(s.nz) for b0 in range(0, s.n, srs.KPTS))


def test_samples_with_a_lone_case_a_neighbour():
    """Samples whose only unmasked neighbour is a case-A gate (a float32 Cressman weight would be <= 0), under the mask the
    GPU test grids with"""
    for name in ("sparse_minr", "scattered"):
        c = srs.cloud(name)
        _, mask = _values_and_mask(c.voxel, len(c), seed=3)
        assert srs.a_only_samples(name, mask) >= 10, name


@pytest.mark.parametrize("name", srs.DENSE)
def test_dense_scenes_split_gates_within_a_block(name):
    s = srs.scene(name)
    assert s.n % srs.KPTS == (1 if name == "dense_minr" else 2)
    step = np.hypot(np.diff(s.xs.astype(np.float64)), np.diff(s.ys.astype(np.float64)))
    assert step.max() < 80.0 and s.radius().min() >= 1000.0
    assert srs.split_within_block(name) >= 50
    assert np.diff(srs.background_pairs(name)[0]).max() > 256          # two laps of the kernel's 128-entry ring


def test_scattered_blocks_are_wide_and_mix_radii():
    s = srs.scene("scattered")
    sparse, dense = srs.scene("sparse_beam"), srs.scene("dense_beam")
    have = sorted(zip(s.xs.tolist(), s.ys.tolist()))
    assert have == sorted(zip(np.concatenate([sparse.xs, dense.xs]).tolist(), np.concatenate([sparse.ys, dense.ys]).tolist()))
    full = s.n // srs.KPTS                                              # the last block holds one point
    assert s.n == 61 and full == 15
    assert srs.block_extents(s)[:full].min() >= 20e3
    ratios = srs.block_radius_ratios(s)[0]                              # at the lowest level
    assert np.count_nonzero(ratios >= 3.0) * 4 >= len(ratios), ratios


def test_duplicate_rows_are_identical():
    s = srs.scene("duplicates")
    ip, idx, d2, r2 = srs.pairs("duplicates")
    for group in srs.DUPLICATE_GROUPS:
        assert len({(float(s.xs[i]), float(s.ys[i])) for i in group}) == 1
        for k in range(s.nz):
            rows = [k * s.n + i for i in group]
            first = rows[0]
            assert ip[first + 1] > ip[first]
            for r in rows[1:]:
                np.testing.assert_array_equal(idx[ip[r]:ip[r + 1]], idx[ip[first]:ip[first + 1]])
                np.testing.assert_array_equal(d2[ip[r]:ip[r + 1]], d2[ip[first]:ip[first + 1]])
    assert srs.DUPLICATE_GROUPS[0][0] % srs.KPTS == 0 and len(srs.DUPLICATE_GROUPS[0]) == srs.KPTS      # a whole block
    assert srs.DUPLICATE_GROUPS[1][0] // srs.KPTS != srs.DUPLICATE_GROUPS[1][-1] // srs.KPTS           # across a seam


@pytest.mark.parametrize("name", srs.EDGES)
def test_edge_points_lie_on_the_rectangle_and_their_gates_beyond_it(name):
    s, c = srs.scene(name), srs.cloud(name)
    x0, x1, y0, y1 = srs.edge_rectangle(name.split("_")[1])
    on_x, on_y = (s.xs == x0) | (s.xs == x1), (s.ys == y0) | (s.ys == y1)
    assert np.count_nonzero(on_x & on_y) == 4 and np.count_nonzero(on_x ^ on_y) == 4
    assert s.xs[8] == 0.0 and s.ys[8] == 0.0 and x0 < 0.0 < x1 and y0 < 0.0 < y1
    member = srs.own_membership(name)
    outside = (c.gx < x0) | (c.gx > x1) | (c.gy < y0) | (c.gy > y1)
    border = c.voxel % s.n < 8
    assert outside[border].all() and np.count_nonzero(member & border) >= 50
    # straight above and below (0, 0): the gate just inside is a neighbour, the gate just outside is not
    vert = np.arange(len(c) - srs.n_vertical(name), len(c))
    assert np.all(c.gx[vert] == 0.0) and np.all(c.gy[vert] == 0.0) and vert.size == 4 * s.nz
    np.testing.assert_array_equal(member[vert], np.arange(vert.size) % 2 == 0)
