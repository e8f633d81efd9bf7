"""The scenes of tests/batch_stream_scenes.py can tell an ordered stream from an unordered one -- proved on the CPU, since
no broken build is ever run on the device.  A pass that read the staging set of another group, or of an earlier call, grids
another volume; that is visible only if every two volumes differ, in their values and in their masks."""
import itertools

import numpy as np
import pytest

import batch_stream_scenes as bs

SHARE = 0.01                       # any two volumes differ on at least this share of the gates both leave unmasked


def _all_volumes():
    return [(which, b, vol) for which in ("A", "B") for b, vol in enumerate(bs.batch(which))]


def test_batches_are_disjoint_and_read_only():
    assert not set(bs.SEEDS["A"]) & set(bs.SEEDS["B"])
    assert len(bs.SEEDS["A"]) == len(bs.SEEDS["B"]) == bs.N_VOLUMES
    for _, _, vol in _all_volumes():
        assert tuple(vol) == bs.FIELDS
        for name, (values, mask) in vol.items():
            assert values.dtype == np.float32 and values.shape == (bs.n_gates(),) and not values.flags.writeable
            assert (mask is None) == (name in bs.UNMASKED)
            if mask is not None:
                assert mask.dtype == bool and mask.shape == values.shape and not mask.flags.writeable
                assert 0 < mask.sum() < mask.size


def test_unmasked_fields_need_no_mask():
    """A field handed over with ``mask=None`` has no gate the oracle would exclude."""
    for which, b, vol in _all_volumes():
        for name in bs.UNMASKED:
            assert np.isfinite(vol[name][0]).all() and not np.ma.getmaskarray(bs.masked_field(which, b, name)).any()


@pytest.mark.parametrize("name", bs.FIELDS)
def test_any_two_volumes_differ(name):
    """Values on at least 1 % of the gates both leave unmasked, and the masks themselves -- A against B included."""
    worst = 1.0
    for (wa, a, va), (wb, b, vb) in itertools.combinations(_all_volumes(), 2):
        (xa, ma), (xb, mb) = va[name], vb[name]
        live = np.ones(xa.shape, bool) if ma is None else ~(ma | mb)
        assert live.sum() > 0.25 * live.size
        share = float((xa[live] != xb[live]).mean())
        worst = min(worst, share)
        assert share >= SHARE, (name, wa, a, wb, b, share)
        if ma is not None:
            assert (ma != mb).mean() >= 0.001, (name, wa, a, wb, b)
    print(f"{name}: the closest two volumes differ on {100.0 * worst:.1f} % of their live gates")


def test_both_paths_run_four_groups_with_a_short_last_one():
    for path, (names, per_pass) in bs.PATHS.items():
        assert set(names) <= set(bs.FIELDS) and set(names) & set(bs.UNMASKED) and set(names) - set(bs.UNMASKED)
        sizes = bs.group_sizes(bs.N_VOLUMES, len(names), per_pass)
        assert sizes == [2, 2, 2, 1], (path, sizes)                      # both staging sets are reused; the last upload is partial
    # the repeated calls: 7, then 2, then 5 volumes -- four groups, one group, three groups
    assert [len(picks) for _, picks in bs.CALLS] == [7, 2, 5]
    for path, (names, per_pass) in bs.PATHS.items():
        assert [len(bs.group_sizes(len(p), len(names), per_pass)) for _, p in bs.CALLS] == [4, 1, 3]
    assert bs.group_sizes(5, 2, 4) == [2, 2, 1] and bs.group_sizes(5, 2, 8) == [4, 1]      # what tests/test_gpu_batch.py sees
    assert bs.group_sizes(3, 8, 8) == [1, 1, 1] and bs.group_sizes(1, 3, 8) == [1]
    for which, b in bs.ANCHORED:
        assert 0 <= b < bs.N_VOLUMES and which in bs.SEEDS
    assert len(bs.ANCHORED) >= 2


def test_every_kind_is_placed_and_the_mixtures_mix():
    for kind in bs.KINDS:
        for i in range(bs.N_VOLUMES):
            for name in bs.FIELDS:
                values, mask = bs.placement(kind, i, name)
                assert values in ("numpy", "pinned", "device", "device_strided") and mask in bs.HOST + ("device", "device_bool")
    used = {p for kind in bs.KINDS for i in range(bs.N_VOLUMES) for name in bs.FIELDS for p in bs.placement(kind, i, name)}
    assert used == set(bs.HOST + bs.DEVICE)
    for path, (names, per_pass) in bs.PATHS.items():
        sizes = bs.group_sizes(bs.N_VOLUMES, len(names), per_pass)
        # across the volumes of one group: every full group holds a host-resident and a device-resident volume, or two host kinds
        i = 0
        seen = set()
        for size in sizes:
            where = [bs.placement("mixed_volumes", i + j, names[0])[0] for j in range(size)]
            seen.add(tuple(w in bs.HOST for w in where))
            if size > 1:
                assert len(set(where)) > 1, (path, i)
            i += size
        assert (True, False) in seen and (False, True) in seen            # host first and device first
        # inside one volume: host and device arrays side by side, in values and in masks
        inside = [p for name in names for p in bs.placement("mixed_fields", 0, name)]
        assert set(inside) & set(bs.HOST) and set(inside) & set(bs.DEVICE), path
        assert any(bs.placement("mixed_fields", 0, n)[1] in bs.DEVICE and bs.placement("mixed_fields", 0, n)[0] in bs.HOST
                   for n in names), path                                   # a device mask next to host values: one staging slot, half used
