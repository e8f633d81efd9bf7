"""The kernels of csrc/rg_shear.hip against the NumPy restatement (tests/shear_oracle.py) on every scene of
tests/shear_scenes.py: azimuthal shear, divergence and fitted velocity BIT-equal and the count equal, with every subset of the
outputs; the median bit-equal; the chain equal to its two calls; the plane scene within the derived one-step bound of the
analytic slopes; overlapping buffers refused."""
import itertools

import numpy as np
import pytest

from radar_processor_amd import _native

import shear_oracle as so
import shear_scenes as ss

pytestmark = pytest.mark.gpu
OUTPUTS = ("azimuthal_shear", "radial_divergence", "velocity", "count")


def _window(s):
    import radar_processor_amd as rg
    return rg.ShearWindow(s["half_rays"], s["az_scale"], s["max_half_rays"], s["half_gates"], s["range_scale"])


def _run(s, want=OUTPUTS):
    import radar_processor_amd as rg
    return rg.velocity_shear_device(s["vel"], _window(s), mask=s["mask"], wrap_rays=bool(s["wrap"]), min_valid=s["min_valid"],
                                    min_fraction=s["min_fraction_q16"] / 65536.0, centre_only=bool(s["centre_only"]), want=want)


def _equal(got, ref, name):
    for member, want in zip(got[:3], ref[:3]):
        if member is not None:
            a, b = so.bits(member.cpu().numpy()), so.bits(want)
            assert a.shape == b.shape and np.array_equal(a, b), f"{name}: {int((a != b).sum())} of {a.size} gates differ"
    if got.count is not None:
        assert np.array_equal(got.count.cpu().numpy(), ref.count), name


@pytest.mark.parametrize("name", sorted(ss.scenes()))
def test_llsd_is_bit_equal_to_the_restatement(name):
    s, ref = ss.scenes()[name], ss.reference(name)
    from radar_processor_amd import shear
    assert shear._check_fit(s["min_valid"], s["min_fraction_q16"] / 65536.0, OUTPUTS)[1] == s["min_fraction_q16"]
    got = _run(s)
    assert all(member is not None and tuple(member.shape) == s["vel"].shape for member in got)
    _equal(got, ref, name)


@pytest.mark.parametrize("name", ["seams_wrap", "bands_open"])
def test_any_subset_of_the_outputs_has_the_same_bits(name):
    s, ref = ss.scenes()[name], ss.reference(name)
    for k in (1, 2, 3):
        for floats in itertools.combinations(OUTPUTS[:3], k):
            for want in (floats, floats + ("count",)):
                got = _run(s, want)
                assert [member is not None for member in got] == [o in want for o in OUTPUTS], want
                _equal(got, ref, f"{name} {want}")


def test_a_two_dimensional_input_is_one_sweep_and_tensors_are_taken_as_they_come():
    import torch
    s, ref = ss.scenes()["seams_wrap"], ss.reference("seams_wrap")
    dev = torch.device("cuda", 0)
    one = dict(s, vel=torch.from_numpy(s["vel"][1]).to(dev), mask=torch.from_numpy(s["mask"][1] != 0).to(dev),
               half_rays=torch.from_numpy(np.array(s["half_rays"])).to(dev), az_scale=torch.from_numpy(np.array(s["az_scale"])).to(dev))
    got = _run(one)
    assert tuple(got.azimuthal_shear.shape) == s["vel"].shape[1:] and got.count.dtype == torch.uint16
    _equal(got, so.Llsd(*(plane[1] for plane in ref)), "sweep 1 alone")
    # rays without gates: empty outputs, no launch
    import radar_processor_amd as rg
    empty = rg.velocity_shear_device(np.zeros((2, 40, 0), np.float32), rg.ShearWindow(np.zeros(0, np.int32), np.zeros(0), 16, 2, 1e-7))
    assert tuple(empty.azimuthal_shear.shape) == (2, 40, 0) and empty.velocity is None
    assert tuple(rg.median_filter_device(np.zeros((2, 40, 0), np.float32)).shape) == (2, 40, 0)


def test_plane_within_one_float32_step_of_the_analytic_slopes():
    """Where no edge clips the window, B = Si = Sj = 0, P = c1 A and Q = c2 C exactly (tests/test_shear_scenes.py), so
    al = (P C - 0) / (A C) is c1 after two roundings (the product, the quotient; relative 2^-52 at most) and al * az_scale after a
    third; the analytic c1 * az_scale[g] carries one.  Both are rounded to float32 once: values 2^-51 apart in float64 round to
    the same float32 or to neighbours.  So: at most ONE float32 step.  The same for c2 * range_scale."""
    s = ss.scenes()["plane"]
    got = _run(s)
    inside = ss.interior("plane")
    shear, div = got.azimuthal_shear.cpu().numpy(), got.radial_divergence.cpu().numpy()
    want_shear = np.broadcast_to((ss.PLANE["c1"] * s["az_scale"]).astype(np.float32)[None, None, :], shear.shape)
    want_div = np.float32(ss.PLANE["c2"] * s["range_scale"])
    for name, a, b in (("shear", shear[inside], want_shear[inside]), ("divergence", div[inside], np.full(inside.sum(), want_div))):
        steps = np.abs(a.view(np.int32).astype(np.int64) - b.view(np.int32).astype(np.int64))
        print(f"plane: {name}: {a.size} gates, largest distance {int(steps.max())} float32 steps")
        assert not np.isnan(a).any() and (np.sign(a) == np.sign(b)).all() and steps.max() <= 1, name
    # the fitted velocity at the centre of an unclipped window is the plane itself: c0 + c1 a + c2 g in 2^-16 m/s
    smooth = got.velocity.cpu().numpy()
    steps = np.abs(smooth[inside].view(np.int32).astype(np.int64) - s["vel"][inside].view(np.int32).astype(np.int64))
    assert steps.max() <= 1


def test_median_is_bit_equal_to_the_restatement():
    import radar_processor_amd as rg
    vel, mask = ss.median_data()
    for hr, hg, wrap, min_valid, centre in ss.median_cases():
        got = rg.median_filter_device(vel, half_rays=hr, half_gates=hg, mask=mask, wrap_rays=bool(wrap), min_valid=min_valid,
                                      centre_only=bool(centre)).cpu().numpy()
        want = so.median(vel, mask, hr, hg, wrap, min_valid, centre)
        assert np.array_equal(so.bits(got), so.bits(want)), (hr, hg, wrap, min_valid, centre)
        # a selection: every output is NaN or the bits of a valid input
        assert np.isin(so.bits(got), np.append(so.bits(vel[so.valid(vel, mask)]), so.NAN_BITS)).all()
    got = rg.median_filter_device(vel[0], half_rays=2, half_gates=1).cpu().numpy()
    assert np.array_equal(so.bits(got), so.bits(so.median(vel[0], None, 2, 1, 1, 1, 1)[0]))
    # more than one workgroup, and a gate count that is no multiple of anything
    s = ss.scenes()["bands_wrap"]
    got = rg.median_filter_device(s["vel"], half_rays=2, half_gates=2, mask=s["mask"], min_valid=3, centre_only=False).cpu().numpy()
    assert np.array_equal(so.bits(got), so.bits(so.median(s["vel"], s["mask"], 2, 2, 1, 3, 0)))


def test_the_chain_is_its_two_calls():
    import radar_processor_amd as rg
    s = ss.scenes()["bands_wrap"]
    w = _window(s)
    kw = dict(min_valid=s["min_valid"], min_fraction=0.125, want=OUTPUTS)
    chain = rg.azimuthal_shear_device(s["vel"], w, median=(1, 2), mask=s["mask"], **kw)
    filtered = rg.median_filter_device(s["vel"], half_rays=1, half_gates=2, mask=s["mask"])
    two = rg.velocity_shear_device(filtered, w, **kw)
    ref = so.llsd(so.median(s["vel"], s["mask"], 1, 2, 1, 1, 1), None, *ss.llsd_args(s)[2:8], s["min_valid"], 8192, 0)
    for a, b in zip(chain, two):
        assert a.cpu().numpy().tobytes() == b.cpu().numpy().tobytes()
    _equal(chain, ref, "chain")
    host = rg.velocity_shear(s["vel"], w, median=(1, 2), mask=s["mask"], **kw)
    assert all(isinstance(member, np.ndarray) for member in host)
    _equal(rg.VelocityShear(*(_Host(member) for member in host)), ref, "host variant")
    plain = rg.azimuthal_shear_device(s["vel"], w, median=None, mask=s["mask"], **kw)
    _equal(plain, so.llsd(*ss.llsd_args(dict(s, min_fraction_q16=8192))), "median=None")


class _Host:
    """An ndarray with the ``.cpu().numpy()`` of a tensor."""
    def __init__(self, a):
        self.a = a

    def cpu(self):
        return self

    def numpy(self):
        return self.a


def test_overlapping_buffers_are_refused_and_nothing_is_written():
    import torch
    import radar_processor_amd as rg
    lib = rg.load_library()
    dev = torch.device("cuda", 0)
    S, R, G = 1, 40, 64
    n = S * R * G
    buf = torch.full((3 * n,), 7.5, dtype=torch.float32, device=dev)
    half = torch.full((G,), 2, dtype=torch.int32, device=dev)
    scale = torch.full((G,), 1e-6, dtype=torch.float64, device=dev)
    P = _native.ptr
    vel, a, b = P(buf), P(buf) + 4 * n, P(buf) + 8 * n
    stream = _native.stream_ptr()
    for args, message in [((vel, 0, S, R, G, 1, 1, 1, 1, 1, vel, stream), "out overlaps vel"),
                          ((vel, 0, S, R, G, 1, 1, 1, 1, 1, vel + 4 * n - 4, stream), "out overlaps vel")]:
        assert lib.rg_polar_median_f32(*args) == _native.RG_EINVAL
        assert lib.rg_last_error().decode() == "rg_polar_median_f32: " + message
    for outs, message in [((vel, 0, 0, 0), "az_shear overlaps vel"), ((a, a, 0, 0), "az_shear overlaps divergence"),
                          ((a, 0, b, a + 4 * n - 2), "az_shear overlaps count"), ((0, 0, a, P(half)), "count overlaps "),
                          ((0, P(scale), 0, 0), "divergence overlaps ")]:             # whichever table lies there
        assert lib.rg_velocity_llsd_f32(vel, 0, S, R, G, P(half), P(scale), 16, 2, 1e-7, 1, 6, 0, 0, *outs, stream) == _native.RG_EINVAL
        assert lib.rg_last_error().decode().startswith("rg_velocity_llsd_f32: " + message)
    torch.cuda.synchronize()
    assert bool((buf == 7.5).all()) and bool((half == 2).all()) and bool((scale == 1e-6).all())
    # side by side they are taken
    assert lib.rg_velocity_llsd_f32(vel, 0, S, R, G, P(half), P(scale), 16, 2, 1e-7, 1, 6, 0, 0, a, b, 0, 0, stream) == _native.RG_OK
    torch.cuda.synchronize()
    assert bool((buf[:n] == 7.5).all()) and bool((buf[n:] == 0.0).all())          # a constant field: no shear, no divergence
