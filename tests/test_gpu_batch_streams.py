"""``batch.VolumeBatch.grid_shard`` under skewed streams: the one place in the library where two streams are ordered by hand.

Host-resident inputs are uploaded one group ahead on a copy stream into one of two persistent staging sets.  Three things
order that stream and the caller's: the event recorded behind a group's upload, the caller's stream waiting for it, and
``_staging_free[gi & 1]``, which keeps an upload out of a set until the pass that last read it is done.  With pageable
NumPy input (tests/test_gpu_batch.py) every copy is synchronous with the host and none of the three can be seen missing.

Here the reference of every comparison is the same call with every input already on the device -- no copy stream, no event
-- anchored once per path to ``oracle.csr_apply`` and then compared bit for bit.  A skew is a bounded delay
(``torch.cuda._sleep``, its rate measured when the module starts and asserted to be one that delays) enqueued on one
stream ahead of the call, with a marker event right behind it: the marker still pending when ``grid_shard`` returns shows
that the host enqueued the whole call while the device was held, so what the device then does is decided by the events
alone.  Under the delayed caller's stream every pass is slowed as well (a short delay in front of the gridding call,
patched in from here), so that an upload released too early lands before the pass reads its staging set, not in a race
with it.  The scenes (tests/batch_stream_scenes.py, held to their promises by tests/test_batch_stream_scenes.py) make every
two volumes differ, so a pass that read another group's staging set gives another grid.

Every skewed test runs on ``COPY_STREAMS`` fresh ``VolumeBatch`` objects, each of which takes the next stream of torch's
pool as its copy stream.  Found with the mutants of DESIGN §7: of four consecutive copy streams one hid a missing
``compute.wait_event(ready)`` and a ``_staging_free`` recorded too early, on both paths -- what a copy stream that shares
one of the process's four hardware queues with the caller's stream would do (kernels, barriers and event records of the
two then execute in the order the host submitted them; only the uploads themselves run free).  A single ``VolumeBatch``
would decide by its place in the file whether it can tell.  No path synchronises with the host inside the group loop:
the marker is asserted pending for both paths and for both reducers.

Measured on an MI355X (profiles/batch_stream_skew.json): ``torch.cuda._sleep`` spins 2.39e6 cycles per millisecond (asked 5 /
20 / 60 ms, measured 5.03 / 19.98 / 59.90); one unskewed call of the largest scene (3 fields x 7 volumes, four groups) spans
0.60 ms on the stream (0.61 at most in seven calls, 0.54 ms of it host enqueueing; 0.45 ms for the CSR path) on the parent
commit.  Twenty times that is 12.2 ms; the delay ahead of a call is 40 ms, with four slowed passes 60 ms per call.  The cycle
count of a delay comes from the rate measured when the module starts, and the marker decides at run time.
"""
import contextlib

import numpy as np
import pytest

from conftest import ATOL_FRAC
from oracle import radar_grid_oracle as oracle

import batch_stream_scenes as bs

pytestmark = pytest.mark.gpu

CALL_MS = 0.61                     # stream time of one unskewed call of the largest scene (3 fields x 7 volumes), the slowest of seven
COPY_STREAMS = 4                   # fresh VolumeBatches, hence copy streams, every skewed test runs on (see the module docstring)
PASS_DELAY_MS = 5.0                # in front of every pass of a call whose caller's stream is delayed
DELAY_MS = 40.0                    # ahead of the call: 65 x CALL_MS, room for a host that stalls for some milliseconds in mid-call
assert 20.0 * CALL_MS <= DELAY_MS and DELAY_MS + 4 * PASS_DELAY_MS <= 100.0
CALIBRATION_CYCLES = 4_000_000


class Skew:
    """Bounded delays on a stream.  ``delay`` returns a marker event recorded right behind the delay."""

    def __init__(self, dev):
        import torch
        self.dev = dev
        torch.cuda._sleep(1000)                                            # loads the kernel
        torch.cuda.synchronize()
        start, end = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        start.record()
        torch.cuda._sleep(CALIBRATION_CYCLES)
        end.record()
        end.synchronize()
        ms = start.elapsed_time(end)
        # 4e6 cycles in under 0.2 ms would be 20 GHz: the primitive does not delay here and another one is needed
        assert ms >= 0.2, f"torch.cuda._sleep({CALIBRATION_CYCLES}) took {ms} ms"
        self.cycles_per_ms = CALIBRATION_CYCLES / ms
        print(f"[skew] torch.cuda._sleep: {self.cycles_per_ms:.0f} cycles per ms")

    def delay(self, stream, ms):
        import torch
        with torch.cuda.stream(stream):
            torch.cuda._sleep(int(ms * self.cycles_per_ms))
            return stream.record_event()


def _place(where, a, dev):
    """One array of the scenes where ``batch_stream_scenes.placement`` says it lives."""
    import torch
    if a is None:
        return None
    is_mask = a.dtype == bool
    if where == "numpy":
        return np.array(a)                                                 # the scenes are read-only; torch.from_numpy wants a writable array
    if where == "pinned":
        return torch.from_numpy(np.array(a, dtype=np.uint8 if is_mask else np.float32)).pin_memory()
    if where == "pinned_bool":
        assert is_mask
        return torch.from_numpy(np.array(a)).pin_memory()
    t = torch.from_numpy(np.array(a)).to(dev)
    if where == "device":
        return t.to(torch.uint8) if is_mask else t
    if where == "device_bool":
        assert is_mask
        return t
    assert where == "device_strided" and not is_mask
    wide = torch.full((a.size, 2), float("nan"), dtype=torch.float32, device=dev)
    wide[:, 0] = t
    return wide[:, 0]


class World:
    """The geometry of both paths, the scenes placed per input kind (cached) and the reference grids."""

    def __init__(self, tmp):
        import torch
        import radar_processor_amd as rg
        assert torch.cuda.is_available()
        torch.cuda.set_device(0)
        self.dev = torch.device("cuda", 0)
        vol = bs.volume(bs.SEEDS["A"][0])                                 # every volume has the same gates
        geom = rg.compute_grid_geometry(vol.gate_x, vol.gate_y, vol.gate_z, bs.SHAPE, bs.LIMITS, str(tmp))
        search = rg.RoiSearch(vol.gate_x, vol.gate_y, vol.gate_z, bs.SHAPE, bs.LIMITS, device=self.dev)
        self.geometry = {"csr": geom, "fused": search}
        self.rows = oracle.canonical_rows(geom.indptr, geom.gate_indices, geom.weights)
        self._placed = {}
        self.skew = Skew(self.dev)
        # the reference: every input on the device, contiguous float32 / uint8 -- _stage returns no event, no copy stream runs
        self.ref = {}
        for path in bs.PATHS:
            for which in bs.SEEDS:
                vb = self.batch(path)
                self.ref[path, which] = vb.grid_shard(self.placed("device", which), rank=0, world_size=1)
                assert getattr(vb, "_staging", None) is None
        torch.cuda.synchronize()

    def batch(self, path):
        from radar_processor_amd import batch
        return batch.VolumeBatch(self.geometry[path], list(bs.PATHS[path][0]), device=self.dev)

    def batches(self, path):
        """``COPY_STREAMS`` fresh batches; each takes the next stream of torch's pool on its first call."""
        return [self.batch(path) for _ in range(COPY_STREAMS)]

    def placed(self, kind, which):
        key = (kind, which)
        if key not in self._placed:
            self._placed[key] = [{name: tuple(_place(where, a, self.dev) for where, a in zip(bs.placement(kind, b, name), pair))
                                  for name, pair in vol.items()} for b, vol in enumerate(bs.batch(which))]
        return self._placed[key]

    def groups(self, path, n_volumes):
        names, per_pass = bs.PATHS[path]
        return len(bs.group_sizes(n_volumes, len(names), per_pass))


@pytest.fixture(scope="module")
def world(tmp_path_factory):
    return World(tmp_path_factory.mktemp("batch_streams"))


def _bits(t):
    import torch
    return t.contiguous().view(-1).view(torch.uint8)


def _same(got, want):
    """Bit for bit, NaN patterns included; dicts and lists element by element."""
    import torch
    if isinstance(want, dict):
        assert list(got) == list(want)
        return all(_same(got[k], want[k]) for k in want)
    if isinstance(want, (list, tuple)):
        assert len(got) == len(want)
        return all(_same(g, w) for g, w in zip(got, want))
    assert got.shape == want.shape and got.dtype == want.dtype and got.device == want.device
    return torch.equal(_bits(got), _bits(want))


def _wrong(got, want, volumes=None):
    """The volumes of ``got`` (keyed by position in the call) that differ from ``want`` (keyed by volume number)."""
    volumes = sorted(want) if volumes is None else volumes
    assert sorted(got) == list(range(len(volumes)))
    return [b for i, b in enumerate(volumes) if not _same(got[i], want[b])]


def _assert_batch(got, want, volumes=None):
    wrong = _wrong(got, want, volumes)
    assert not wrong, f"volumes {wrong} differ from the device-resident reference"


@contextlib.contextmanager
def _slowed_passes(monkeypatch, skew, ms):
    """Every gridding call of ``grid_shard`` gets a delay of ``ms`` in front of it on the caller's stream."""
    import torch
    from radar_processor_amd import batch
    with monkeypatch.context() as patch:
        for name in ("grid_fields_device", "roi_grid_fields_device", "grid_products_device"):
            def slowed(*args, _real=getattr(batch, name), **kwargs):
                skew.delay(torch.cuda.current_stream(), ms)
                return _real(*args, **kwargs)
            patch.setattr(batch, name, slowed)
        yield


def _skewed_call(world, monkeypatch, vb, volumes, **kwargs):
    """``grid_shard`` with the caller's stream held for ``DELAY_MS`` and every pass slowed; returns ``(result, the marker
    was still pending when the call returned)``."""
    import torch
    torch.cuda.synchronize()
    with _slowed_passes(monkeypatch, world.skew, PASS_DELAY_MS):
        marker = world.skew.delay(torch.cuda.current_stream(), DELAY_MS)
        got = vb.grid_shard(volumes, rank=0, world_size=1, **kwargs)
        pending = not marker.query()
    torch.cuda.synchronize()
    return got, pending


# ---- the reference ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("path", bs.PATHS)
def test_reference_is_the_oracles_grid(world, path):
    """The device-resident run against ``oracle.csr_apply`` on two volumes: rtol 1e-5, ``ATOL_FRAC``, identical NaN sets."""
    names = bs.PATHS[path][0]
    for which, b in bs.ANCHORED:
        got = world.ref[path, which][b].cpu().numpy()
        for i, name in enumerate(names):
            data, mask = oracle.merge_masks(bs.masked_field(which, b, name))
            want = oracle.csr_apply(*world.rows, data, mask, bs.SHAPE)
            np.testing.assert_array_equal(np.isnan(got[i]), np.isnan(want))
            scale = float(np.abs(data[np.isfinite(data) & ~mask]).max())
            np.testing.assert_allclose(got[i], want, rtol=1e-5, atol=ATOL_FRAC * scale, equal_nan=True)
            assert np.isfinite(want).sum() >= 100                         # the oracle's grid: not an empty comparison


@pytest.mark.parametrize("path", bs.PATHS)
def test_reference_grids_of_any_two_volumes_differ(world, path):
    import torch
    grids = [world.ref[path, which][b] for which in bs.SEEDS for b in range(bs.N_VOLUMES)]
    flat = torch.stack([g.contiguous().view(-1).view(torch.int32) for g in grids])
    differ = (flat[:, None, :] != flat[None, :, :]).float().mean(dim=-1)
    differ.fill_diagonal_(1.0)
    assert float(differ.min()) >= 0.01, "two volumes grid alike: a pass that read the wrong staging set could pass"


# ---- 1: input kinds, no skew ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", bs.KINDS)
@pytest.mark.parametrize("path", bs.PATHS)
def test_input_kinds_equal_the_reference(world, path, kind):
    """Every input kind, with calls of 7, then 2, then 5 volumes on one ``VolumeBatch``: four, one and three groups, so the
    staging sets are reused within a call and carry events of the call before."""
    vb = world.batch(path)
    for which, picks in bs.CALLS:
        placed = world.placed(kind, which)
        events = []
        got = vb.grid_shard([placed[b] for b in picks], events=events, rank=0, world_size=1)
        assert len(events) == world.groups(path, len(picks))
        _assert_batch(got, world.ref[path, which], picks)


# ---- 2: the caller's stream delayed, page-locked input -----------------------------------------------------------------------------------
@pytest.mark.parametrize("path", bs.PATHS)
def test_uploads_wait_for_the_pass_that_reads_their_staging_set(world, path, monkeypatch):
    """The caller's stream is held while the host enqueues all four groups (asserted: the marker is pending at return), so
    the copy stream could run all four uploads at once.  Only ``_staging_free`` keeps the upload of group g + 2 out of the
    set group g is still to be gridded from.  Page-locked values with uint8 masks: a bool mask is converted on the host into
    a pageable temporary, and that copy waits for the copy stream, hence for the held pass (``Tensor.copy_``)."""
    wrong = {}
    for k, vb in enumerate(world.batches(path)):
        vb.grid_shard(world.placed("pinned_u8", "B"), rank=0, world_size=1)    # staging allocated; both sets hold B, with their events
        events = []
        got, pending = _skewed_call(world, monkeypatch, vb, world.placed("pinned_u8", "A"), events=events)
        assert pending, "the host did not enqueue the whole call while the caller's stream was held"
        assert len(events) == world.groups(path, bs.N_VOLUMES) == 4
        wrong[k] = _wrong(got, world.ref[path, "A"])
    assert not any(wrong.values()), f"volumes that differ from the device-resident reference, per copy stream: {wrong}"


# ---- 3: the copy stream delayed -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("path", bs.PATHS)
def test_passes_wait_for_their_upload(world, path):
    """Both staging sets hold batch A; the copy stream is held, then batch B is gridded.  A pass that did not wait for its
    upload would grid what the sets still hold: A's."""
    import torch
    wrong = {}
    for k, vb in enumerate(world.batches(path)):
        _assert_batch(vb.grid_shard(world.placed("pinned_u8", "A"), rank=0, world_size=1), world.ref[path, "A"])
        torch.cuda.synchronize()
        marker = world.skew.delay(vb._copy_stream, DELAY_MS)
        got = vb.grid_shard(world.placed("pinned_u8", "B"), rank=0, world_size=1)
        pending = not marker.query()
        torch.cuda.synchronize()
        assert pending, "the host did not enqueue the whole call while the copy stream was held"
        wrong[k] = _wrong(got, world.ref[path, "B"])
        assert wrong[k] or not any(_same(got[b], world.ref[path, "A"][b]) for b in range(bs.N_VOLUMES))
    assert not any(wrong.values()), f"volumes that differ from the device-resident reference, per copy stream: {wrong}"


# ---- 4: reducers under the skew of 2 ----------------------------------------------------------------------------------------------------
def _reducer(name):
    import radar_processor_amd as rg
    if name == "column_max":
        return lambda g: rg.column_max(g[0])
    return rg.PlaneProducts(cappi=(3000.0,), z_min_idx=1, z_max_idx=3)


@pytest.mark.parametrize("reducer", ("column_max", "plane_products"))
@pytest.mark.parametrize("path", bs.PATHS)
def test_reducers_under_a_delayed_callers_stream(world, path, reducer, monkeypatch):
    """A callable reducer and a ``PlaneProducts`` request: the same planes as the same call on device-resident input, one
    pair of events per group."""
    want = world.batch(path).grid_shard(world.placed("device", "A"), products=_reducer(reducer), rank=0, world_size=1)
    assert not _same(want[0], want[1])
    for vb in world.batches(path):
        vb.grid_shard(world.placed("pinned_u8", "B"), products=_reducer(reducer), rank=0, world_size=1)
        events = []
        got, pending = _skewed_call(world, monkeypatch, vb, world.placed("pinned_u8", "A"), products=_reducer(reducer), events=events)
        assert pending, "the host did not enqueue the whole call while the caller's stream was held"
        assert len(events) == 4
        _assert_batch(got, want)


# ---- 5: a staging buffer in a recycled block ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("path", bs.PATHS)
def test_first_upload_waits_for_the_blocks_previous_tenant(world, path):
    """The staging tensors come from the pool of the caller's stream.  A block of that pool may be handed out while work
    queued on the caller's stream still reads its previous tenant -- harmless on that stream, but the copy stream writes
    into it.  Here the previous tenant holds a pattern, a copy of it is queued behind a delay, the tenant is freed and the
    first call of a fresh ``VolumeBatch`` takes its block (asserted); the queued copy must still find the pattern."""
    import torch
    volumes = world.placed("pinned_u8", "A")
    pattern = checker = None
    for _ in range(COPY_STREAMS):
        vb = world.batch(path)
        shape = (vb.volumes_per_pass * len(vb.field_names), bs.n_gates())
        if pattern is None:
            pattern = (torch.arange(shape[0] * shape[1], dtype=torch.float32, device=world.dev) + 0.5).reshape(shape)
            checker = torch.empty_like(pattern)
        checker.zero_()
        torch.cuda.synchronize()
        torch.cuda.empty_cache()
        tenant = torch.empty(shape, dtype=torch.float32, device=world.dev)
        tenant.copy_(pattern)
        torch.cuda.synchronize()
        block = tenant.data_ptr()
        world.skew.delay(torch.cuda.current_stream(), DELAY_MS)
        checker.copy_(tenant)
        del tenant
        got = vb.grid_shard(volumes, rank=0, world_size=1)
        assert block in {buf.data_ptr() for pair in vb._staging for buf in pair}, "no staging buffer took the freed block"
        torch.cuda.synchronize()
        assert torch.equal(checker, pattern), "the first upload overwrote a block that queued work was still to read"
        _assert_batch(got, world.ref[path, "A"])
        del vb                                                             # its staging goes back to the pool


# ---- 6: a device-resident input whose producer is still queued ------------------------------------------------------------------------------
@pytest.mark.parametrize("path", bs.PATHS)
def test_conversion_of_a_device_input_waits_for_its_producer(world, path):
    """A group of page-locked inputs with one bool mask on the device.  The mask holds the complement of the real one; the
    write of the real one is queued on the caller's stream behind a delay.  The conversion to uint8 must read the real mask,
    as any other work the caller queues behind that write would."""
    import torch
    name = bs.PATHS[path][0][0]
    volumes = [dict(v) for v in world.placed("pinned_u8", "A")]
    real = torch.from_numpy(np.array(bs.batch("A")[0][name][1])).to(world.dev)
    mask = torch.logical_not(real)
    volumes[0][name] = (volumes[0][name][0], mask)
    for vb in world.batches(path):
        torch.logical_not(real, out=mask)
        torch.cuda.synchronize()
        marker = world.skew.delay(torch.cuda.current_stream(), DELAY_MS)
        mask.copy_(real)
        got = vb.grid_shard(volumes, rank=0, world_size=1)
        pending = not marker.query()
        torch.cuda.synchronize()
        assert pending, "the write of the real mask was not pending when the call was enqueued"
        _assert_batch(got, world.ref[path, "A"])
