"""Slab seams of the compact-only / packed-only geometry build (``geometry_builder._build_compact_only``), below full size.

``compute_grid_geometry(layout="auto")`` builds a large geometry one slab of whole grid levels at a time: gate indices and
weights go through base pointers shifted back by the slab's first pair, the row pointers are an int64 view that starts at a
non-zero entry, the per-level gate lists are addressed from ``level0``, the slab's dictionaries come from
``rg_csr_compact_count`` / ``rg_csr_compact_fill``, its record pointers are spliced behind the previous slab's, and
``rg_csr_compact_pack_dense`` rotates the dispatch order by ``plane0``.  With the default 1.2e9 pairs per slab every small
geometry is ONE slab; here the slab size is set so that seams fall between, before and after levels with and without pairs.

Truth never comes from the code under test: the reference's committed CSRs (tests/golden), the NumPy oracle
(oracle.build_geometry / pair_weights_f64 / csr_apply_rowwise_order / mean_error_bound) and the NumPy record encoder and
layout restatements of tests/slab_scenes.py.  Every test asserts the slabs it actually got (``_build`` counts the calls of
``CompactCSR._planes``, one per slab) against ``slab_scenes.slabs_for``.

 1. the kernels' slab arguments on a hand-made compact copy (5 x 7 x 130: ragged line group, three segments, every residue of
    the extra rotation): pack / count / fill called slab by slab for three partitions of the planes, and the apply kernels
    over the slab-packed records with int64 row pointers;
 2. the slab builder on every g3 / g4 / g6 fixture of the reference, seams at 1 pair, at ``L[i] + L[i+1]`` and one less, at a
    third of the pairs and above the total, both layouts;
 3. a scene three segments wide with dense, wide and empty chunks and a pair-less level, against the oracle: builds, gridding
    by the public path, products, decoding across seams, the interchange file and the layout policy.
"""
import contextlib

import numpy as np
import pytest

import slab_scenes as scenes
from conftest import (assert_same_to_rounding, builder_kwargs, golden_names, grid_spec, load_golden, reference_indices,
                      volume_for)
from oracle import radar_grid_oracle as oracle

pytestmark = pytest.mark.gpu

TOA = 17000.0


@pytest.fixture(scope="module")
def rg():
    import radar_processor_amd as pkg
    pkg.load_library()
    return pkg


# ---- helpers -------------------------------------------------------------------------------------------------------------
@contextlib.contextmanager
def _slab_spy():
    """Planes of every slab a build processes: ``_build_compact_only`` calls ``CompactCSR._planes`` once per slab."""
    from radar_processor_amd.grid_geometry import CompactCSR
    orig, planes = CompactCSR._planes, []

    def spy(indptr, gate_idx_ptr, n_planes, ny, nx, local_ptr):
        planes.append(int(n_planes))
        return orig(indptr, gate_idx_ptr, n_planes, ny, nx, local_ptr)
    CompactCSR._planes = staticmethod(spy)
    try:
        yield planes
    finally:
        CompactCSR._planes = staticmethod(orig)


def _build(search, weighting, limits, pairs_per_slab, packed):
    """``_build_compact_only`` wrapped as ``compute_grid_geometry`` wraps it -> ``(geometry or None, slabs)``."""
    from radar_processor_amd import geometry_builder
    from radar_processor_amd.grid_geometry import GridGeometry
    with _slab_spy() as planes:
        built = geometry_builder._build_compact_only(search, weighting, pairs_per_slab=pairs_per_slab, packed=packed)
    ends = np.cumsum(planes).tolist()
    slabs = list(zip([0] + ends[:-1], ends))
    if built is None:
        return None, slabs
    csr, compact = built
    return GridGeometry.from_device(search.grid_shape, limits, csr, search.toa, compact=compact), slabs


def _arrays(geom):
    """Row pointers, gate indices and weights as the geometry's readers rebuild them, and the record pointers."""
    csr, compact = geom.device_csr(), geom.device_compact()
    rec_ptr = None if compact.rec_ptr is None else compact.rec_ptr.cpu().numpy()
    return (csr.indptr.cpu().numpy().astype(np.int64), compact.decode(csr).cpu().numpy(),
            compact.decode_weights(csr).cpu().numpy(), rec_ptr)


def _assert_same_arrays(got, want, what):
    """Two builds of one geometry: row pointers, decoded indices, weights and record pointers bit for bit."""
    for a, b, part in zip(got, want, ("indptr", "gate indices", "weights", "rec_ptr")):
        if a is None or b is None:
            assert a is None and b is None, (what, part)
        else:
            assert a.dtype == b.dtype and np.array_equal(a.view(np.int32) if a.dtype == np.float32 else a,
                                                         b.view(np.int32) if b.dtype == np.float32 else b), (what, part)


def _assert_matches_csr(arrays, ref_ip, ref_idx, ref_w, weighting):
    """The bars of test_builder_matches_reference_csr: row pointers and neighbour sets equal, Barnes weights within 1 ulp
    and different in fewer than 1e-3 of the pairs, Cressman and uniform weights bit-equal."""
    ip, idx, w = oracle.canonical_rows(*arrays[:3])
    r_ip, r_idx, r_w = oracle.canonical_rows(ref_ip, ref_idx, ref_w)
    np.testing.assert_array_equal(ip, r_ip.astype(np.int64))
    np.testing.assert_array_equal(idx, r_idx)
    assert w.dtype == np.float32 and r_w.dtype == np.float32
    if weighting == "barnes2":
        ulp = np.abs(w.view(np.int32).astype(np.int64) - r_w.view(np.int32).astype(np.int64))
        assert ulp.max(initial=0) <= 1
        assert (ulp > 0).mean() < 1e-3 if ulp.size else True
    else:
        np.testing.assert_array_equal(w, r_w)


def _same_bits(got, want_np):
    got_np = got.cpu().numpy() if hasattr(got, "cpu") else got
    assert got_np.shape == want_np.shape
    np.testing.assert_array_equal(np.isnan(got_np), np.isnan(want_np))
    live = ~np.isnan(want_np)
    return np.array_equal(got_np.view(np.int32)[live], want_np.view(np.int32)[live])


# ---- 1. the kernels' slab arguments on a hand-made compact copy --------------------------------------------------------------
class _SlabCase:
    """The hand-made geometry of slab_scenes.make_slab_case on the device, with int64 row pointers, and its records packed
    slab by slab (kept per partition and record order)."""

    def __init__(self):
        import torch
        from radar_processor_amd.grid_geometry import DeviceCSR
        self.torch = torch
        self.c = c = scenes.make_slab_case()
        self.dev = torch.device("cuda", torch.cuda.current_device())
        self.shape = c["shape"]
        self.n_vox = int(np.prod(self.shape))
        self.indptr = self.up(c["indptr"])
        self.local = self.up(c["pos"].astype(np.uint16).view(np.int16))
        self.wts, self.gidx = self.up(c["wts"]), self.up(c["gidx"])
        self.dict_ptr, self.dict = self.up(c["dict_ptr"]), self.up(c["dict"])
        self.csr = DeviceCSR(self.indptr, self.gidx, self.wts, int(c["gidx"].max()))
        assert self.csr.is_i64
        self.fields = [self.up(f) for f in c["fields"]]
        self.masks = [None if m is None else self.up(m.astype(np.uint8)) for m in c["masks"]]
        self._packed, self._want = {}, {}

    def up(self, a):
        return self.torch.from_numpy(np.ascontiguousarray(a)).to(self.dev)

    def slab_copy(self, src, p0, p1):
        """A buffer that holds exactly the slab's elements, as the builder's scratch buffers do (never empty)."""
        buf = self.torch.empty(max(p1 - p0, 1), dtype=src.dtype, device=self.dev)
        buf[:p1 - p0].copy_(src[p0:p1])
        return buf

    def want(self, order):
        """The NumPy encoder's stream and rec_ptr for the WHOLE grid."""
        if order not in self._want:
            slot_of, n_slots = scenes.slot_table(self.shape, order)
            self._want[order] = scenes.encode_records(self.c, self.shape, slot_of, n_slots) + (n_slots,)
        return self._want[order]

    def pack(self, parts, order):
        """``rg_csr_compact_pack_dense`` once per slab of ``parts`` -> (records, rec_ptr, error flag) on the device."""
        key = (tuple(parts), order)
        if key in self._packed:
            return self._packed[key]
        from radar_processor_amd import _native
        from radar_processor_amd.grid_geometry import CompactCSR
        torch, c = self.torch, self.c
        lib = _native.load_library()
        nz, ny, nx = self.shape
        n_xy = ny * nx
        nsx, nyg, _ = scenes.layout(self.shape)
        stream, want_ptr, n_slots = self.want(order)
        slots_per_plane, level_ptr = n_slots // nz, c["indptr"][::n_xy]
        # the slabs' record pointers laid end to end, exactly as the builder splices them
        rec_ptr = torch.zeros(n_slots + 1, dtype=torch.int64, device=self.dev)
        slab_dict_ptr, n_units = [], 0
        for (iz0, iz1) in parts:
            c0, c1 = iz0 * nyg * nsx, iz1 * nyg * nsx
            dp = (self.dict_ptr[c0:c1 + 1] - self.dict_ptr[c0]).contiguous()      # the slab's own dict_ptr: starts at 0
            ip = self.indptr[iz0 * n_xy:iz1 * n_xy + 1]                           # a view: absolute pair positions
            assert iz0 == 0 or int(ip[0]) != 0
            rp = CompactCSR.record_pointers(ip, (iz1 - iz0, ny, nx), order, dp, plane0=iz0)
            s0 = iz0 * slots_per_plane
            assert rp.numel() == (iz1 - iz0) * slots_per_plane + 1
            rec_ptr[s0 + 1:s0 + rp.numel()] = rp[1:] + n_units
            n_units += int(rp[-1])
            slab_dict_ptr.append(dp)
        # checked BEFORE any launch: the pack kernel writes where rec_ptr points
        np.testing.assert_array_equal(rec_ptr.cpu().numpy(), want_ptr)
        rec = torch.full((int(want_ptr[-1]), 4), 0x5A5A5A5A, dtype=torch.int32, device=self.dev)   # every byte must be written
        err = torch.zeros(1, dtype=torch.int32, device=self.dev)
        with torch.cuda.device(self.dev):
            for (iz0, iz1), dp in zip(parts, slab_dict_ptr):
                p0, p1 = int(level_ptr[iz0]), int(level_ptr[iz1])
                l_slab, w_slab = self.slab_copy(self.local, p0, p1), self.slab_copy(self.wts, p0, p1)
                _native.check(lib.rg_csr_compact_pack_dense(
                    _native.ptr(self.indptr) + 8 * iz0 * n_xy, 1, _native.ptr(l_slab) - 2 * p0, _native.ptr(w_slab) - 4 * p0,
                    (iz1 - iz0) * n_xy, nx, ny, _native.ptr(dp), _native.ptr(rec_ptr) + 8 * iz0 * slots_per_plane, order, iz0,
                    scenes.W_BASE, _native.ptr(rec), _native.ptr(err), _native.stream_ptr()), "rg_csr_compact_pack_dense")
                torch.cuda.synchronize(self.dev)                                  # the slab's buffers die here
        self._packed[key] = (rec, rec_ptr, int(err.item()))
        return self._packed[key]

    def compact(self, rec, rec_ptr, order):
        from radar_processor_amd.grid_geometry import CompactCSR
        c = self.c
        k = CompactCSR(self.local, self.dict_ptr, self.dict, int(c["sizes"].max()), 4096, self.shape,
                       self.up(c["chunk_pairs"]), self.up(c["sizes"]))
        k.rec, k.rec_ptr, k.rec_order, k.w_base, k._pack_tried = rec, rec_ptr, order, scenes.W_BASE, True
        return k

    def run(self, compact, nf, tile=0):
        """One pass of ``nf`` fields: through ``compact``'s records (row-wise kernel, or the tile kernel for ``tile`` = 384),
        or through ``rg_csr_apply_f32`` without a compact copy."""
        from radar_processor_amd.grid_geometry import GridGeometry
        from radar_processor_amd.gridding import CsrGridder
        geom = GridGeometry.from_device(self.shape, ((0.0, 1.0),) * 3, self.csr, TOA, compact=compact)
        gr = CsrGridder(geom, self.c["n_gates"], nf, device=self.dev)             # compact=False: the standard kernel
        if compact is not None:
            gr.compact, gr.packed_stream, gr.tile = compact, True, tile
            gr.window = compact.window_for(nf, rowwise=tile != 384)
        gr.pack(self.fields[:nf], self.masks[:nf])
        out = self.torch.full((nf, self.n_vox), 9.0, dtype=self.torch.float32, device=self.dev)
        gr.apply(out, fill_value=-3.0)
        return out


@pytest.fixture(scope="module")
def slab_case(rg):
    return _SlabCase()


@pytest.mark.parametrize("order", [scenes.ORDER_DISPATCH, scenes.ORDER_SEGMENT], ids=["dispatch", "segment"])
@pytest.mark.parametrize("parts", scenes.SLAB_PARTITIONS, ids=["each_plane", "01_2_34", "one_slab"])
def test_pack_kernel_slab_by_slab_writes_the_whole_grid_s_stream(rg, slab_case, parts, order):
    """``rg_csr_compact_pack_dense`` called once per slab -- int64 row pointers that start at the slab's first (non-zero) pair,
    positions and weights through pointers shifted back by ``2 p0`` / ``4 p0`` bytes, the slab's own ``dict_ptr``,
    ``rec_ptr + first slot``, ``plane0`` -- fills the bytes of the NumPy encoder's stream for the whole grid, padding
    included, whatever the partition; ``CompactCSR.record_pointers`` of the slabs, laid end to end, is the encoder's
    ``rec_ptr`` (asserted inside ``pack`` before anything is launched); no error flag."""
    from radar_processor_amd import _native
    assert (scenes.LINES, scenes.ROTATION, scenes.DENSE_MAX) == (_native.RG_COMPACT_LINES, _native.RG_COMPACT_ROTATION,
                                                                _native.RG_DENSE_MAX_DICT)
    nsx, nyg, _ = scenes.layout(slab_case.shape)
    assert {scenes.rotation_of_group(p * nyg, nsx) for p in range(slab_case.shape[0])} == set(range(nsx))
    rec, rec_ptr, flag = slab_case.pack(parts, order)
    stream, want_ptr, _ = slab_case.want(order)
    print(f"slab pack: {len(parts)} slabs {parts}, order {order}, {int(want_ptr[-1])} units")
    assert flag == 0
    got = rec.cpu().numpy().view(np.uint8).reshape(-1)
    assert got.size == stream.size
    bad = np.nonzero(got != stream)[0]
    assert bad.size == 0, f"first differing bytes {bad[:8]} of {got.size} ({len(parts)} slabs, order {order})"


def test_count_and_fill_kernels_slab_by_slab(rg, slab_case):
    """``rg_csr_compact_count`` / ``rg_csr_compact_fill`` through ``CompactCSR._planes`` with a view of the row pointers and
    gate-index / position addresses shifted back by the slab's first pair: every chunk's dictionary is, as a set, the distinct
    gates of its pairs (np.unique), the sizes are those of the one-call build, and ``dict[dict_ptr[chunk] + position]`` gives
    back every pair's gate index."""
    import torch
    from radar_processor_amd import _native
    from radar_processor_amd.grid_geometry import CompactCSR
    case, c = slab_case, slab_case.c
    nz, ny, nx = case.shape
    n_xy, level_ptr = ny * nx, c["indptr"][::ny * nx]
    nsx, nyg, n_chunks = scenes.layout(case.shape)
    stride = c["n_gates"]
    want_keys = np.unique(c["chunk_of_pair"] * stride + c["gidx"])                 # (chunk, gate), sorted
    with torch.cuda.device(case.dev):
        one_local = torch.zeros(c["n_pairs"], dtype=torch.int16, device=case.dev)
        one_counts, _ = CompactCSR._planes(case.indptr, _native.ptr(case.gidx), nz, ny, nx, _native.ptr(one_local))
        one_counts = one_counts.cpu().numpy()
        assert np.array_equal(one_counts, np.bincount(want_keys // stride, minlength=n_chunks))
        for parts in scenes.SLAB_PARTITIONS:
            counts, dicts, local = [], [], np.zeros(c["n_pairs"], dtype=np.int64)
            for (iz0, iz1) in parts:
                p0, p1 = int(level_ptr[iz0]), int(level_ptr[iz1])
                g_slab = case.slab_copy(case.gidx, p0, p1)
                l_slab = torch.zeros(max(p1 - p0, 1), dtype=torch.int16, device=case.dev)
                built = CompactCSR._planes(case.indptr[iz0 * n_xy:iz1 * n_xy + 1], _native.ptr(g_slab) - 4 * p0, iz1 - iz0, ny, nx,
                                           _native.ptr(l_slab) - 2 * p0)
                assert built is not None and built[0].numel() == (iz1 - iz0) * nyg * nsx
                counts.append(built[0].cpu().numpy())
                dicts.append(built[1].cpu().numpy())
                local[p0:p1] = l_slab[:p1 - p0].cpu().numpy().view(np.uint16)
            counts, dict_ = np.concatenate(counts), np.concatenate(dicts)
            assert np.array_equal(counts, one_counts), parts
            dict_ptr = np.concatenate([[0], np.cumsum(counts)])
            chunk_of_entry = np.repeat(np.arange(n_chunks), counts)
            assert np.array_equal(np.sort(chunk_of_entry * stride + dict_), want_keys), parts
            assert (local < counts[c["chunk_of_pair"]]).all(), parts
            assert np.array_equal(dict_[dict_ptr[c["chunk_of_pair"]] + local], c["gidx"]), parts


def test_apply_kernels_over_the_slab_packed_records(rg, slab_case):
    """The row-wise kernel (1, 3, 8 fields) over records packed plane by plane == ``oracle.csr_apply_rowwise_order`` bit for bit,
    and the tile kernel (tile = 384; 1 and 4 fields) over records packed as ``[0,1][2][3,4]`` == ``rg_csr_apply_f32`` bit for
    bit -- both with int64 row pointers, as on the one-call records (test_gpu_dense_records.py)."""
    case, c, t = slab_case, slab_case.c, slab_case.torch
    order = scenes.ORDER_DISPATCH
    rec, rec_ptr, flag = case.pack(scenes.SLAB_PARTITIONS[0], order)
    assert flag == 0
    by_plane = case.compact(rec, rec_ptr, order)
    for nf in (1, 3, 8):
        want = oracle.csr_apply_rowwise_order(c["indptr"], c["gidx"], c["wts"], c["fields"][:nf], c["masks"][:nf], case.shape,
                                              fill_value=-3.0).reshape(nf, case.n_vox)
        assert _same_bits(case.run(by_plane, nf), want), nf
    rec, rec_ptr, flag = case.pack(scenes.SLAB_PARTITIONS[1], order)
    assert flag == 0
    by_runs = case.compact(rec, rec_ptr, order)
    for nf in (1, 4):
        got, want = case.run(by_runs, nf, tile=384), case.run(None, nf)
        assert t.equal(got.view(t.int32), want.view(t.int32)), nf


# ---- 2. the slab builder on the reference's own geometries -------------------------------------------------------------------
SEAM_FIXTURES = golden_names("g3_") + golden_names("g4_") + golden_names("g6_")


@pytest.mark.parametrize("packed", [False, True], ids=["compact", "packed"])
@pytest.mark.parametrize("name", SEAM_FIXTURES)
def test_slab_builder_matches_the_reference_csr_at_every_seam(rg, name, packed):
    """Every partition of a fixture's levels into slabs gives the reference's CSR (canonical rows; the weight bars of
    test_builder_matches_reference_csr), and all partitions agree with each other bit for bit.  ``pairs_per_slab`` comes from
    the fixture's own per-level pair counts L: 1 (a slab per level with pairs, runs of pair-less levels as slabs of their
    own), ``L[i] + L[i+1]`` for the interior level ``slab_scenes.seam_level`` finds and the same minus 1 (the ``<=`` of the
    rule from both sides), a third of the pairs, and more than all of them.  The slabs of every build are asserted against
    ``slab_scenes.slabs_for``.  Cressman weights have no packed layout: ``packed=True`` must return ``None``.  The corner
    window has no pairs and therefore never a second slab: it builds and grids to all-fill."""
    meta, ref = load_golden(name)
    vol = volume_for(meta)
    shape, limits = grid_spec(meta)
    kw = builder_kwargs(meta)
    weighting = kw.pop("weighting")
    search = rg.RoiSearch(vol.gate_x, vol.gate_y, vol.gate_z, shape, limits, **kw)
    level_pairs = np.diff(ref["indptr"][::shape[1] * shape[2]].astype(np.int64))
    total = int(level_pairs.sum())
    if total == 0:
        assert name == "g3_c2_corner_barnes2"
        for cap in (1, 10):
            geom, slabs = _build(search, weighting, limits, cap, packed)
            assert geom is not None and slabs == [(0, shape[0])] and geom.n_pairs() == 0
            got = rg.apply_geometry(geom, rg.get_field_data(vol.as_radar(), meta["fields"][0]), fill_value=-7.0)
            assert got.shape == shape and (got == np.float32(-7.0)).all()
        return
    i = scenes.seam_level(level_pairs)
    assert i is not None
    seam = int(level_pairs[i] + level_pairs[i + 1])
    caps = [1, seam, seam - 1, max(total // 3, 1), total + 1]
    first, counts = None, {}
    for cap in caps:
        want_slabs = scenes.slabs_for(level_pairs, cap)
        geom, slabs = _build(search, weighting, limits, cap, packed)
        if packed and weighting == "cressman":                    # refused before the first slab
            assert geom is None and slabs == [], (name, cap)
            continue
        assert slabs == want_slabs, (name, cap)
        counts[cap] = len(slabs)
        assert geom is not None, (name, cap)
        csr, compact = geom.device_csr(), geom.device_compact()
        assert csr.gate_indices is None and (csr.weights is None) == packed and (compact.rec is not None) == packed
        arrays = _arrays(geom)
        if first is None:
            first = arrays
            _assert_matches_csr(arrays, ref["indptr"], reference_indices(name, meta, ref), ref["weights"], weighting)
        else:
            _assert_same_arrays(arrays, first, (name, cap))
    print(f"{name} {'packed' if packed else 'compact'}: slabs per pairs_per_slab {counts} (seam level {i})")
    if not counts:
        return
    # the seams fell where they were aimed: a second slab everywhere but above the total, a slab per level with pairs ...
    assert counts[1] >= int((level_pairs > 0).sum()) >= 2 and counts[total + 1] == 1 and counts[max(total // 3, 1)] >= 3
    # ... and at L[i] + L[i+1] a slab is exactly full, which one pair less cuts differently
    at, below = scenes.slabs_for(level_pairs, seam), scenes.slabs_for(level_pairs, seam - 1)
    assert any(int(level_pairs[a:b].sum()) == seam for a, b in at) and at != below


# ---- 3. the wide scene ---------------------------------------------------------------------------------------------------
N_WIDE_FIELDS = 11


class _Wide:
    """The wide scene on the device: searches, slab-built geometries (kept per weighting, slab size, layout and gate-list
    kind), eleven fields with per-field masks and a shared mask."""

    def __init__(self, rg):
        import torch
        self.rg, self.torch = rg, torch
        self.scene = w = scenes.wide_scene()
        self.vol = w["vol"]
        self.dev = torch.device("cuda", torch.cuda.current_device())
        self.n_gates = self.vol.n_total_gates
        rng = np.random.default_rng(11)
        self.fields = [rng.normal(5.0 * k, 20.0, self.n_gates).astype(np.float32) for k in range(N_WIDE_FIELDS)]
        self.masks = [(rng.random(self.n_gates) < 0.15) if k % 3 else None for k in range(N_WIDE_FIELDS)]
        self.shared = rng.random(self.n_gates) < 0.1
        up = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(self.dev)       # noqa: E731
        self.f_t = [up(f) for f in self.fields]
        self.m_t = [None if m is None else up(m.astype(np.uint8)) for m in self.masks]
        self.shared_t = up(self.shared.astype(np.uint8))
        self.excluded = [self.shared if m is None else (m | self.shared) for m in self.masks]
        self._searches, self._geoms, self._csr_geoms = {}, {}, {}

    def search(self, per_level=None, window=None):
        if (per_level, window) not in self._searches:
            v = self.vol
            self._searches[per_level, window] = self.rg.RoiSearch(v.gate_x, v.gate_y, v.gate_z, scenes.WIDE_SHAPE,
                                                                  scenes.WIDE_LIMITS, per_level=per_level, window=window,
                                                                  **scenes.WIDE_KW)
        return self._searches[per_level, window]

    def build(self, weighting, cap, packed, per_level=None):
        """The slab-built geometry; its slabs are asserted on every build."""
        key = (weighting, cap, packed, per_level)
        if key not in self._geoms:
            geom, slabs = _build(self.search(per_level), weighting, scenes.WIDE_LIMITS, cap, packed)
            print(f"wide scene {weighting} pairs_per_slab={cap} packed={packed} per_level={per_level}: {len(slabs)} slabs {slabs}")
            assert slabs == ([] if geom is None else scenes.WIDE_SLABS[cap]), key
            assert (geom is None) == (packed and weighting == "cressman"), key
            self._geoms[key] = geom
        return self._geoms[key]

    def csr_geometry(self, weighting, tmp):
        """The standard ``layout="csr"`` build, its compact copy built first."""
        if weighting not in self._csr_geoms:
            v = self.vol
            g = self.rg.compute_grid_geometry(v.gate_x, v.gate_y, v.gate_z, scenes.WIDE_SHAPE, scenes.WIDE_LIMITS, str(tmp),
                                              weighting=weighting, layout="csr", **scenes.WIDE_KW)
            assert g.device_compact() is not None
            self._csr_geoms[weighting] = g
        return self._csr_geoms[weighting]

    def grid(self, geom, nf):
        return self.rg.grid_fields_device(geom, self.f_t[:nf], self.m_t[:nf], shared_mask=self.shared_t).cpu().numpy()


@pytest.fixture(scope="module")
def wide(rg):
    return _Wide(rg)


def _dense_wide_empty(sizes):
    return int(((sizes <= scenes.DENSE_MAX) & (sizes > 0)).sum()), int((sizes > scenes.DENSE_MAX).sum()), int((sizes == 0).sum())


def _assert_record_bytes(compact, arrays, shape, sizes, n_gates, what):
    """The records of a packed build, byte for byte, against the NumPy encoder: every pair's position is looked up in the
    build's own dictionaries (their order is the build's business), the decoded weights are coded, and the stream is laid
    out in the dispatch order of the whole grid."""
    ip, idx, wts, got_ptr = arrays
    dict_, dict_ptr = compact.dict.cpu().numpy(), compact.dict_ptr.cpu().numpy()
    chunk_of_pair = np.repeat(scenes.chunk_of_rows(shape), np.diff(ip))
    entry_keys = np.repeat(np.arange(sizes.size), sizes) * n_gates + dict_
    by_key = np.argsort(entry_keys)
    entry = by_key[np.searchsorted(entry_keys[by_key], chunk_of_pair * n_gates + idx)]
    assert np.array_equal(dict_[entry], idx), what
    case = dict(indptr=ip, pos=entry - dict_ptr[chunk_of_pair], wts=wts, sizes=sizes)
    slot_of, n_slots = scenes.slot_table(shape, scenes.ORDER_DISPATCH)
    stream, rec_ptr = scenes.encode_records(case, shape, slot_of, n_slots)
    assert np.array_equal(got_ptr, rec_ptr), what
    got = compact.rec.cpu().numpy().view(np.uint8).reshape(-1)
    assert got.size == stream.size and np.array_equal(got, stream), what


@pytest.mark.parametrize("packed", [False, True], ids=["compact", "packed"])
@pytest.mark.parametrize("weighting", scenes.WEIGHTINGS)
def test_wide_scene_slab_builds_match_the_oracle(rg, wide, weighting, packed):
    """``pairs_per_slab`` of 1, 6327, 6328 and 10**12 cut the six levels into 6, 3, 3 and 1 slabs (asserted per build, with
    per-level gate lists and, for the first and third, with one gate list for all levels).  Every build: neighbour sets
    bit-exact against the oracle, weights within the reference bars, chunk sizes and coding the oracle's, ``rec_ptr`` that of
    ``CompactCSR.record_pointers`` on the whole grid and as long as the records; the record bytes are those of the NumPy
    encoder fed with the decoded arrays and the build's dictionaries; all builds from one search agree bit for bit (the
    order of a row's pairs follows the search's cell size, which differs between the two kinds of gate list)."""
    from radar_processor_amd.grid_geometry import CompactCSR
    w = wide.scene
    sizes = w["chunk_sizes"]
    print("wide scene chunks: %d dense / %d wide / %d empty" % _dense_wide_empty(sizes))
    assert _dense_wide_empty(sizes) == (34, 2, 18)
    first = {}
    for cap, per_level in [(c, None) for c in scenes.WIDE_SLABS] + [(1, False), (6328, False)]:
        geom = wide.build(weighting, cap, packed, per_level)
        assert wide.search(per_level).per_level == (per_level is None)
        if packed and weighting == "cressman":
            assert geom is None
            continue
        csr, compact = geom.device_csr(), geom.device_compact()
        assert csr.gate_indices is None and (csr.weights is None) == packed and csr.n_pairs == int(w["indptr"][-1])
        arrays = _arrays(geom)
        if per_level not in first:                           # in-row order is (cell row, gate): it follows the search's cells
            first[per_level] = arrays
            _assert_matches_csr(arrays, w["indptr"], w["idx"], w["w32"][weighting], weighting)
        else:
            _assert_same_arrays(arrays, first[per_level], (weighting, cap, per_level))
        assert np.array_equal(compact.chunk_counts.cpu().numpy(), sizes)
        assert np.array_equal(np.diff(compact.dict_ptr.cpu().numpy()), sizes)
        assert np.array_equal(compact.dense_chunks().cpu().numpy(), sizes <= scenes.DENSE_MAX)
        assert np.array_equal(compact.chunk_pairs.cpu().numpy(), w["chunk_pairs"])
        if not packed:
            assert compact.local_idx is not None
            continue
        assert compact.local_idx is None and compact.rec_order == scenes.ORDER_DISPATCH and compact.w_base == scenes.W_BASE
        whole = CompactCSR.record_pointers(csr.indptr, scenes.WIDE_SHAPE, compact.rec_order, compact.dict_ptr)
        assert np.array_equal(arrays[3], whole.cpu().numpy()) and compact.rec.shape == (int(arrays[3][-1]), 4)
        _assert_record_bytes(compact, arrays, scenes.WIDE_SHAPE, sizes, wide.n_gates, (weighting, cap, per_level))


@pytest.mark.parametrize("weighting", ["barnes2", "nearest"])
def test_windowed_wide_scene_rotates_every_slab_differently(rg, wide, weighting):
    """Three line groups times three segments rotate every level of the wide scene alike, so ``plane0`` cannot show in its
    records.  Its first eight lines (``RoiSearch(window=...)``) have two line groups: built packed with a slab per level, the
    slabs at levels 1 and 2 lie one and two columns further round than grids of their own would.  Against the oracle's rows of
    the window: neighbour sets, weights, chunk sizes, and the record bytes in the whole grid's dispatch order; one slab gives
    the same bits."""
    win = scenes.wide_window_scene()
    search = wide.search(window=scenes.WIDE_WINDOW)
    assert search.grid_shape == scenes.WINDOW_SHAPE
    first = None
    for cap in (1, 10 ** 12):
        geom, slabs = _build(search, weighting, scenes.WIDE_LIMITS, cap, True)
        print(f"windowed wide scene {weighting} pairs_per_slab={cap}: {len(slabs)} slabs {slabs}")
        assert geom is not None and slabs == scenes.slabs_for(win["level_pairs"], cap) and len(slabs) == (6 if cap == 1 else 1)
        compact = geom.device_compact()
        arrays = _arrays(geom)
        if first is None:
            first = arrays
            _assert_matches_csr(arrays, win["indptr"], win["idx"], win["w32"][weighting], weighting)
        else:
            _assert_same_arrays(arrays, first, (weighting, cap))
        assert np.array_equal(compact.chunk_counts.cpu().numpy(), win["chunk_sizes"])
        _assert_record_bytes(compact, arrays, scenes.WINDOW_SHAPE, win["chunk_sizes"], wide.n_gates, (weighting, cap))


@pytest.mark.parametrize("weighting", scenes.WEIGHTINGS)
def test_gridding_through_every_slab_built_geometry(rg, wide, weighting, tmp_path):
    """``grid_fields_device`` for 1, 3, 5, 8 and 11 fields (per-field masks and a shared mask) through every slab-built
    geometry -- ``_use_compact``, ``_fields_per_pass`` and ``CsrGridder`` on a geometry without ``gate_indices`` / ``weights``:

     * every voxel within ``oracle.mean_error_bound`` of its float64 mean (the oracle's exact weights, DELTA_CSR), same fill;
     * bit for bit the documented result.  Barnes / uniform: 68 % of this scene's pairs lie in its two wide chunks, so the
       ``layout="csr"`` geometry turns its compact copy down (more than 2 % of the pairs past any LDS window) and runs
       ``rg_csr_apply_f32``, while a geometry that has nothing but its compact copy runs the row-wise kernel: the two differ
       by kernel, not by slab.  The reference is therefore ``oracle.csr_apply_rowwise_order`` on the decoded arrays, in the
       passes ``fields_per_pass`` cuts (whatever it chooses; the arrays are held against the oracle, as sets per row, in
       test_wide_scene_slab_builds_match_the_oracle -- the in-row order is the build's own).  Cressman: the
       tile kernel, which has the bits of ``rg_csr_apply_f32``: the same call on the ``layout="csr"`` build."""
    from radar_processor_amd.gridding import fields_per_pass
    w = wide.scene
    counts = (1, 3, 5, 8, 11)
    stats = [oracle.voxel_stats(w["indptr"], w["idx"], w["w64"][weighting], wide.fields[k], wide.excluded[k])
             for k in range(N_WIDE_FIELDS)]
    builds = [(cap, packed) for cap in scenes.WIDE_SLABS for packed in ((False,) if weighting == "cressman" else (False, True))]
    decoded, emu, bounded = None, {}, set()

    def want(nf, per_pass):
        """The documented bits of an ``nf``-field call that fuses ``per_pass`` fields per pass (a pass's add order depends on
        its field count, so the oracle is run pass by pass; each pass once)."""
        if weighting == "cressman":                      # per field the same bits whatever the pass
            if nf not in emu:
                emu[nf] = wide.grid(wide.csr_geometry(weighting, tmp_path), nf)
            return emu[nf]
        parts = []
        for f0 in range(0, nf, per_pass):
            f1 = min(nf, f0 + per_pass)
            if (f0, f1) not in emu:
                emu[f0, f1] = oracle.csr_apply_rowwise_order(*decoded[:3], wide.fields[f0:f1], wide.excluded[f0:f1],
                                                             scenes.WIDE_SHAPE)
            parts.append(emu[f0, f1])
        return np.concatenate(parts)

    for cap, packed in builds:
        geom = wide.build(weighting, cap, packed)
        per_pass = fields_per_pass(geom)                 # the policy's choice (4 or 8 today); the reference follows it
        assert 1 <= per_pass <= 8
        if decoded is None:
            decoded = _arrays(geom)
        else:                                            # one reference serves every build: they decode to the same arrays
            _assert_same_arrays(_arrays(geom)[:3], decoded[:3], (weighting, cap, packed))
        for nf in counts:
            got = wide.grid(geom, nf)
            assert got.shape == (nf,) + scenes.WIDE_SHAPE
            ref = want(nf, per_pass)
            assert _same_bits(got, ref), (weighting, cap, packed, nf)
            # The bound is evaluated once per distinct reference result and holds for every build by transitivity: each
            # build's grid was just asserted bit-equal to ``ref`` (NaN pattern included), so a grid inside the bound puts
            # all of them inside it.
            if (nf, per_pass) not in bounded:
                bounded.add((nf, per_pass))
                for k in range(nf):
                    ratio = oracle.bound_ratio(got[k], stats[k], oracle.DELTA_CSR[weighting])
                    assert ratio.max(initial=0.0) <= 1.0, (weighting, packed, nf, k, float(ratio.max()))
    assert {nf for nf, _ in bounded} == set(counts)


def test_products_of_the_packed_only_geometry(rg, wide, monkeypatch):
    """``grid_products_device(fused=True)`` on the packed-only geometry (planes mode: colmin, colmean, colmax / argmax and
    CAPPIs at a level, between two levels and above the grid) returns the bits of the separate K3 / K4 kernels applied to the
    stored grid; the column minimum and maximum are also NumPy's over the grid ``grid_fields_device`` returns.  The launches
    are counted: the fused call is ONE planes-mode launch and stores no grid, the separate call is one ``apply``."""
    from radar_processor_amd.gridding import CsrGridder
    t = wide.torch
    geom = wide.build("barnes2", 6328, True)
    products = rg.PlaneProducts(colmin=True, colmean=True, cappi=(1500.0, 2000.0, 9000.0), fused=True)
    nf = 3
    calls = []
    for method in ("apply", "apply_planes", "apply_columns"):
        def spy(self, *a, _orig=getattr(CsrGridder, method), _name=method, **kw):
            calls.append(_name)
            return _orig(self, *a, **kw)
        monkeypatch.setattr(CsrGridder, method, spy)
    fused = rg.grid_products_device(geom, wide.f_t[:nf], wide.m_t[:nf], shared_mask=wide.shared_t, products=products)
    assert calls == ["apply_planes"], calls
    plain = rg.grid_products_device(geom, wide.f_t[:nf], wide.m_t[:nf], shared_mask=wide.shared_t, products=products,
                                    fused=False)
    assert calls == ["apply_planes", "apply"], calls
    grid = wide.grid(geom, nf)
    assert len(fused) == len(plain) == nf
    for k in range(nf):
        assert sorted(fused[k]) == sorted(plain[k]) == ["argmax", "cappi", "colmax", "colmean", "colmin"]
        for key in ("colmax", "colmin", "colmean"):
            assert t.equal(fused[k][key].view(t.int32), plain[k][key].view(t.int32)), (k, key)
        assert t.equal(fused[k]["argmax"], plain[k]["argmax"]), k
        for alt in products.cappi:
            assert t.equal(fused[k]["cappi"][alt].view(t.int32), plain[k]["cappi"][alt].view(t.int32)), (k, alt)
        assert np.array_equal(fused[k]["colmin"].cpu().numpy(), np.fmin.reduce(grid[k], axis=0), equal_nan=True)
        assert np.array_equal(fused[k]["colmax"].cpu().numpy(), np.fmax.reduce(grid[k], axis=0), equal_nan=True)
        assert np.array_equal(fused[k]["cappi"][1500.0].cpu().numpy(), grid[k][1], equal_nan=True)
        assert np.isnan(fused[k]["cappi"][9000.0].cpu().numpy()).all()


def test_decoding_across_level_seams(rg, wide):
    """``CompactCSR.decode`` / ``decode_weights`` of the geometry built with a slab per level, from its records alone: 1, 7, 149
    and 10**6 rows per decoding step, over row ranges that start and end inside a segment, span the seam between two levels,
    cover the pair-less level up to the end of the grid, and lie inside it -- each the matching slice of the whole grid's
    arrays (which test_wide_scene_slab_builds_match_the_oracle holds against the oracle); the whole grid in steps of 149 and
    10**6 rows."""
    geom = wide.build("barnes2", 1, True)
    csr, compact = geom.device_csr(), geom.device_compact()
    assert csr.weights is None and compact.local_idx is None
    ip, idx, wts, _ = _arrays(geom)
    n_xy = scenes.WIDE_SHAPE[1] * scenes.WIDE_SHAPE[2]
    starts = scenes.segment_starts(scenes.WIDE_SHAPE[2])
    assert starts == [0, 50, 100, 150]
    ranges = [(17, 133), (n_xy - 40, n_xy + 260), (4 * n_xy + 700, 6 * n_xy), (5 * n_xy + 10, 5 * n_xy + 90)]
    assert ip[133] > ip[17] and ip[n_xy] > ip[n_xy - 40] and ip[n_xy + 260] > ip[n_xy]
    assert ip[5 * n_xy] > ip[4 * n_xy + 700] and ip[6 * n_xy] == ip[5 * n_xy]
    for rows_per_slab in (1, 7, 149, 10 ** 6):
        for (r0, r1) in ranges + ([(0, 6 * n_xy)] if rows_per_slab >= 149 else []):
            got = compact.decode(csr, r0, r1, rows_per_slab=rows_per_slab).cpu().numpy()
            assert np.array_equal(got, idx[ip[r0]:ip[r1]]), (rows_per_slab, r0, r1)
            got = compact.decode_weights(csr, r0, r1, rows_per_slab=rows_per_slab).cpu().numpy()
            assert np.array_equal(got.view(np.int32), wts[ip[r0]:ip[r1]].view(np.int32)), (rows_per_slab, r0, r1)


def test_interchange_file_of_the_packed_only_geometry(rg, wide, tmp_path):
    """``save_geometry`` of the packed-only geometry (three slabs), then ``load_geometry``: equal (``==``) to the
    ``layout="csr"`` build -- the nine-key file is the interchange contract, whatever the layout in HBM."""
    geom = wide.build("barnes2", 6327, True)
    path = str(tmp_path / "wide.npz")
    rg.save_geometry(geom, path)
    back = rg.load_geometry(path)
    assert back == wide.csr_geometry("barnes2", tmp_path)
    assert back.indptr.dtype == np.int32 and back.n_pairs() == int(wide.scene["indptr"][-1])


def test_layout_policy_on_a_small_grid(rg, wide, tmp_path, monkeypatch):
    """With the large-geometry threshold lowered to 1000 pairs (``pass_policy.LARGE_GEOMETRY_PAIRS``: the packed layout's, and
    with it the one from which ``apply_geometry`` asks for the compact copy): ``layout="auto"`` keeps records only for Barnes
    and uniform weights and the reference's arrays for Cressman; ``layout="packed"`` with Cressman falls to ``"compact"``;
    and ``apply_geometry`` on each equals the ``layout="csr"`` result to rounding (conftest.assert_same_to_rounding)."""
    from radar_processor_amd import pass_policy
    monkeypatch.setattr(pass_policy, "LARGE_GEOMETRY_PAIRS", 1000)
    v = wide.vol
    name = sorted(v.fields)[0]
    radar = v.as_radar()
    fdata = rg.get_field_data(radar, name)
    data, mask = oracle.merge_masks(v.fields[name])
    scale = float(np.abs(data[np.isfinite(data) & ~mask]).max())
    n_pairs = int(wide.scene["indptr"][-1])

    def make(weighting, layout):
        return rg.compute_grid_geometry(v.gate_x, v.gate_y, v.gate_z, scenes.WIDE_SHAPE, scenes.WIDE_LIMITS, str(tmp_path),
                                        weighting=weighting, layout=layout, **scenes.WIDE_KW)
    for weighting in scenes.WEIGHTINGS:
        want = rg.apply_geometry(make(weighting, "csr"), fdata)
        assert np.isfinite(want).any() and np.isnan(want).any()
        if weighting == "cressman":
            # "auto" keeps the reference's arrays only while they and their compact copy fit: 10.4 bytes per pair + 10 GiB free
            free_b, _ = wide.torch.cuda.mem_get_info(wide.dev)
            assert free_b >= 10.4 * n_pairs + (10 << 30), (f"{free_b / 2 ** 30:.1f} GiB free on the device: below 10 GiB "
                                                            "layout='auto' builds 'compact' for Cressman, which is not "
                                                            "what this test is about")
        auto = make(weighting, "auto")
        csr = auto.device_csr()
        if weighting == "cressman":
            assert csr.gate_indices is not None and csr.weights is not None
        else:
            compact = auto.device_compact()
            assert csr.gate_indices is None and csr.weights is None and compact.local_idx is None and compact.rec is not None
        assert_same_to_rounding(rg.apply_geometry(auto, fdata), want, scale)
        if weighting == "cressman":
            fell = make(weighting, "packed")
            csr, compact = fell.device_csr(), fell.device_compact()
            assert csr.gate_indices is None and csr.weights is not None and compact.rec is None and compact.local_idx is not None
            assert_same_to_rounding(rg.apply_geometry(fell, fdata), want, scale)
