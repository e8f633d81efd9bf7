"""The prologue kernels every gridding path starts with, pinned to the contracts of include/radargrid_hip.h through the C
ABI: ``rg_pack_fields_f32`` (bits of the packed layout, the exclusion sentinel), ``rg_gate_mask_f32`` (strict comparisons at
the thresholds, the ``n % 4`` tail), ``rg_scan_counts_i64`` (int64 totals, an unaligned workspace), ``rg_geom_bin_gates_f32``
and the per-level lists (keep rule, cell key, order, ``cell_start``), and the neighbour sets near the supported limit of
``beam_factor``.  Every contract is discrete -- bits, bytes, integers, orders -- so nothing is compared to a tolerance except
the gridded means of the sentinel scene.  References and inputs: tests/prologue_scenes.py (asserted on the CPU by
tests/test_prologue_scenes.py).  Every output buffer carries a canary on both sides."""
import ctypes

import numpy as np
import pytest

import prologue_scenes as ps
from conftest import assert_same_to_rounding
from oracle import radar_grid_oracle as oracle
from test_gpu_roi_rim import _check_csr

pytestmark = pytest.mark.gpu

CANARY32 = 0x5EEDBEEF
CANARY8 = 0xA5
PAD = 64                      # canary elements on either side of an output (64 floats = 256 bytes: alignment is kept)


@pytest.fixture(scope="module")
def env():
    import torch
    import radar_processor_amd as rg
    from radar_processor_amd import _native
    lib = rg.load_library()
    return dict(torch=torch, rg=rg, native=_native, lib=lib, dev=torch.device("cuda", 0))


def _dev(env, a):
    return env["torch"].from_numpy(np.ascontiguousarray(a)).to(env["dev"])


def _canary(env, n, dtype):
    """A tensor of PAD + n + PAD elements of ``dtype`` filled with the canary, and the pointer of element PAD."""
    torch = env["torch"]
    if dtype == torch.uint8:
        t = torch.full((n + 2 * PAD,), CANARY8, dtype=torch.uint8, device=env["dev"])
    elif dtype == torch.int64:
        t = torch.full((n + 2 * PAD,), CANARY32, dtype=torch.int64, device=env["dev"])
    else:
        t = torch.full((n + 2 * PAD,), CANARY32, dtype=torch.int32, device=env["dev"])
    return t, t.data_ptr() + PAD * t.element_size()


def _split(t, n):
    """host copy of a canary tensor -> (payload[n], True when both canaries are intact)"""
    h = t.cpu().numpy()
    want = CANARY8 if h.dtype == np.uint8 else CANARY32
    return h[PAD:PAD + n], bool((h[:PAD] == want).all() and (h[PAD + n:] == want).all())


def _ptrs(*v):
    return (ctypes.c_void_p * len(v))(*[None if x is None else (x if isinstance(x, int) else x.data_ptr()) for x in v])


# ---- 1. pack -------------------------------------------------------------------------------------------------------------
MASK_BYTES = np.array([1, 2, 0x80, 0xFF], dtype=np.uint8)


def _pack_inputs(n_gates, seed):
    """Eight fields with special_values() scattered over them, eight masks and a shared mask with bytes from {1, 2, 0x80,
    0xFF}: about a third of the gates are masked per field, so specials land on masked and unmasked gates alike."""
    rng = np.random.default_rng(seed)
    sp = np.array(list(ps.special_values().values()), dtype=np.uint32)
    fields, masks = [], []
    for f in range(8):
        v = rng.normal(10.0, 20.0, n_gates).astype(np.float32)
        special = rng.random(n_gates) < (0.5 if n_gates <= 300 else 0.05)
        special[0] = True
        pick = (np.arange(n_gates) * 7 + f * 5 + 11) % sp.size            # gate 0 of field 0: the sentinel itself
        v.view(np.uint32)[special] = sp[pick][special]
        fields.append(v)
        masks.append(np.where(rng.random(n_gates) < 0.3, MASK_BYTES[rng.integers(4, size=n_gates)], 0).astype(np.uint8))
    shared = np.where(rng.random(n_gates) < 0.2, MASK_BYTES[rng.integers(4, size=n_gates)], 0).astype(np.uint8)
    return fields, masks, shared


def _pack(env, fields_t, masks_t, shared_t, n_gates, stride, masks_null=False):
    lib, native, torch = env["lib"], env["native"], env["torch"]
    out, ptr = _canary(env, n_gates * stride, torch.int32)
    nf = len(fields_t)
    rc = lib.rg_pack_fields_f32(nf, _ptrs(*fields_t), None if masks_null else _ptrs(*masks_t),
                                None if shared_t is None else shared_t.data_ptr(), n_gates, stride, ptr, native.stream_ptr())
    assert rc == native.RG_OK, lib.rg_last_error()
    got, intact = _split(out, n_gates * stride)
    assert intact, "rg_pack_fields_f32 wrote outside packed[0 .. n_gates * stride)"
    return got.view(np.uint32).reshape(n_gates, stride)


@pytest.mark.parametrize("n_gates", [1, 255, 256, 257, 70001])
def test_pack_layout_bit_for_bit(env, n_gates):
    """n_fields 1..8 at every allowed stride, masks none / some per field / shared only / both: the packed uint32s are the
    reference's wherever it prescribes bits; a sentinel-valued or signalling-NaN unmasked value is a NaN that is not the
    sentinel; nothing is written outside the buffer."""
    fields, masks, shared = _pack_inputs(n_gates, seed=n_gates)
    f_t = [_dev(env, f) for f in fields]
    m_t = [_dev(env, m) for m in masks]
    s_t = _dev(env, shared)
    n_alias = n_snan = n_runs = n_masked_special = 0
    for nf in range(1, 9):
        for stride in ps.strides_for(nf):
            for mode in ("none", "per_field", "shared", "both"):
                per = mode in ("per_field", "both")
                mk = [masks[f] if per and f % 2 == 0 else None for f in range(nf)]
                mk_t = [m_t[f] if per and f % 2 == 0 else None for f in range(nf)]
                sh, sh_t = (shared, s_t) if mode in ("shared", "both") else (None, None)
                got = _pack(env, f_t[:nf], mk_t, sh_t, n_gates, stride, masks_null=(mode == "none"))
                want = ps.pack_fields_ref(fields[:nf], mk, sh, stride)
                loose = ps.pack_loose_slots(fields[:nf], mk, sh, stride)
                label = f"{nf} fields, stride {stride}, masks {mode}"
                bad = (got != want) & ~loose
                assert not bad.any(), f"{label}: {int(bad.sum())} slots differ, first (gate, slot) {np.argwhere(bad)[:4].tolist()}"
                at = got[loose]
                assert np.isnan(at.view(np.float32)).all() and (at != ps.EXCLUDED_BITS).all(), \
                    f"{label}: a sentinel-valued or signalling unmasked value was packed as {[hex(v) for v in at[:4]]}"
                fb = np.stack([ps.bits(f) for f in fields[:nf]], axis=1)
                n_alias += int((loose[:, :nf] & (fb == ps.EXCLUDED_BITS)).sum())
                n_snan += int((loose[:, :nf] & ps.is_signalling(fb)).sum())
                n_masked_special += int(((want[:, :nf] == ps.EXCLUDED_BITS) & (np.isnan(fb.view(np.float32)) | (fb == 0x80000000))).sum())
                n_runs += 1
    # masks_host == NULL is all-None
    a = _pack(env, f_t[:3], [None] * 3, s_t, n_gates, 4, masks_null=True)
    b = _pack(env, f_t[:3], [None] * 3, s_t, n_gates, 4, masks_null=False)
    assert np.array_equal(a, b)
    print(f"G = {n_gates}: {n_runs} launches, {n_alias} sentinel-valued and {n_snan} signalling-NaN unmasked slots, "
          f"{n_masked_special} masked NaN / -0 slots")
    assert n_runs == 60 and n_alias >= 10 and (n_gates == 1 or (n_snan >= 10 and n_masked_special >= 10))


def test_pack_zero_gates_with_null_buffers(env):
    lib, native = env["lib"], env["native"]
    assert lib.rg_pack_fields_f32(2, _ptrs(None, None), None, None, 0, 2, None, native.stream_ptr()) == native.RG_OK
    assert lib.rg_pack_fields_f32(1, _ptrs(None), _ptrs(None), None, 0, 8, None, native.stream_ptr()) == native.RG_OK


# ---- 2. the sentinel, end to end -----------------------------------------------------------------------------------------
def _sentinel_oracle(weighting="barnes2"):
    s = ps.sentinel_scene()
    ip, idx, w = oracle.build_geometry(s.gx, s.gy, s.gz, s.shape, s.limits, min_radius=s.min_radius,
                                       beam_factor=s.beam_factor, weighting=weighting)
    want = oracle.csr_apply_f64(ip, idx, w, s.a_ref, s.mask, s.shape)
    without = oracle.csr_apply_f64(ip, idx, w, s.a_ref, s.mask | s.hot, s.shape)
    row = np.repeat(np.arange(len(ip) - 1), np.diff(ip))
    touched = np.zeros(len(ip) - 1, dtype=bool)
    touched[row[s.hot[idx]]] = True
    return s, want, without, touched.reshape(s.shape)


def _assert_sentinel(s, got_a, got_ref, got_without, want, without, touched, label):
    """A (sentinel bits on the hot gates) grids to the NaN pattern of the float64 oracle on A' (canonical NaN there) and to
    the bits of A'; with the hot gates masked, to the oracle without them."""
    got_a, got_ref, got_without = (np.asarray(g, dtype=np.float32).reshape(s.shape) for g in (got_a, got_ref, got_without))
    n_touched = int(touched.sum())
    wrong = np.isnan(got_a) != np.isnan(want)
    print(f"{label}: {n_touched} voxels with a sentinel-valued neighbour, {int(wrong.sum())} with another NaN pattern than the oracle")
    assert n_touched >= 50 and np.isnan(want[touched]).all()
    assert not wrong.any(), (f"{label}: {int(wrong.sum())} voxels differ from the oracle's NaN pattern, "
                             f"{int((wrong & touched).sum())} of them next to a sentinel-valued gate")
    assert np.array_equal(got_a.view(np.uint32), got_ref.view(np.uint32)), f"{label}: A and A' grid to different bits"
    scale = float(np.abs(s.a_ref[~(s.mask | s.hot)]).max())
    assert_same_to_rounding(got_without, without, scale)


def test_sentinel_valued_data_through_the_csr_kernels(env, tmp_path):
    """rg_csr_apply_f32, the compact tile kernel, the tile kernel over the records and the packed row-wise kernel (1, 3 and
    8 fields, the field in slots 0, 1 and 5)."""
    from radar_processor_amd.gridding import CsrGridder
    torch, rg, dev = env["torch"], env["rg"], env["dev"]
    s, want, without, touched = _sentinel_oracle()
    geom = rg.compute_grid_geometry(s.gx, s.gy, s.gz, s.shape, s.limits, str(tmp_path), min_radius=s.min_radius,
                                    beam_factor=s.beam_factor)
    t = {k: _dev(env, v) for k, v in dict(a=s.a, a_ref=s.a_ref).items()}
    m_t, m_hot_t = _dev(env, s.mask.astype(np.uint8)), _dev(env, (s.mask | s.hot).astype(np.uint8))
    o_t = [_dev(env, v) for v in s.others]
    om_t = [_dev(env, m.astype(np.uint8)) for m in s.other_masks]
    runs = [("standard", dict(), 1, 0), ("tile", dict(compact=True, packed=False), 1, 0),
            ("records+tile", dict(compact=True, tile=384), 1, 0), ("row-wise", dict(compact=True), 1, 0),
            ("row-wise 3", dict(compact=True), 3, 1), ("row-wise 8", dict(compact=True), 8, 5),
            ("standard 3", dict(), 3, 2), ("tile 3", dict(compact=True, packed=False), 3, 0)]
    for label, kw, nf, slot in runs:
        gr = CsrGridder(geom, s.n, nf, device=dev, **kw)
        assert (gr.compact is not None) == bool(kw) and gr.packed_stream == (label.startswith(("records", "row-wise")))
        outs = {}
        for key, field, mask in (("a", t["a"], m_t), ("a_ref", t["a_ref"], m_t), ("without", t["a"], m_hot_t)):
            fields = o_t[:slot] + [field] + o_t[slot:nf - 1]
            masks = om_t[:slot] + [mask] + om_t[slot:nf - 1]
            gr.pack(fields, masks)
            o = torch.empty((nf, gr.n_vox), dtype=torch.float32, device=dev)
            gr.apply(o)
            outs[key] = o.cpu().numpy()
        assert np.array_equal(outs["a"].view(np.uint32), outs["a_ref"].view(np.uint32)), label
        _assert_sentinel(s, outs["a"][slot], outs["a_ref"][slot], outs["without"][slot], want, without, touched, label)


@pytest.mark.parametrize("weighting", ["barnes2", "cressman", "nearest"])
def test_sentinel_valued_data_through_the_csr_free_paths(env, weighting):
    """rg_roi_grid_f32, rg_roi_section_f32 along one grid row and a one-entry rg_roi_grid_mosaic_f32."""
    from radar_processor_amd import mosaic, section
    rg, dev = env["rg"], env["dev"]
    s, want, without, touched = _sentinel_oracle(weighting)
    roi = dict(min_radius=s.min_radius, beam_factor=s.beam_factor)
    search = rg.RoiSearch(s.gx, s.gy, s.gz, s.shape, s.limits, device=dev, **roi)
    a, a_ref = _dev(env, s.a), _dev(env, s.a_ref)
    m_t, m_hot_t = _dev(env, s.mask.astype(np.uint8)), _dev(env, (s.mask | s.hot).astype(np.uint8))
    other, other_m = _dev(env, s.others[0]), _dev(env, s.other_masks[0].astype(np.uint8))

    def three(run):
        return [run(f, m) for f, m in ((a, m_t), (a_ref, m_t), (a, m_hot_t))]
    got = three(lambda f, m: rg.roi_grid_fields_device(search, [other, f], [other_m, m], weighting=weighting)[1].cpu().numpy())
    _assert_sentinel(s, *got, want, without, touched, f"rg_roi_grid_f32 {weighting}")
    # a section through every column of the grid, row by row: sample (k, iy * nx + ix) is the voxel (k, iy, ix)
    xs = np.tile(np.linspace(s.limits[2][0], s.limits[2][1], s.shape[2], dtype="float32"), s.shape[1])
    ys = np.repeat(np.linspace(s.limits[1][0], s.limits[1][1], s.shape[1], dtype="float32"), s.shape[2])
    got = three(lambda f, m: section.section_fields_device(search, xs, ys, [f], [m], weighting=weighting)[0].cpu().numpy())
    _assert_sentinel(s, *got, want, without, touched, f"rg_roi_section_f32 {weighting}")
    ms = mosaic.MosaicSearch([(s.gx, s.gy, s.gz, (0.0, 0.0, 0.0))], s.shape, s.limits, device=dev, **roi)
    got = three(lambda f, m: mosaic.mosaic_fields_device(ms, [[f]], masks=[[m]], weighting=weighting)[0].cpu().numpy())
    _assert_sentinel(s, *got, want, without, touched, f"rg_roi_grid_mosaic_f32 {weighting}")


def test_sentinel_valued_gate_that_wins_the_closest_gate_mode(env):
    """RG_W_CLOSEST stores the winner's value bit for bit -- except that a winner carrying the sentinel's bits arrives as a
    NaN that is not the sentinel (it was rewritten when the fields were packed)."""
    rg, dev = env["rg"], env["dev"]
    s = ps.sentinel_scene()
    idx = oracle.closest_gate_choice(s.gx, s.gy, s.gz, [s.mask], s.shape, s.limits, s.min_radius, s.beam_factor,
                                     toa=17000.0)["idx32"][0]
    search = rg.RoiSearch(s.gx, s.gy, s.gz, s.shape, s.limits, device=dev, min_radius=s.min_radius, beam_factor=s.beam_factor)
    got = rg.roi_grid_fields_device(search, [_dev(env, s.a)], [_dev(env, s.mask.astype(np.uint8))], weighting="closest",
                                    fill_value=-999.0)[0].cpu().numpy()
    won = (idx >= 0) & s.hot[np.maximum(idx, 0)]
    print(f"closest-gate mode: a sentinel-valued gate wins {int(won.sum())} of {idx.size} voxels")
    assert won.sum() >= 20
    at = got.view(np.uint32)[won]
    assert np.isnan(got[won]).all() and (at != ps.EXCLUDED_BITS).all(), [hex(v) for v in at[:4]]
    want = np.where(idx >= 0, s.a[np.maximum(idx, 0)], np.float32(-999.0)).astype(np.float32)
    assert np.array_equal(got.view(np.uint32)[~won], want.view(np.uint32)[~won])


# ---- 3. gate mask --------------------------------------------------------------------------------------------------------
MASK_SIZES = (1, 2, 3, 4, 5, 1021, 1024, 1027, 100003)


@pytest.mark.parametrize("op", ps.GATE_OPS)
def test_gate_mask_byte_for_byte(env, op):
    """Every case of gate_mask_cases() tiled to sizes around the uchar4 path, from a zero mask and from a mask holding 0, 1,
    2 and 0xFF: the result is ``old | pred`` byte for byte and the bytes after ``n`` are untouched."""
    lib, native, torch = env["lib"], env["native"], env["torch"]
    rng = np.random.default_rng(3)
    n_calls = n_set = n_edge = 0
    for case_op, a, b, data in ps.gate_mask_cases():
        if case_op != op:
            continue
        for n in MASK_SIZES:
            d = ps.tile_to(data, n)
            pred = ps.gate_mask_ref(op, d, a, b)
            d_t = _dev(env, d)
            for prefill in (False, True):
                old = np.array([0, 1, 2, 0xFF], dtype=np.uint8)[rng.integers(4, size=n)] if prefill else np.zeros(n, np.uint8)
                m_t, ptr = _canary(env, n, torch.uint8)
                m_t[PAD:PAD + n] = _dev(env, old)
                rc = lib.rg_gate_mask_f32(d_t.data_ptr(), n, native.GATE_OPS[op], a, b, ptr, native.stream_ptr())
                assert rc == native.RG_OK, lib.rg_last_error()
                got, intact = _split(m_t, n)
                label = f"{op}({a!r}, {b!r}), n = {n}, {'prefilled' if prefill else 'zero'} mask"
                assert intact, f"{label}: bytes outside mask[0 .. n) were written"
                want = old | pred.astype(np.uint8)
                bad = np.nonzero(got != want)[0]
                assert bad.size == 0, (f"{label}: {bad.size} bytes differ; first at {bad[:4].tolist()}: data "
                                       f"{d[bad[:4]].tolist()} got {got[bad[:4]].tolist()} want {want[bad[:4]].tolist()}")
                n_calls += 1
                n_set += int(pred.sum())
            a32, b32 = np.float32(a), np.float32(b)
            n_edge += int(((d == a32) | (d == b32)).sum())
    print(f"{op}: {n_calls} launches, {n_set} gates excluded, {n_edge} data values exactly on a threshold")
    assert n_calls >= 18 and n_edge >= 100 and (n_set > 0)


# ---- 4. scan -------------------------------------------------------------------------------------------------------------
def _scan(env, counts, n, ws_offset=0):
    lib, native, torch = env["lib"], env["native"], env["torch"]
    c_t = _dev(env, counts)
    out, ptr = _canary(env, n + 1, torch.int64)
    ws_bytes = int(lib.rg_scan_workspace_bytes(n))
    raw = torch.empty(ws_bytes + 512, dtype=torch.uint8, device=env["dev"])
    base = (raw.data_ptr() + 255) // 256 * 256 + ws_offset
    assert base + ws_bytes <= raw.data_ptr() + raw.numel()
    rc = lib.rg_scan_counts_i64(c_t.data_ptr(), n, ptr, base, ws_bytes, native.stream_ptr())
    assert rc == native.RG_OK, lib.rg_last_error()
    got, intact = _split(out, n + 1)
    assert intact, "rg_scan_counts_i64 wrote outside indptr[0 .. n]"
    return got


def _check_scan(env, counts, n, label):
    want = np.concatenate([[0], np.cumsum(counts[:n].astype(np.int64))])
    for off in (0, 8):
        got = _scan(env, counts, n, ws_offset=off)
        assert got.dtype == np.int64 and np.array_equal(got, want), f"{label}, workspace + {off}: first difference at " \
            f"{int(np.argmax(got != want))} (total {int(got[-1])}, want {int(want[-1])})"
    return int(want[-1])


@pytest.mark.parametrize("n", [0, 1, 255, 256, 257, 65537, 1000003])
def test_scan_counts(env, n):
    """Random row lengths with 30 % zeros; the trailing counts[n] (12345) is read but never added; the workspace pointer
    aligned and offset by 8 bytes with exactly rg_scan_workspace_bytes(n) bytes."""
    rng = np.random.default_rng(n)
    counts = np.where(rng.random(n + 1) < 0.3, 0, rng.integers(0, 51, size=n + 1)).astype(np.int32)
    counts[n] = 12345
    total = _check_scan(env, counts, n, f"n = {n}")
    print(f"n = {n}: total {total}")
    assert total == int(counts[:n].sum(dtype=np.int64))


def test_scan_totals_beyond_int32_and_uint32(env):
    n = 5000
    rng = np.random.default_rng(9)
    counts = rng.integers(0, 2 ** 31, size=n + 1).astype(np.int32)
    counts[:3] = 2 ** 31 - 1                        # the running sum passes 2^31 after two rows, 2^32 after three
    counts[n] = 12345
    total = _check_scan(env, counts, n, "large counts")
    want = np.cumsum(counts[:n].astype(np.int64))
    assert want[1] >= 2 ** 31 and want[2] >= 2 ** 32 and total > 2 ** 40 and counts.max() == 2 ** 31 - 1
    print(f"large counts: total {total} = 2^{np.log2(total):.1f}")


def test_scan_refuses_a_short_workspace(env):
    lib, native, torch = env["lib"], env["native"], env["torch"]
    n = 1000
    c_t = _dev(env, np.ones(n + 1, dtype=np.int32))
    out = torch.zeros(n + 1, dtype=torch.int64, device=env["dev"])
    ws_bytes = int(lib.rg_scan_workspace_bytes(n))
    ws = torch.empty(ws_bytes, dtype=torch.uint8, device=env["dev"])
    assert lib.rg_scan_counts_i64(c_t.data_ptr(), n, out.data_ptr(), ws.data_ptr(), ws_bytes - 1, native.stream_ptr()) == native.RG_EWORKSPACE
    assert int(out.abs().sum().item()) == 0


# ---- 5. the gate lists -----------------------------------------------------------------------------------------------------
def _cellgrid(env, c, levels=0):
    return env["native"].CellGrid(x0=c.x0, y0=c.y0, inv_cx=c.inv_cx, inv_cy=c.inv_cy, z_lo=c.z_lo, z_hi=c.z_hi, ncx=c.ncx,
                                  ncy=c.ncy, levels=levels, level0=0)


def _gate_tensors(env, s):
    return [_dev(env, v) for v in (s.gx, s.gy, s.gz)]


def _records_of(t, n_records):
    """(records [n, 4] uint32, canaries intact?) of a canary tensor of 4 * n_records int32."""
    got, intact = _split(t, 4 * n_records)
    return got.view(np.uint32).reshape(n_records, 4), intact


def _as_u32(rec):
    return rec.view(np.uint32).reshape(-1, 4)


def _bin_single(env, s):
    lib, native, torch = env["lib"], env["native"], env["torch"]
    c = s.cells
    gx, gy, gz = _gate_tensors(env, s)
    n_cells = c.ncx * c.ncy
    sorted_t, sorted_ptr = _canary(env, 4 * max(s.n, 1), torch.int32)
    start_t, start_ptr = _canary(env, n_cells + 1, torch.int32)
    ws_bytes = int(lib.rg_geom_bin_workspace_bytes(s.n, c.ncx, c.ncy))
    assert ws_bytes > 0
    ws = torch.empty(ws_bytes, dtype=torch.uint8, device=env["dev"])
    rc = lib.rg_geom_bin_gates_f32(gx.data_ptr(), gy.data_ptr(), gz.data_ptr(), s.n, float(np.float32(s.alt)),
                                   float(np.float32(s.toa)), _cellgrid(env, c), sorted_ptr, start_ptr, ws.data_ptr(), ws_bytes,
                                   native.stream_ptr())
    assert rc == native.RG_OK, lib.rg_last_error()
    start, ok1 = _split(start_t, n_cells + 1)
    rec, ok2 = _records_of(sorted_t, max(s.n, 1))
    assert ok1 and ok2, f"{s.name}: a write outside cell_start[0 .. {n_cells}] or sorted_gates[0 .. n_gates)"
    return rec, start


@pytest.mark.parametrize("name", [s.name for s in ps.binning_scenes()])
def test_single_gate_list(env, name):
    """rg_geom_bin_gates_f32: cell_start and the records of the kept gates, bit for bit, in (cell, gate index) order; the
    records past n_binned are not written."""
    s = next(x for x in ps.binning_scenes() if x.name == name)
    want_rec, want_start = ps.bin_gates_ref(s.gx, s.gy, s.gz, s.alt, s.toa, s.cells)
    rec, start = _bin_single(env, s)
    n_binned = int(start[-1])
    _, keep, _ = ps.gate_cells(s.gx, s.gy, s.gz, s.alt, s.toa, s.cells)
    kept_planted = {case: int(keep[idx].sum()) for case, idx in s.planted.items()}
    print(f"{name}: {n_binned} of {s.n} gates binned; planted gates kept per case: {kept_planted}")
    assert n_binned == int(keep.sum()) == want_rec.size
    assert np.array_equal(start, want_start), f"cell_start differs at cells {np.nonzero(start != want_start)[0][:6].tolist()}"
    got = rec[:n_binned]
    bad = np.nonzero((got != _as_u32(want_rec)).any(axis=1))[0]
    assert bad.size == 0, (f"{bad.size} records differ; first at position {int(bad[0])}: got index {int(got[bad[0], 3])}, "
                           f"want {int(want_rec['index'][bad[0]])}")
    canary = np.uint32(CANARY32)
    assert (rec[n_binned:] == canary).all(), "a record past n_binned was written"
    for case, (kept, need) in ps.PLANTED.items():
        if name.startswith("planted_"):
            assert kept_planted[case] == (len(s.planted[case]) if kept else 0) and len(s.planted[case]) >= need


def _bin_levels(env, s):
    lib, native, torch = env["lib"], env["native"], env["torch"]
    c, nz = s.cells, len(s.zc)
    gx, gy, gz = _gate_tensors(env, s)
    zc_t = _dev(env, s.zc)
    cells = _cellgrid(env, c, levels=nz)
    head = (gx.data_ptr(), gy.data_ptr(), gz.data_ptr(), s.n, float(np.float32(s.alt)), float(np.float32(s.toa)), cells,
            zc_t.data_ptr(), nz, s.min_radius, s.beam_factor)
    total = torch.full((1,), -7, dtype=torch.int64, device=env["dev"])
    rc = lib.rg_geom_bin_levels_count(*head, total.data_ptr(), native.stream_ptr())
    assert rc == native.RG_OK, lib.rg_last_error()
    n_entries = int(total.item())
    assert 0 <= n_entries <= nz * s.n
    n_cells = nz * c.ncx * c.ncy
    sorted_t, sorted_ptr = _canary(env, 4 * max(n_entries, 1), torch.int32)
    start_t, start_ptr = _canary(env, n_cells + 1, torch.int32)
    ws_bytes = int(lib.rg_geom_bin_levels_workspace_bytes(s.n, n_entries, n_cells))
    assert ws_bytes > 0
    ws = torch.empty(ws_bytes, dtype=torch.uint8, device=env["dev"])
    rc = lib.rg_geom_bin_gates_levels_f32(*head, n_entries, sorted_ptr, start_ptr, ws.data_ptr(), ws_bytes, native.stream_ptr())
    assert rc == native.RG_OK, lib.rg_last_error()
    start, ok1 = _split(start_t, n_cells + 1)
    rec, ok2 = _records_of(sorted_t, max(n_entries, 1))
    assert ok1 and ok2, f"{s.name}: a write outside cell_start or sorted_gates[0 .. n_entries)"
    return rec[:n_entries], start, n_entries


def _check_level_lists(env, s):
    """The per-level lists of scene ``s`` against the reference: returns the listed (level, gate) set after asserting the
    count, the must / never / free-band rule, the (level, cell, gate index) order, the records and cell_start."""
    rec, start, n_entries = _bin_levels(env, s)
    assert int(start[-1]) == n_entries, f"count pass {n_entries}, cell_start[-1] {int(start[-1])}"
    nz, n_cells = len(s.zc), s.cells.ncx * s.cells.ncy
    level = np.searchsorted(start[::n_cells], np.arange(n_entries), side="right") - 1
    assert level.min(initial=0) >= 0 and level.max(initial=0) < nz
    gate = rec[:, 3].astype(np.int64)
    assert gate.min(initial=0) >= 0 and gate.max(initial=0) < s.n
    listed = np.zeros((nz, s.n), dtype=bool)
    listed[level, gate] = True
    assert int(listed.sum()) == n_entries, "a (level, gate) pair is listed twice"
    must, may, never = ps.level_lists_ref(s.gx, s.gy, s.gz, s.alt, s.toa, s.cells, s.zc, s.min_radius, s.beam_factor)
    n_missing, n_never, n_may = int((must & ~listed).sum()), int((listed & never).sum()), int((listed & may).sum())
    print(f"{s.name}: {n_entries} entries; {int(must.sum())} required, {n_missing} missing, {n_never} beyond the inflation, "
          f"{n_may} in the free band")
    assert n_missing == 0, f"{n_missing} required (level, gate) pairs are not listed, first {np.argwhere(must & ~listed)[:4].tolist()}"
    assert n_never == 0 and n_may <= 0.01 * n_entries
    want_rec, want_start = ps.level_order_ref(s.gx, s.gy, s.gz, s.alt, s.toa, s.cells, listed)
    assert np.array_equal(start, want_start), f"cell_start differs at {np.nonzero(start != want_start)[0][:6].tolist()}"
    bad = np.nonzero((rec != _as_u32(want_rec)).any(axis=1))[0]
    assert bad.size == 0, f"{bad.size} entries out of (level, cell, gate index) order or with other bits; first at {int(bad[0])}"
    return listed


@pytest.mark.parametrize("alt", ps.LEVEL_ALTS)
@pytest.mark.parametrize("min_radius,beam_factor", ps.LEVEL_PARAMS)
def test_per_level_gate_lists(env, min_radius, beam_factor, alt):
    """rg_geom_bin_levels_count + rg_geom_bin_gates_levels_f32: the count is the number of entries written; the listed
    (level, gate) set holds every pair within R_g, none beyond the documented inflation, at most 1 % in between; the entries
    are in (level, cell, gate index) order with the single list's records and the matching cell_start."""
    s = ps.level_scene(min_radius, beam_factor, alt)
    listed = _check_level_lists(env, s)
    inside = sum(bool(listed[s.planted_level[int(i)], i]) for i in s.planted["inside"])
    outside = sum(bool(listed[s.planted_level[int(i)], i]) for i in s.planted["outside"])
    print(f"{s.name}: planted just inside {inside}/{len(s.planted['inside'])} listed, just outside {outside}")
    assert inside == len(s.planted["inside"]) == ps.N_LEVEL_EDGE and outside == 0


def test_per_level_gate_lists_exactly_on_the_bound(env):
    """Gates whose distance to a level IS the reach bound (|dz| = 9 |g| / 11 at beam_factor 0.45, every number exact): only
    the float64 rounding of R_g decides about them, which is what the lists' inflation covers -- every pair the reference's
    R_g admits is listed, and so is every planted pair (none of them lies beyond the inflation)."""
    s = ps.on_bound_scene()
    listed = _check_level_lists(env, s)
    k, g = np.array(s.pairs).T
    print(f"on-bound scene: {int(listed[k, g].sum())} of {len(s.pairs)} planted pairs listed")
    assert listed[k, g].all()


# ---- 6. neighbour completeness near the limit of beam_factor ---------------------------------------------------------------
@pytest.mark.parametrize("eps", ps.VERTICAL_EPS)
@pytest.mark.parametrize("beam_factor", ps.VERTICAL_BEAMS)
def test_neighbours_on_the_vertical_near_the_beam_factor_limit(env, beam_factor, eps):
    """Gates on the radar's vertical at r_v (1 - eps) below and above their voxel, where the per-level reach bound is tight:
    per-level lists and the single list return the oracle's CSR (indices equal, Cressman and uniform weights bit for bit,
    Barnes within one ulp) and the CSR-free gridder its NaN pattern; every planted gate is in its voxel's row."""
    rg, dev = env["rg"], env["dev"]
    s = ps.vertical_rim_scene(beam_factor, eps)
    rng = np.random.default_rng(5)
    val = rng.normal(20.0, 10.0, s.gx.size).astype(np.float32)
    mask = rng.random(s.gx.size) < 0.15
    mask[:len(s.planted)] = False
    roi = dict(min_radius=s.min_radius, beam_factor=s.beam_factor)
    for per_level in (True, False):
        search = rg.RoiSearch(s.gx, s.gy, s.gz, s.shape, s.limits, device=dev, per_level=per_level, **roi)
        assert search.per_level == per_level
        for weighting in ("barnes2", "cressman", "nearest"):
            o_ip, o_idx, o_w = oracle.build_geometry(s.gx, s.gy, s.gz, s.shape, s.limits, weighting=weighting, **roi)
            label = f"bf {beam_factor} eps {eps} per_level {per_level} {weighting}"
            csr = search.build_csr(weighting)
            _check_csr(csr, o_ip, o_idx, o_w, weighting, label)
            ip, idx = csr.indptr.cpu().numpy().astype(np.int64), csr.gate_indices.cpu().numpy()
            found = sum(g in idx[ip[v]:ip[v + 1]] for v, g in s.planted)
            assert found == len(s.planted) == 2 * s.shape[0], f"{label}: {found} of {len(s.planted)} planted gates found"
            got = rg.roi_grid_fields_device(search, [_dev(env, val)], [_dev(env, mask.astype(np.uint8))],
                                            weighting=weighting)[0].cpu().numpy()
            want = oracle.csr_apply_f64(o_ip, o_idx, o_w, val, mask, s.shape)
            assert np.array_equal(np.isnan(got), np.isnan(want)), label
        print(f"bf {beam_factor} eps {eps} per_level {per_level}: {int(o_ip[-1])} pairs, {found} planted gates in their rows, "
              f"smallest margin to the rim {s.margins.min():.2e} m")
