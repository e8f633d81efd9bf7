"""Connected-component labelling, the cell table and despeckling on the GPU (csrc/rg_components.hip) against the flood-fill
restatement of tests/components_oracle.py, through the public functions and through the raw C ABI.

Shapes (tests/component_scenes.py) follow from the tile constants: one pixel, one row and one column across two seams, exactly
one tile, one pixel more each way, and several tiles with ragged edges -- nothing above 69 x 199.  Asserted: ``labels`` and
``cell_ptr`` equal the oracle's; ``area``, ``bbox``, ``sum_yx``, ``vmax`` (bitwise) and ``argmax`` exactly;
``|vsum - fsum| <= area * 2^-53 * sum|v|`` per cell, the worst-case bound of a float64 sum in any order (a non-finite sum must
be the same non-finite value); despeckle output and mask bytewise, in place too; a second run gives identical bytes for
everything but ``vsum``."""
import functools

import numpy as np
import pytest

import component_scenes as cs
import components_oracle as co

pytestmark = pytest.mark.gpu
CANARY = 64
SHAPE_IDS = [f"{h}x{w}" for h, w in cs.SHAPES]


@pytest.fixture(scope="module")
def env():
    import torch
    import radar_processor_amd as rg
    from radar_processor_amd import _native
    lib = rg.load_library()
    return dict(torch=torch, rg=rg, native=_native, lib=lib, dev=torch.device("cuda", 0))


@functools.lru_cache(maxsize=None)
def reference(shape, name, connectivity):
    """(labels, cell_ptr, table) of one scene from the oracle: computed once, shared by every test."""
    s = cs.scene(shape, name)
    labels, cell_ptr = co.label(s.planes, s.lo, s.hi, s.mask, connectivity, s.wrap)
    table = co.stats(s.planes, labels, cell_ptr)
    for a in (labels, cell_ptr, *table.values()):
        a.setflags(write=False)
    return labels, cell_ptr, table


def _dev(env, a):
    return None if a is None else env["torch"].from_numpy(np.array(a)).to(env["dev"])


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def _check_table(got, want, where):
    """``got``: a dict of host arrays from the device; ``want``: the oracle's table."""
    for name in ("area", "bbox", "sum_yx", "argmax"):
        np.testing.assert_array_equal(got[name], want[name], err_msg=f"{where}: {name}")
    np.testing.assert_array_equal(_bits(got["vmax"]), _bits(want["vmax"]), err_msg=f"{where}: vmax bits")
    finite = np.isfinite(want["vsum"])
    np.testing.assert_array_equal(got["vsum"][~finite], want["vsum"][~finite], err_msg=f"{where}: non-finite vsum")
    bound = want["area"] * 2.0 ** -53 * want["abs_sum"]
    excess = np.abs(got["vsum"][finite] - want["vsum"][finite]) - bound[finite]
    assert not excess.size or excess.max() <= 0.0, f"{where}: vsum lies {excess.max()} beyond the bound"


def _table_host(t):
    return {k: v.cpu().numpy() for k, v in t._asdict().items() if v is not None and hasattr(v, "cpu")}


def _label_and_table(env, s, connectivity):
    rg = env["rg"]
    planes, mask = _dev(env, s.planes), _dev(env, s.mask)
    labels, cell_ptr = rg.label_components_device(planes, s.lo, upper=s.hi, mask=mask, connectivity=connectivity,
                                                  wrap_rows=s.wrap)
    table = rg.cell_table_device(planes, labels, cell_ptr)
    return labels.cpu().numpy(), cell_ptr.cpu().numpy(), _table_host(table)


def _check_scene(env, shape, name, connectivity):
    s = cs.scene(shape, name)
    where = f"{shape} {name} connectivity {connectivity}"
    want_labels, want_ptr, want = reference(shape, name, connectivity)
    labels, cell_ptr, table = _label_and_table(env, s, connectivity)
    print(f"{where}: {int(want_ptr[-1])} cells, largest {int(want['area'].max()) if len(want['area']) else 0} pixels")
    assert labels.dtype == np.int32 and cell_ptr.dtype == np.int32
    np.testing.assert_array_equal(cell_ptr, want_ptr, err_msg=f"{where}: cell_ptr")
    np.testing.assert_array_equal(labels, want_labels, err_msg=f"{where}: labels")
    np.testing.assert_array_equal(table["plane"], want["plane"], err_msg=f"{where}: plane")
    np.testing.assert_array_equal(table["id"], want["id"], err_msg=f"{where}: id")
    _check_table(table, want, where)
    return labels, cell_ptr, table


# ---- the first run of the kernels: the two smallest shapes alone -----------------------------------------------------------
@pytest.mark.parametrize("connectivity", (4, 8))
@pytest.mark.parametrize("shape", cs.FIRST_RUN_SHAPES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_first_run_one_pixel_and_one_tile(env, shape, connectivity):
    for s in cs.scenes(shape):
        _check_scene(env, shape, s.name, connectivity)


# ---- every scene at every shape --------------------------------------------------------------------------------------------
@pytest.mark.parametrize("connectivity", (4, 8))
@pytest.mark.parametrize("shape", cs.SHAPES, ids=SHAPE_IDS)
def test_labels_and_table_equal_the_oracle_and_repeat(env, shape, connectivity):
    for s in cs.scenes(shape):
        first = _check_scene(env, shape, s.name, connectivity)
        again = _label_and_table(env, s, connectivity)                       # a second run: identical bytes but for vsum
        assert first[0].tobytes() == again[0].tobytes() and first[1].tobytes() == again[1].tobytes(), s.name
        for name in ("plane", "id", "area", "bbox", "sum_yx", "vmax", "argmax"):
            assert first[2][name].tobytes() == again[2][name].tobytes(), (s.name, name)


@pytest.mark.parametrize("connectivity", (4, 8))
@pytest.mark.parametrize("shape", cs.SHAPES, ids=SHAPE_IDS)
def test_despeckle_equals_the_oracle_bytewise(env, shape, connectivity):
    rg, nat, lib, torch = env["rg"], env["native"], env["lib"], env["torch"]
    n_px = shape[0] * shape[1]
    for s in cs.scenes(shape):
        labels, cell_ptr, table = reference(shape, s.name, connectivity)
        largest = int(table["area"].max()) if len(table["area"]) else 1
        planes, mask = _dev(env, s.planes), _dev(env, s.mask)
        labels_t, ptr_t, area_t = _dev(env, labels), _dev(env, cell_ptr), _dev(env, table["area"])
        for min_size, fill in ((1, np.nan), (2, -9.25), (largest, np.nan), (largest + 1, 0.0)):
            where = f"{shape} {s.name} connectivity {connectivity} min_size {min_size}"
            want, want_removed = co.despeckle_labelled(s.planes, labels, cell_ptr, min_size, fill)
            out, removed = rg.despeckle_device(planes, s.lo, min_size, upper=s.hi, mask=mask, connectivity=connectivity,
                                               wrap_rows=s.wrap, fill_value=fill, return_mask=True)
            assert out.shape == planes.shape and out.dtype == torch.float32 and removed.dtype == torch.uint8
            assert out.cpu().numpy().tobytes() == want.tobytes(), where
            assert removed.cpu().numpy().tobytes() == want_removed.tobytes(), where
            assert (largest + 1 != min_size) or int(want_removed.sum()) == int(table["area"].sum())      # all cells go
            # the raw entry point in place (src == out), from the oracle's labelling, without a mask output
            work = planes.clone()
            n = s.planes.shape[0]
            if len(table["area"]):
                with torch.cuda.device(env["dev"]):
                    assert lib.rg_despeckle_select_f32(nat.ptr(work), nat.ptr(labels_t), nat.ptr(ptr_t), nat.ptr(area_t), n,
                                                       shape[0], shape[1], min_size, fill, nat.ptr(work), 0,
                                                       nat.stream_ptr()) == 0
                assert work.cpu().numpy().tobytes() == want.tobytes(), f"{where}: in place"
        assert planes.cpu().numpy().tobytes() == s.planes.tobytes()                                       # inputs untouched
        # the NumPy convenience, 2-D in and out
        if s.planes.shape[0] == 1:
            got = rg.despeckle(s.planes[0], s.lo, 2, upper=s.hi, mask=None if s.mask is None else s.mask[0],
                               connectivity=connectivity, wrap_rows=s.wrap)
            assert isinstance(got, np.ndarray) and got.shape == shape
            assert got.tobytes() == co.despeckle_labelled(s.planes, labels, cell_ptr, 2)[0][0].tobytes(), s.name
    assert n_px > 0


# ---- the raw C ABI: pointers offset by one element, canaries, NULL outputs --------------------------------------------------
def _guarded(env, n, dtype, pattern):
    """A buffer of 2 * CANARY + n + 1 elements filled with ``pattern``; the view starts ONE element past the canary."""
    buf = env["torch"].full((2 * CANARY + n + 1,), pattern, dtype=dtype, device=env["dev"])
    return buf, buf[CANARY + 1:CANARY + 1 + n]


def _intact(buf, n, pattern):
    host = buf.cpu().numpy()
    return bool((host[:CANARY + 1] == pattern).all() and (host[CANARY + 1 + n:] == pattern).all())


@pytest.mark.parametrize("connectivity", (4, 8))
@pytest.mark.parametrize("name", ("random_0.41", "random_0.593", "lattice", "three_planes_wrap", "spiral", "all_foreground"))
def test_raw_abi_with_offset_pointers_and_canaries(env, name, connectivity):
    torch, nat, lib = env["torch"], env["native"], env["lib"]
    shape = cs.SHAPES[-1]
    s = cs.scene(shape, name)
    want_labels, want_ptr, want = reference(shape, name, connectivity)
    n, (h, w) = s.planes.shape[0], shape
    px, cells = n * h * w, int(want_ptr[-1])
    src_buf, src = _guarded(env, px, torch.float32, -12345.5)
    src.copy_(torch.from_numpy(s.planes.ravel()))
    mask_t = None
    if s.mask is not None:
        mask_buf, mask_t = _guarded(env, px, torch.uint8, 0)
        mask_t.copy_(torch.from_numpy(s.mask.ravel()))
    lab_buf, lab = _guarded(env, px, torch.int32, -77)
    ptr_buf, ptr = _guarded(env, n + 1, torch.int32, -77)
    need = int(lib.rg_components_workspace_bytes(n, h, w))
    ws_buf, ws = _guarded(env, need // 4, torch.int32, -77)
    with torch.cuda.device(env["dev"]):
        assert lib.rg_label_components_f32(nat.ptr(src), nat.ptr(mask_t), n, h, w, s.lo, s.hi, connectivity, int(s.wrap),
                                           nat.ptr(lab), nat.ptr(ptr), nat.ptr(ws), need, nat.stream_ptr()) == 0
    np.testing.assert_array_equal(ptr.cpu().numpy(), want_ptr)
    np.testing.assert_array_equal(lab.cpu().numpy().reshape(n, h, w), want_labels)
    assert _intact(lab_buf, px, -77) and _intact(ptr_buf, n + 1, -77) and _intact(ws_buf, need // 4, -77)
    assert _intact(src_buf, px, -12345.5) and src.cpu().numpy().tobytes() == s.planes.tobytes()
    # a workspace one byte short is refused before any launch
    with torch.cuda.device(env["dev"]):
        assert lib.rg_label_components_f32(nat.ptr(src), nat.ptr(mask_t), n, h, w, s.lo, s.hi, connectivity, int(s.wrap),
                                           nat.ptr(lab), nat.ptr(ptr), nat.ptr(ws), need - 1,
                                           nat.stream_ptr()) == nat.RG_EWORKSPACE
    # the table into offset outputs (the 8-byte ones offset by one of THEIR elements)
    out = dict(area=_guarded(env, cells, torch.int32, -77), bbox=_guarded(env, 4 * cells, torch.int32, -77),
               sum_yx=_guarded(env, 2 * cells, torch.int64, -77), vmax=_guarded(env, cells, torch.float32, -12345.5),
               argmax=_guarded(env, cells, torch.int32, -77), vsum=_guarded(env, cells, torch.float64, -12345.5))
    with torch.cuda.device(env["dev"]):
        assert lib.rg_component_stats_f32(nat.ptr(src), nat.ptr(lab), nat.ptr(ptr), n, h, w, cells, *(nat.ptr(out[k][1]) for k in
                                          ("area", "bbox", "sum_yx", "vmax", "argmax", "vsum")), nat.stream_ptr()) == 0
    got = {k: v[1].cpu().numpy() for k, v in out.items()}
    got["bbox"], got["sum_yx"] = got["bbox"].reshape(cells, 4), got["sum_yx"].reshape(cells, 2)
    _check_table(got, want, f"{name} connectivity {connectivity} (raw)")
    for k, (buf, view) in out.items():
        assert _intact(buf, view.numel(), -77 if buf.dtype in (torch.int32, torch.int64) else -12345.5), k
    # any output may be NULL: each one alone gives the same bytes (argmax needs vmax)
    for k in ("area", "bbox", "sum_yx", "vmax", "vsum"):
        buf, view = _guarded(env, out[k][1].numel(), out[k][1].dtype, -77 if out[k][1].dtype in (torch.int32, torch.int64) else -12345.5)
        args = [nat.ptr(view) if j == k else 0 for j in ("area", "bbox", "sum_yx", "vmax", "argmax", "vsum")]
        with torch.cuda.device(env["dev"]):
            assert lib.rg_component_stats_f32(nat.ptr(src), nat.ptr(lab), nat.ptr(ptr), n, h, w, cells, *args, nat.stream_ptr()) == 0
        if k != "vsum":
            assert view.cpu().numpy().tobytes() == out[k][1].cpu().numpy().tobytes(), k
    # despeckle into offset outputs
    o_buf, o = _guarded(env, px, torch.float32, -12345.5)
    m_buf, m = _guarded(env, px, torch.uint8, 7)
    with torch.cuda.device(env["dev"]):
        assert lib.rg_despeckle_select_f32(nat.ptr(src), nat.ptr(lab), nat.ptr(ptr), nat.ptr(out["area"][1]), n, h, w, 3, -1.5,
                                           nat.ptr(o), nat.ptr(m), nat.stream_ptr()) == 0
    want_out, want_removed = co.despeckle_labelled(s.planes, want_labels, want_ptr, 3, -1.5)
    assert o.cpu().numpy().tobytes() == want_out.tobytes() and m.cpu().numpy().tobytes() == want_removed.tobytes()
    assert _intact(o_buf, px, -12345.5) and _intact(m_buf, px, 7)


def test_c_abi_refusals_and_empty_planes(env):
    torch, nat, lib = env["torch"], env["native"], env["lib"]
    src = torch.zeros((2, 4, 5), dtype=torch.float32, device=env["dev"])
    lab = torch.zeros((2, 4, 5), dtype=torch.int32, device=env["dev"])
    ptr = torch.full((3,), -77, dtype=torch.int32, device=env["dev"])
    ws = torch.zeros(64, dtype=torch.int32, device=env["dev"])
    inf = float("inf")

    def call(src_p=nat.ptr(src), n=2, h=4, w=5, lo=0.0, hi=inf, c=8, lab_p=nat.ptr(lab), ptr_p=nat.ptr(ptr), ws_p=nat.ptr(ws),
             ws_bytes=256):
        with torch.cuda.device(env["dev"]):
            return lib.rg_label_components_f32(src_p, 0, n, h, w, lo, hi, c, 0, lab_p, ptr_p, ws_p, ws_bytes, nat.stream_ptr())

    assert call() == 0 and ptr.cpu().tolist() == [0, 1, 2] and (lab == 1).all()
    for kw in (dict(src_p=0), dict(lab_p=0), dict(ptr_p=0), dict(ws_p=0), dict(n=0), dict(h=-1), dict(w=-1), dict(c=6), dict(c=0),
               dict(lo=float("nan")), dict(hi=float("nan")), dict(n=2, h=32768, w=32768), dict(lab_p=nat.ptr(src) + 8)):
        assert call(**kw) == nat.RG_EINVAL, kw
        assert lib.rg_last_error().decode().startswith("rg_label_components_f32")
    assert call(ws_bytes=160) == nat.RG_EWORKSPACE and call(lab_p=nat.ptr(lab) + 2) == nat.RG_EALIGN
    ptr.fill_(-77)
    assert call(h=0) == 0 and ptr.cpu().tolist() == [0, 0, 0]                   # no pixels: cell_ptr is zeroed
    with torch.cuda.device(env["dev"]):
        area = torch.zeros(2, dtype=torch.int32, device=env["dev"])
        stats = lambda **kw: lib.rg_component_stats_f32(*[kw.get(k, d) for k, d in (
            ("src", nat.ptr(src)), ("lab", nat.ptr(lab)), ("ptr", nat.ptr(ptr)), ("n", 2), ("h", 4), ("w", 5), ("cells", 2),
            ("area", nat.ptr(area)), ("bbox", 0), ("sum_yx", 0), ("vmax", 0), ("argmax", 0), ("vsum", 0))], nat.stream_ptr())
        for kw in (dict(src=0), dict(lab=0), dict(ptr=0), dict(n=0), dict(cells=-1), dict(argmax=nat.ptr(area))):
            assert stats(**kw) == nat.RG_EINVAL, kw
        assert stats(cells=0, src=0) == 0
        select = lambda **kw: lib.rg_despeckle_select_f32(*[kw.get(k, d) for k, d in (
            ("src", nat.ptr(src)), ("lab", nat.ptr(lab)), ("ptr", nat.ptr(ptr)), ("area", nat.ptr(area)), ("n", 2), ("h", 4),
            ("w", 5), ("min_size", 1), ("fill", 0.0), ("out", nat.ptr(src)), ("mask", 0))], nat.stream_ptr())
        for kw in (dict(src=0), dict(lab=0), dict(ptr=0), dict(area=0), dict(out=0), dict(min_size=0), dict(w=-1)):
            assert select(**kw) == nat.RG_EINVAL, kw
    torch.cuda.synchronize()


# ---- the cell table with a geometry, and identify_cells --------------------------------------------------------------------
class _Geometry:
    def __init__(self, shape):
        self.grid_shape = (5,) + tuple(shape)
        self.grid_limits = ((0.0, 8000.0), (-34250.0, 33750.0), (-99000.0, 99000.0))


@pytest.mark.parametrize("connectivity", (4, 8))
def test_cell_table_with_a_geometry_and_identify_cells(env, connectivity):
    rg = env["rg"]
    shape = cs.SHAPES[-1]
    geometry = _Geometry(shape)
    for name in ("random_0.41", "random_0.8", "comb"):
        s = cs.scene(shape, name)
        labels, cell_ptr, want = reference(shape, name, connectivity)
        planes = _dev(env, s.planes[0])                                    # a 2-D plane in, 2-D labels out
        labels_t, ptr_t = rg.label_components_device(planes, s.lo, connectivity=connectivity)
        assert tuple(labels_t.shape) == shape
        table = rg.cell_table_device(planes, labels_t, ptr_t, geometry)
        metres = co.centroids(want, geometry.grid_shape, geometry.grid_limits)
        for col, ref in metres.items():
            got = getattr(table, col)
            assert got.dtype == np.float64 and got.tobytes() == ref.tobytes(), (name, col)
        assert (metres["area_km2"] > 0).all()
        # identify_cells: the oracle's table filtered by min_size, ordered by id
        for min_size in (1, 4, int(want["area"].max()), int(want["area"].max()) + 1):
            keep = want["area"] >= min_size
            cells = rg.identify_cells(s.planes[0], geometry, s.lo, min_size=min_size, connectivity=connectivity)
            assert sorted(cells) == sorted(["id", "area", "bbox", "sum_yx", "vmax", "argmax", "vsum", *metres])
            _check_table(cells, {k: v[keep] for k, v in want.items()}, f"{name} identify_cells min_size {min_size}")
            np.testing.assert_array_equal(cells["id"], want["id"][keep])
            for col, ref in metres.items():
                assert cells[col].tobytes() == ref[keep].tobytes(), (name, col, min_size)
        assert "centroid_x" not in rg.identify_cells(s.planes[0], None, s.lo)


def test_labelling_runs_on_the_current_stream_without_synchronising(env):
    """Label and despeckle on a side stream while the default stream is idle: the results are right after that stream's own
    synchronisation, so every launch went to the caller's stream."""
    torch, rg = env["torch"], env["rg"]
    shape = cs.SHAPES[-1]
    s = cs.scene(shape, "random_0.593")
    want_labels, want_ptr, _ = reference(shape, "random_0.593", 4)
    planes = _dev(env, s.planes)
    torch.cuda.synchronize()
    side = torch.cuda.Stream(device=env["dev"])
    with torch.cuda.stream(side):
        labels, cell_ptr = rg.label_components_device(planes, s.lo, connectivity=4)
        out = rg.despeckle_device(planes, s.lo, 5, connectivity=4)
    side.synchronize()
    np.testing.assert_array_equal(labels.cpu().numpy(), want_labels)
    np.testing.assert_array_equal(cell_ptr.cpu().numpy(), want_ptr)
    assert out.cpu().numpy().tobytes() == co.despeckle_labelled(s.planes, want_labels, want_ptr, 5)[0].tobytes()
