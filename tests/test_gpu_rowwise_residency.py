"""The one-field grid-mode row-wise kernel after its scalar diet (one chunk per workgroup at compile time, the split-chunk
dictionary bounds read inside the per-pair path only; seven workgroups per CU instead of six, EXPERIMENTS R5.3): every path of
the streaming code on the smallest geometry that reaches it, through ``rg_csr_compact_apply_packed_f32_ex`` with ``int`` and ``long`` row pointers.

  dense130  grid (1, 4, 130): unbalanced segments of 44 / 43 / 43 rows, 400 gates -- the window + 14-byte records; the same
            geometry with a window of 64 entries, smaller than every dictionary -- the per-pair path over 14-byte records;
  gap130    dense130 with its middle chunk emptied: a chunk without a record (the early exit) between two full ones;
  wide64    grid (1, 4, 64), every row mentions all 2100 gates: more than 2048 dictionary entries (16-byte records), and a
            segment spans 134 400 pairs, more than the 16-bit row ends hold (the row-pointer fallback), 64 lanes per row;
  split64   grid (1, 4, 64), 66 560 distinct gates in one chunk: a split dictionary, the per-pair path over 16-byte records.

Nothing there may change a byte read or the order of an addition: every grid is compared BIT FOR BIT with
``oracle.csr_apply_rowwise_order`` at the same lane split, no voxel keeps its prefill and the guard words keep theirs.
(tests/test_gpu_row_ends.py scene B already drives wide records, the fallback and an empty chunk at one field with ``int`` row
pointers through ``CsrGridder.apply``; tests/test_gpu_rowwise_prologue.py the short-row cases with both pointer types.)
"""
import numpy as np
import pytest

import row_ends_scenes as helpers
from oracle import radar_grid_oracle as oracle

pytestmark = pytest.mark.gpu

LIMITS = ((0.0, 1.0), (0.0, 1.0), (0.0, 1.0))
FILL = -3.0
PREFILL = 12345.0
GUARD = 64
SHAPE_130, SHAPE_64 = (1, 4, 130), (1, 4, 64)
SMALL_WINDOW = 64


def _dense130(gap):
    rng = np.random.default_rng(1701 + gap)
    lengths = np.zeros(4 * 130, dtype=np.int64)
    for (line, sx, r0, nrows, chunk) in helpers.segments(SHAPE_130):
        if gap and sx == 1:
            continue
        lengths[r0:r0 + nrows] = rng.choice([0, 1, 2, 3, 4, 5, 7, 11, 40], size=nrows)
        lengths[r0] = lengths[r0 + nrows - 1] = 0                 # empty rows at both ends of a segment
        lengths[r0 + 1] = 200                                     # a row of several steps
    return helpers._finish(SHAPE_130, lengths, lambda seg, n: (seg[1] * 50 + rng.integers(0, 300, size=n)) % 400, rng, 400)


def _wide64():
    rng = np.random.default_rng(1703)
    lengths = np.full(4 * 64, 2100, dtype=np.int64)
    return helpers._finish(SHAPE_64, lengths, lambda seg, n: (np.arange(n) + 13 * seg[0]) % 2100, rng, 2100)


def _split64():
    rng = np.random.default_rng(1704)
    lengths = np.full(4 * 64, 260, dtype=np.int64)
    perm = rng.permutation(4 * 64 * 260)

    def gidx_of(seg, n):
        return perm[seg[0] * 64 * 260:seg[0] * 64 * 260 + n]
    return helpers._finish(SHAPE_64, lengths, gidx_of, rng, 4 * 64 * 260 + 40)


SCENES = {"dense130": lambda: _dense130(0), "gap130": lambda: _dense130(1), "wide64": _wide64, "split64": _split64}
# (scene, window: None = the geometry's own, lane splits)
CASES = [("dense130", None, (0, 2, 64)), ("dense130", SMALL_WINDOW, (0, 2, 64)), ("gap130", None, (0, 8)),
         ("wide64", None, (0,)), ("split64", None, (0,))]


@pytest.fixture(scope="module")
def rg():
    import radar_processor_amd as rg
    rg.load_library()
    return rg


class _Scene:
    def __init__(self, name):
        import torch
        from radar_processor_amd import _native
        from radar_processor_amd.grid_geometry import CompactCSR, DeviceCSR, GridGeometry
        from radar_processor_amd.gridding import CsrGridder
        self.torch = torch
        self.c = c = SCENES[name]()
        self.shape = c["shape"]
        self.n_vox = int(np.prod(self.shape))
        self.dev = dev = torch.device("cuda")
        self.csr = DeviceCSR(torch.from_numpy(c["indptr"].astype(np.int32)).to(dev), torch.from_numpy(c["gidx"]).to(dev),
                             torch.from_numpy(c["wts"]).to(dev), int(c["gidx"].max()))
        self.indptr64 = torch.from_numpy(c["indptr"]).to(dev)
        self.gridders = {}
        for order in (_native.RG_REC_ORDER_DISPATCH, _native.RG_REC_ORDER_SEGMENT):
            compact = CompactCSR.build(self.csr, self.shape)
            compact.rec_order = order
            assert compact.ensure_packed(self.csr) and compact.row_end16 is not None
            geom = GridGeometry.from_device(self.shape, LIMITS, self.csr, 17000.0, compact=compact)
            gr = CsrGridder(geom, c["n_gates"], 1, device=dev)
            gr.compact, gr.packed_stream, gr.tile = compact, True, 0
            gr.window = compact.window_for(1, rowwise=True)
            gr.pack([torch.from_numpy(c["fields"][0]).to(dev)], [torch.from_numpy(c["masks"][0].astype(np.uint8)).to(dev)])
            self.gridders[order] = gr
        self._emu = {}

    def emu(self, hint):
        if hint not in self._emu:
            c = self.c
            self._emu[hint] = oracle.csr_apply_rowwise_order(c["indptr"], c["gidx"], c["wts"], c["fields"][:1], c["masks"][:1],
                                                             self.shape, fill_value=FILL, lanes_hint=hint).reshape(1, self.n_vox)
        return self._emu[hint]


@pytest.fixture(scope="module")
def scene(rg):
    cache = {}

    def get(name):
        if name not in cache:
            cache[name] = _Scene(name)
        return cache[name]
    return get


def _same_bits(got, want_np):
    got_np = got.cpu().numpy()
    if not np.array_equal(np.isnan(got_np), np.isnan(want_np)):
        return False
    live = ~np.isnan(want_np)
    return np.array_equal(got_np.view(np.int32)[live], want_np.view(np.int32)[live])


def test_scenes_reach_the_paths_they_are_named_for(rg, scene):
    from radar_processor_amd import _native
    sizes, spans, windows, empty = {}, {}, {}, {}
    for name in SCENES:
        s = scene(name)
        compact = s.gridders[_native.RG_REC_ORDER_DISPATCH].compact
        sizes[name] = (compact.dict_ptr[1:] - compact.dict_ptr[:-1]).cpu().numpy()
        spans[name] = np.array(sorted(s.c["spans"].values()))
        windows[name] = s.gridders[_native.RG_REC_ORDER_DISPATCH].window
        rp = compact.rec_ptr.cpu().numpy()
        empty[name] = [bool(rp[b * helpers.LINES] == rp[(b + 1) * helpers.LINES]) for b in range(len(sizes[name]))]
    dense = _native.RG_DENSE_MAX_DICT
    assert [seg[3] for seg in helpers.segments(SHAPE_130)[:3]] == [44, 43, 43]
    for name in ("dense130", "gap130"):                              # window + 14-byte records, 16-bit row ends
        assert sizes[name].max() <= dense and sizes[name].max() <= windows[name] and spans[name].max() <= helpers.ROW_END16_MAX
    assert SMALL_WINDOW < sizes["dense130"].min()                      # per-pair path in every chunk
    assert sum(empty["gap130"]) == 1 and not any(empty["dense130"])
    assert sorted(scene("gap130").c["chunk_pairs"] == 0) == [False, False, True] and scene("gap130").c["chunk_pairs"][1] == 0
    assert sizes["wide64"].tolist() == [2100] and dense < 2100 <= windows["wide64"]      # window + 16-byte records
    assert spans["wide64"].min() == 64 * 2100 > helpers.ROW_END16_MAX  # every segment reads the row pointers
    assert sizes["split64"].max() > 65536 > windows["split64"]       # a split dictionary: the per-pair path


@pytest.mark.parametrize("name,window,hints", CASES, ids=[f"{n}-{'own' if w is None else w}" for n, w, _ in CASES])
def test_one_field_grid_mode_is_the_documented_add_order_bit_for_bit(rg, scene, name, window, hints):
    from radar_processor_amd import _native
    lib = _native.load_library()
    s = scene(name)
    for order, gr in s.gridders.items():
        args32 = gr._stream_args(FILL)
        assert args32[1] == 0 and args32[4] == order and args32[13] == 1
        args64 = (_native.ptr(s.indptr64), 1) + tuple(args32[2:])
        for hint in hints:
            want = s.emu(hint)
            for args in (args32, args64):
                for table in (True, False):
                    buf = s.torch.full((s.n_vox + 2 * GUARD,), PREFILL, dtype=s.torch.float32, device=s.dev)
                    out = buf[GUARD:GUARD + s.n_vox].view(1, s.n_vox)
                    _native.check(lib.rg_csr_compact_apply_packed_f32_ex(
                        *args, _native.ptr(out), gr.window if window is None else window, 2000 + hint if hint else 0,
                        _native.ptr(gr.compact.row_end16) if table else 0, _native.stream_ptr()),
                        "rg_csr_compact_apply_packed_f32_ex")
                    where = (name, window, order, hint, args is args64, table)
                    assert _same_bits(out, want), where
                    assert not bool((out == PREFILL).any()), where
                    assert bool((buf[:GUARD] == PREFILL).all()) and bool((buf[-GUARD:] == PREFILL).all()), where
    if name == "gap130":
        rows = np.concatenate([np.arange(r0, r0 + n) for (_, _, r0, n, ch) in helpers.segments(SHAPE_130) if ch == 1])
        assert (s.emu(0)[:, rows] == FILL).all()
