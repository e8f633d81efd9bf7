"""Chains of entry points captured into a graph on inputs A and replayed on inputs B, with poisoned outputs and dirty
workspaces, through the raw C ABI (include/radargrid_hip.h: "no global mutable state: entry points are thread-safe per
stream"; INTEGRATION.md section 2: "nothing in the library allocates or synchronises, so the calls can be captured into a
hipGraph").  Scenes: tests/graph_replay_scenes.py; tests/test_graph_replay_scenes.py proves on the CPU that a replay which
reproduced A's result, or a key left in a workspace, cannot pass.

The replay gives B's result only if every launch and memset went to the given stream, nothing was read on the host or baked
into a launch argument from device data, and every scratch word is written inside the call before it is read.

The protocol of every chain (``_protocol``):
 1  static inputs, every output between canaries, workspaces of exactly the size the ``*_workspace_bytes`` function asks for;
 2  A in, the chain eagerly once (module load), checked against A's restatement -- a failure here is not capture's;
 3  the same enqueue captured with ``torch.cuda.graph`` as radar_processor_amd/pipeline.py does it: one stream, no branches;
    every entry point returns RG_OK while capturing;
 4  B in, every output poisoned, the workspaces as A's run left them; replay; B's restatement, canaries intact;
 5  the workspaces filled with 0xFF, then with 0x00, the outputs poisoned again; replay; B's restatement and the same bytes;
 6  once more with nothing changed (an in-place input restored): the same bytes;
 7  A back in; replay; A's restatement.

No comparison here is new.  Each is the rule of the family's own GPU test, named at the check: bits nearly everywhere; where a
family's contract is wider (one unit of q at a tie of exp10 in convection, one float32 step of a rain rate, the unspecified
order of the overlap pairs, the undecided pixels of the warp) the stage is compared exactly as that family's test compares it,
and the next stage is held to the restatement fed the device's own output of the stage before.

``CHAINED`` and ``EXCLUDED`` at the end name every entry point that takes a stream: in a chain, or excluded with its reason
(the probe, the steps of a geometry build, the three calls the pipeline's own replay tests capture);
tests/test_stream_contract_host.py holds the table complete."""
import ctypes
import threading

import numpy as np
import pytest

from oracle import radar_grid_oracle as oracle

import accumulation_oracle as ao
import closest_scenes as cls
import combine_scenes as cbs
import convection_oracle as co
import georef_oracle as go
import graph_replay_scenes as gs
import product_scenes as ps
import slab_scenes as sl
import test_gpu_columns as family_columns
import test_gpu_column_profile as family_profile
import test_gpu_components as family_components
import test_gpu_convection as family_convection
import test_gpu_motion as family_motion
import test_gpu_product_contracts as family_products
import test_gpu_warp as family_warp
import verification_oracle as vo
import warp_oracle as wo

pytestmark = pytest.mark.gpu
CANARY = 64                       # elements before and after every output
_PATTERN = {"uint8": 0xA5, "int16": -21555, "int32": -1234567, "int64": -1234567890123, "float32": -12345.5, "float64": -12345.5}
_STATE = {"broken": None}         # the first capture or replay that failed: nothing after it touches the device


@pytest.fixture(scope="module")
def env():
    import torch
    import radar_processor_amd as rg
    from radar_processor_amd import _native, georef, motion
    lib = rg.load_library()
    return dict(torch=torch, rg=rg, native=_native, georef=georef, motion=motion, lib=lib, dev=torch.device("cuda", 0))


def _c(ctype, values):
    return (ctype * max(len(values), 1))(*values)


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


class Chain:
    """The buffers of one chain and the calls on them.

    ``inputs``   name -> {"A": array, "B": array}: static device arrays, overwritten with a scene's by ``load``;
    ``in_place`` the same for arrays an entry point overwrites with its result: they lie between canaries like an output and
                 are restored from the scene before every run;
    ``outputs``  name -> (shape, dtype name);   ``workspaces``  name -> bytes, exactly what the library asks for;
    ``enqueue(chain, stream)`` calls the entry points on ``chain.t[name]`` and returns their statuses;
    ``check(chain, got, which)`` holds the outputs ``got`` (name -> array) to the restatement of scene ``which``;
    ``canonical(got)`` the outputs in the form two runs are compared in, byte for byte, where the contract leaves an order
                 open (default: as they are)."""

    def __init__(self, env, name, inputs, outputs, enqueue, check, workspaces=None, in_place=None, canonical=None):
        torch = env["torch"]
        self.env, self.name, self.inputs, self.in_place = env, name, inputs, in_place or {}
        self._enqueue, self._check, self.canonical = enqueue, check, canonical or (lambda got: got)
        self.t, self.guard, self.scratch = {}, {}, {}
        for key, pair in inputs.items():
            assert pair["A"].shape == pair["B"].shape and pair["A"].dtype == pair["B"].dtype, key
            self.t[key] = torch.empty(pair["A"].shape, dtype=getattr(torch, str(pair["A"].dtype)), device=env["dev"])
        shapes = dict(outputs)
        shapes.update({key: (pair["A"].shape, str(pair["A"].dtype)) for key, pair in self.in_place.items()})
        for key, (shape, dtype) in shapes.items():
            n = int(np.prod(shape))
            buf = torch.full((n + 2 * CANARY,), _PATTERN[dtype], dtype=getattr(torch, dtype), device=env["dev"])
            self.guard[key], self.t[key] = buf, buf[CANARY:CANARY + n].view(tuple(shape))
        for key, nbytes in (workspaces or {}).items():
            buf = torch.full((int(nbytes) + 2 * CANARY,), _PATTERN["uint8"], dtype=torch.uint8, device=env["dev"])
            self.guard[key], self.scratch[key] = buf, buf[CANARY:CANARY + int(nbytes)]
            self.t[key] = self.scratch[key]
        self.outputs = tuple(shapes)

    def load(self, which):
        torch = self.env["torch"]
        for key, pair in self.inputs.items():
            self.t[key].copy_(torch.from_numpy(np.array(pair[which])))
        self.restore(which)

    def restore(self, which):
        for key, pair in self.in_place.items():
            self.t[key].copy_(self.env["torch"].from_numpy(np.array(pair[which])))

    def poison(self):
        for key in self.outputs:
            if key not in self.in_place:
                self.t[key].fill_(_PATTERN[str(self.t[key].dtype).split(".")[-1]])

    def dirty(self, byte):
        for ws in self.scratch.values():
            ws.fill_(byte)

    def enqueue(self, stream):
        with self.env["torch"].cuda.device(self.env["dev"]):
            return self._enqueue(self, stream)

    def read(self):
        """Every output as an array, after the canaries of every guarded buffer were found intact."""
        for key, buf in self.guard.items():
            edge = self.env["torch"].cat([buf[:CANARY], buf[buf.numel() - CANARY:]]).cpu().numpy()
            assert (edge == edge.dtype.type(_PATTERN[str(edge.dtype)])).all(), f"{self.name}: canary of {key}"
        return {key: self.t[key].cpu().numpy() for key in self.outputs}

    def check(self, got, which):
        self._check(self, got, which)

    def inputs_unchanged(self, which):
        return all(self.t[key].cpu().numpy().tobytes() == pair[which].tobytes() for key, pair in self.inputs.items())


def _pair(chain, member):
    return {w: member(getattr(gs, chain)(w)) for w in gs.WHICH}


def _same_bytes(chain, a, b, what):
    a, b = chain.canonical(a), chain.canonical(b)
    for key in a:
        assert a[key].tobytes() == b[key].tobytes(), f"{what}: {key} differs"


def _guard_device(step):
    """Runs one step that talks to the device; a raise marks the module broken before it travels on."""
    try:
        return step()
    except BaseException as exc:
        _STATE["broken"] = f"{type(exc).__name__}: {exc}"
        raise


def _unbroken():
    if _STATE["broken"] is not None:
        pytest.fail(f"not run: a capture or replay of this module failed before ({_STATE['broken']})")


def _protocol(env, chain):
    torch, lib = env["torch"], env["lib"]
    _unbroken()
    # 2: A, eagerly: a wrong result here is the family's, not capture's, and stops nothing else; a fault stops everything
    chain.load("A")
    statuses = _guard_device(lambda: chain.enqueue(env["native"].stream_ptr()))
    assert all(s == 0 for s in statuses), (chain.name, statuses, lib.rg_last_error().decode())
    _guard_device(torch.cuda.synchronize)
    eager = chain.read()
    chain.check(eager, "A")
    chain.restore("A")
    torch.cuda.synchronize()

    # 3: capture
    def capture():
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph):
            captured = chain.enqueue(env["native"].stream_ptr())
        return graph, captured

    graph, statuses = _guard_device(capture)
    if any(s != 0 for s in statuses):
        _STATE["broken"] = f"{chain.name}: statuses {statuses} while capturing: {lib.rg_last_error().decode()}"
        pytest.fail(_STATE["broken"])

    def replay(which, dirty=None):
        chain.load(which)
        chain.poison()
        if dirty is not None:
            chain.dirty(dirty)

        def go():
            graph.replay()
            torch.cuda.synchronize()
        _guard_device(go)
        return chain.read()

    # 4: B, outputs poisoned, the workspaces as A left them
    on_b = replay("B")
    chain.check(on_b, "B")
    assert chain.inputs_unchanged("B"), chain.name
    # 5: dirty workspaces
    for byte in (0xFF, 0x00):
        again = replay("B", dirty=byte)
        chain.check(again, "B")                               # also what ``canonical`` leaves out of the byte comparison
        _same_bytes(chain, on_b, again, f"{chain.name}: workspaces filled with {byte:#04x}")
    # 6: nothing changed but an in-place input restored, and no poison: the outputs are overwritten where they stand
    chain.restore("B")
    _guard_device(lambda: (graph.replay(), torch.cuda.synchronize()))
    _same_bytes(chain, on_b, chain.read(), f"{chain.name}: replayed again")
    # 7: A again
    on_a = replay("A")
    chain.check(on_a, "A")
    _same_bytes(chain, eager, on_a, f"{chain.name}: the replay on A against the eager run on A")


# ---- verification ----------------------------------------------------------------------------------------------------------------
def _verification(env):
    nat, lib = env["native"], env["lib"]
    s = gs.verification("A")
    n, h, w = s.forecast.shape
    T, S = len(s.thresholds), len(s.scales)
    ends = gs.verification_ends(s)
    thr, scales = _c(ctypes.c_float, s.thresholds), _c(ctypes.c_int32, s.scales)

    def enqueue(c, stream):
        t, P = c.t, nat.ptr
        out = [lib.rg_contingency_f32(P(t["forecast"]), P(t["observed"]), P(t["mask"]), n, h, w, thr, T, P(t["counts"]), P(t["valid"]),
                                      stream),
               lib.rg_exceedance_sat_i32(P(t["forecast"]), P(t["observed"]), P(t["mask"]), n, h, w, thr, T, P(t["sat_f"]), stream),
               lib.rg_exceedance_sat_i32(P(t["observed"]), P(t["forecast"]), P(t["mask"]), n, h, w, thr, T, P(t["sat_o"]), stream),
               lib.rg_fss_sums_i32(P(t["sat_f"]), P(t["sat_o"]), n * T, h, w, scales, S, P(t["sums"]), stream)]
        return out + [lib.rg_box_fraction_f32(P(t["sat_f"]), n * T, h, w, scale, P(t["frac"][k]), stream) for k, scale in enumerate(ends)]

    def check(c, got, which):
        """tests/test_gpu_verification.py and test_gpu_nowcast_scale.py: integers equal, the fractions bit for bit."""
        want = gs.expected("verification", which)
        for key in ("counts", "valid", "sat_f", "sat_o", "sums"):
            assert np.array_equal(got[key], want[key]), f"verification on {which}: {int((got[key] != want[key]).sum())} of {key} differ"
        for k, scale in enumerate(ends):
            assert np.array_equal(_bits(got["frac"][k]), _bits(vo.box_fraction(want["sat_f"], scale))), (which, scale)

    return Chain(env, "verification", dict(forecast=_pair("verification", lambda s: s.forecast),
                                           observed=_pair("verification", lambda s: s.observed),
                                           mask=_pair("verification", lambda s: s.mask)),
                 dict(counts=((n, T, 3), "int64"), valid=((n,), "int64"), sat_f=((n, T, h, w), "int32"), sat_o=((n, T, h, w), "int32"),
                      sums=((n, T, S, 3), "int64"), frac=((2, n, T, h, w), "float32")), enqueue, check)


# ---- convection ------------------------------------------------------------------------------------------------------------------
def _convection(env):
    nat, lib = env["native"], env["lib"]
    s = gs.convection("A")
    shape = n, h, w = s.dbz.shape
    K = len(s.footprints)
    table_bytes, ws_bytes = int(lib.rg_echo_table_bytes(n, h, w)), int(lib.rg_convective_area_workspace_bytes(n, h, w, K))
    hw0, hw = _c(ctypes.c_int32, [0]), _c(ctypes.c_int32, s.hw)
    rows, ry = family_convection._area_tables(s.footprints)
    edges = _c(ctypes.c_double, s.edges)

    def enqueue(c, stream):
        t, P = c.t, nat.ptr
        return [lib.rg_echo_table_f32(P(t["dbz"]), P(t["mask"]), n, h, w, s.min_dbz, P(t["table"]), table_bytes, stream),
                lib.rg_disk_background(P(t["table"]), n, h, w, hw0, 0, P(t["q"]), P(t["flag"]), None, stream),
                lib.rg_disk_background(P(t["table"]), n, h, w, hw, len(s.hw) - 1, P(t["S"]), P(t["N"]), P(t["bkg"]), stream),
                lib.rg_convective_centres_f32(P(t["dbz"]), P(t["mask"]), P(t["bkg"]), n, h, w, s.min_dbz, s.intense, s.peak[0], s.peak[1],
                                              edges, len(s.edges) + 1, P(t["centres"]), stream),
                lib.rg_convective_area_u8(P(t["centres"]), P(t["dbz"]), P(t["mask"]), n, h, w, s.min_dbz, K, rows, ry, P(t["workspace"]),
                                          ws_bytes, P(t["classes"]), stream)]

    def check(c, got, which):
        """tests/test_gpu_convection.py, test_every_stage_equals_the_restatement_fed_the_stage_before, and on these main scenes
        the oracle end to end for the centres and the classes (test_main_scenes_equal_the_oracle_end_to_end)."""
        s, want = gs.convection(which), gs.expected("convection", which)
        assert int(np.abs(got["q"] - want["q"]).max()) <= 1, which
        assert np.array_equal(got["flag"], want["flag"]) and np.array_equal(got["q"] > 0, want["flag"] != 0)
        S, N, _ = co.background(s.dbz, s.hw, s.mask, s.min_dbz, q=got["q"])
        assert np.array_equal(got["S"], S) and np.array_equal(got["N"], N) and np.array_equal(N, want["N"]), which
        assert family_convection._within_one_step(got["bkg"], co.background_from_sums(got["S"], got["N"])), which
        assert np.array_equal(got["centres"], co.centres(s.dbz, got["bkg"], s.edges, s.mask, s.min_dbz, s.intense, s.peak)), which
        assert np.array_equal(got["classes"], co.area(got["centres"], s.dbz, s.footprints, s.mask, s.min_dbz)), which
        assert np.array_equal(got["centres"], want["centres"]) and np.array_equal(got["classes"], want["classes"]), which

    # the echo table is scratch between the calls of this chain: a workspace, left dirty and filled like one
    return Chain(env, "convection", dict(dbz=_pair("convection", lambda s: s.dbz), mask=_pair("convection", lambda s: s.mask)),
                 dict(q=(shape, "int64"), flag=(shape, "int32"), S=(shape, "int64"), N=(shape, "int32"), bkg=(shape, "float32"),
                      centres=(shape, "uint8"), classes=(shape, "uint8")), enqueue, check,
                 workspaces=dict(table=table_bytes, workspace=ws_bytes))


# ---- tracking --------------------------------------------------------------------------------------------------------------------
def _tracking(env):
    nat, lib = env["native"], env["lib"]
    n, h, w = gs.tracking("A").labels_prev.shape
    M, cells = gs.TRACK_MAX_PAIRS, gs.TRACK_CELLS
    need = int(lib.rg_cell_overlap_workspace_bytes(M))
    assert need == 12 * gs.overlap_capacity(M)
    lut = gs.track_lut()

    def enqueue(c, stream):
        t, P = c.t, nat.ptr
        return [lib.rg_cell_overlap_i32(P(t["labels_prev"]), P(t["ptr_prev"]), P(t["labels_next"]), P(t["ptr_next"]), n, h, w, M,
                                        P(t["rows"]), P(t["count"]), P(t["totals"]), P(t["table"]), need, stream),
                lib.rg_relabel_cells_i32(P(t["labels_prev"]), P(t["ptr_prev"]), n, h, w, P(t["lut"]), cells, P(t["relabel_prev"]), stream),
                lib.rg_relabel_cells_i32(P(t["relabel_next"]), P(t["ptr_next"]), n, h, w, P(t["lut"]), cells, P(t["relabel_next"]),
                                         stream)]                                    # in place

    def check(c, got, which):
        """tests/test_gpu_tracking.py, test_raw_abi_full_tables_canaries_and_a_short_workspace: the totals, the written
        triples as a set (their order is the table's), nothing written beyond them; the relabelled planes bit for bit."""
        want = gs.expected("tracking", which)
        k = len(want["pairs"])
        assert got["totals"].tolist() == [k, 0], (which, got["totals"].tolist())
        r, cnt = got["rows"].reshape(-1, 2), got["count"]
        assert (r[k:] == _PATTERN["int32"]).all() and (cnt[k:] == _PATTERN["int32"]).all(), which
        triples = {(int(a), int(b), int(v)) for (a, b), v in zip(r[:k], cnt[:k])}
        assert triples == {tuple(row) for row in want["pairs"].tolist()}, f"tracking on {which}: the pairs differ"
        for key in ("relabel_prev", "relabel_next"):
            assert got[key].tobytes() == want[key].tobytes(), (which, key)

    def canonical(got):
        """The pairs come out in the order of the table's slots, which the race for a slot decides: sorted, like the oracle's."""
        k = min(int(got["totals"][0]), M)
        triples = np.concatenate([got["rows"].reshape(-1, 2)[:k], got["count"][:k, None]], axis=1)
        out = {key: a for key, a in got.items() if key not in ("rows", "count")}
        out["pairs"] = triples[np.lexsort((triples[:, 1], triples[:, 0]))]
        out["beyond"] = np.concatenate([got["rows"][2 * k:], got["count"][k:]])
        return out

    return Chain(env, "tracking",
                 dict(labels_prev=_pair("tracking", lambda s: s.labels_prev), ptr_prev=_pair("tracking", lambda s: s.ptr_prev),
                      labels_next=_pair("tracking", lambda s: s.labels_next), ptr_next=_pair("tracking", lambda s: s.ptr_next),
                      lut=dict(A=lut, B=lut)),
                 dict(rows=((2 * M,), "int32"), count=((M,), "int32"), totals=((2,), "int32"), relabel_prev=((n, h, w), "int32")),
                 enqueue, check, workspaces=dict(table=need), in_place=dict(relabel_next=_pair("tracking", lambda s: s.labels_next)),
                 canonical=canonical)


# ---- raster ----------------------------------------------------------------------------------------------------------------------
def _raster(env):
    nat, lib = env["native"], env["lib"]
    name = gs.RASTER_SCENE
    s = wo.scene(name)
    H, W = s.raster.height, s.raster.width
    f, f8 = gs.RASTER_FACTOR, gs.RASTER_FACTOR_RGBA
    (oh, ow), (oh8, ow8) = wo.overview_shape(H, W, f), wo.overview_shape(H, W, f8)
    source, georef, raster = family_warp._structs(env, s)
    nan = float("nan")
    ny, nx = s.shape
    vmin, vmax, n_lut, _ = gs.COLORMAP
    lut = gs.colormap_lut()

    def enqueue(c, stream):
        t, P = c.t, nat.ptr
        return [lib.rg_warp_mercator_f32(P(t["planes"]), 3, source, georef, raster, 0, nan, P(t["near"]), stream),
                lib.rg_overview_f32(P(t["near"]), 3, H, W, f, 0, P(t["near_overview"]), stream),
                lib.rg_warp_mercator_f32(P(t["plane"]), 1, source, georef, raster, 1, nan, P(t["bilinear"]), stream),
                lib.rg_overview_f32(P(t["bilinear"]), 1, H, W, f, 1, P(t["bilinear_overview"]), stream),
                lib.rg_warp_mercator_rgba8(P(t["rgba_src"]), source, georef, raster, P(t["rgba"]), stream),
                lib.rg_overview_rgba8(P(t["rgba"]), H, W, f8, P(t["rgba_overview"]), stream),
                lib.rg_colormap_rgba(P(t["plane"]), 0, ny * nx, vmin, vmax, 0, 0.0, P(t["lut"]), n_lut, P(t["coloured"]), stream),
                lib.rg_warp_mercator_rgba8(P(t["coloured"]), source, georef, raster, P(t["coloured_warped"]), stream)]

    def check(c, got, which):
        """tests/test_gpu_warp.py: nearest samples by ``_assert_nearest`` (bits on every decided pixel, a candidate on an
        undecided one); bilinear values by the rule of ``warp_oracle.bilinear_differences`` (the oracle's fill set on decided
        pixels, every kept value within ``bilinear_allowance``); the overviews by test_overview_levels_against_the_restatement,
        each fed the device's own image of the stage before."""
        src = gs.raster(which)
        fx, fy, cc = wo.mapped(name)
        family_warp._assert_nearest(name, got["near"], src["planes"], np.float32(np.nan))
        assert np.array_equal(_bits(got["near_overview"]), _bits(wo.overview_nearest(got["near"], f))), which
        plane, bil = src["plane"][0], got["bilinear"][0]
        want, _, filled = wo.sample_bilinear(plane, fx, fy, cc, s.lattice, np.nan)
        decided = ~wo.undecided_bilinear(name, plane)
        assert decided.sum() >= (1.0 - wo.UNDECIDED_CAP) * decided.size and not (np.isnan(bil) != filled)[decided].any(), which
        both = decided & ~filled & ~np.isnan(bil)
        diff = np.abs(bil[both].astype(np.float64) - want[both].astype(np.float32).astype(np.float64))
        assert both.sum() > 1000 and (diff <= wo.bilinear_allowance(name, want[both], plane)).all(), which
        mean = wo.overview_average(got["bilinear"], f)
        assert np.array_equal(np.isnan(got["bilinear_overview"]), np.isnan(mean)), which
        live = ~np.isnan(mean)
        err = np.abs(got["bilinear_overview"][live].astype(np.float64) - mean[live].astype(np.float32))
        assert live.any() and (err <= wo.ulp_f32(mean[live])).all(), which
        family_warp._assert_nearest(name, got["rgba"], src["rgba"], 0)
        assert np.array_equal(got["rgba_overview"], wo.overview_nearest(got["rgba"], f8)), which
        # tests/test_gpu_product_contracts.py, test_colormap_explicit_tables: RGBA byte for byte; then onto the map like any image
        assert np.array_equal(got["coloured"], ps.colormap_reference(plane, vmin, vmax, lut)), which
        family_warp._assert_nearest(name, got["coloured_warped"], got["coloured"], 0)

    return Chain(env, "raster", dict(planes=_pair("raster", lambda d: d["planes"]), plane=_pair("raster", lambda d: d["plane"]),
                                     rgba_src=_pair("raster", lambda d: d["rgba"]), lut=dict(A=lut, B=lut)),
                 dict(near=((3, H, W), "float32"), near_overview=((3, oh, ow), "float32"), bilinear=((1, H, W), "float32"),
                      bilinear_overview=((1, oh, ow), "float32"), rgba=((H, W, 4), "uint8"), rgba_overview=((oh8, ow8, 4), "uint8"),
                      coloured=((ny, nx, 4), "uint8"), coloured_warped=((H, W, 4), "uint8")),
                 enqueue, check)


# ---- accumulation ----------------------------------------------------------------------------------------------------------------
def _accumulation(env):
    nat, lib = env["native"], env["lib"]
    s = gs.accumulation("A")
    shape = n, h, w = s.dbz_prev.shape
    p, q = ao.zr_constants(*gs.ZR[:2])
    min_dbz, max_dbz = gs.ZR[2:]
    restated = {}

    def enqueue(c, stream):
        t, P = c.t, nat.ptr
        out = [lib.rg_rain_rate_f32(P(t["dbz_" + k]), None, n, h, w, p, q, min_dbz, max_dbz, P(t["rate_" + k]), stream)
               for k in ("prev", "next")]
        for par, key in ((s.bilinear, "bilinear"), (s.nearest, "nearest")):
            out.append(lib.rg_accumulate_advected_f32(P(t["rate_prev"]), P(t["rate_next"]), n, h, w, P(t["motion"]),
                                                      nat.MotionLattice(*par.lattice), par.hours, par.n_steps, par.substeps,
                                                      env["motion"].ADVECT_METHODS[par.method], par.min_steps, par.fill,
                                                      P(t["depth_" + key]), P(t["steps_" + key]), stream))
        return out

    def check(c, got, which):
        """tests/test_gpu_accumulation.py: the rate's classes exact and a wet value the restatement's float32 or its
        neighbour (test_rain_rate_classes_are_exact_and_values_within_one_float32_step); depth and step counts bit for bit
        (test_accumulation_equals_the_restatement_bit_for_bit), the restatement fed the device's own rates."""
        sc, want = gs.accumulation(which), gs.expected("accumulation", which)
        for k, dbz in (("rate_prev", sc.dbz_prev), ("rate_next", sc.dbz_next)):
            rate = got[k]
            none = np.isnan(dbz)
            dry = ~none & ~(dbz >= np.float32(min_dbz))
            wet = ~none & ~dry
            assert (_bits(rate)[none] == ao.NAN_BITS).all() and np.array_equal(np.isnan(rate), none), (which, k)
            assert (_bits(rate)[dry] == 0).all() and wet.any() and (rate[wet] > 0.0).all(), (which, k)
            steps = np.abs(family_motion._ordered(rate[wet]) - family_motion._ordered(want[k][wet]))
            assert (steps <= 1).all(), f"{which} / {k}: {int((steps > 1).sum())} values lie more than one float32 step off"
        key = got["rate_prev"].tobytes() + got["rate_next"].tobytes()
        if key not in restated:
            restated[key] = gs.accumulation_from_rates(sc, got["rate_prev"], got["rate_next"])
        for acc, name in zip(restated[key], ("bilinear", "nearest")):
            assert np.array_equal(got["steps_" + name], acc.steps), (which, name)
            assert np.array_equal(_bits(got["depth_" + name]), _bits(acc.out)), \
                f"{which} / {name}: {int((_bits(got['depth_' + name]) != _bits(acc.out)).sum())} values differ"

    return Chain(env, "accumulation", dict(dbz_prev=_pair("accumulation", lambda a: a.dbz_prev),
                                           dbz_next=_pair("accumulation", lambda a: a.dbz_next),
                                           motion=_pair("accumulation", lambda a: a.motion)),
                 dict(rate_prev=(shape, "float32"), rate_next=(shape, "float32"), depth_bilinear=(shape, "float32"),
                      steps_bilinear=(shape, "uint8"), depth_nearest=(shape, "float32"), steps_nearest=(shape, "uint8")), enqueue, check)


# ---- motion ----------------------------------------------------------------------------------------------------------------------
def _motion(env):
    nat, lib = env["native"], env["lib"]
    import motion_scenes as ms
    s = gs.motion("A")
    h, w = s.prev.shape
    nby, nbx = (h - s.B) // s.S + 1, (w - s.B) // s.S + 1
    lat = gs.motion_field("A")[1]
    lo, inv = float(np.float32(ms.LO)), float(np.float32(254.0 / (ms.HI - ms.LO)))
    leads = _c(ctypes.c_double, gs.ADVECT_LEADS)
    L = len(gs.ADVECT_LEADS)

    def enqueue(c, stream):
        t, P = c.t, nat.ptr
        out = [lib.rg_motion_quantize_f32(P(t[k]), None, 1, h, w, lo, inv, P(t["q_" + k]), stream) for k in ("prev", "next")]
        out.append(lib.rg_block_match_u8(P(t["q_prev"]), P(t["q_next"]), 1, h, w, s.B, s.S, s.R, s.B * s.B // 8, P(t["disp"]),
                                         P(t["motion"]), P(t["score"]), stream))
        for method in ("nearest", "bilinear"):
            out.append(lib.rg_advect_f32(P(t["prev"]), 1, h, w, P(t["field"]), nat.MotionLattice(*lat), leads, L, gs.ADVECT_SUBSTEPS,
                                         env["motion"].ADVECT_METHODS[method], gs.ADVECT_FILL, P(t["advect_" + method]), stream))
        return out

    def check(c, got, which):
        """tests/test_gpu_motion.py: levels and displacements equal, score and motion the float32 of the restatement's
        float64 or its neighbour (``_assert_rounded``), advected planes bit for bit."""
        want = gs.expected("motion", which)
        match = gs.motion_match(which)[2]
        for key in ("q_prev", "q_next", "disp"):
            assert np.array_equal(got[key], want[key]), (which, key)
        family_motion._assert_rounded(got["score"], match.score, f"motion on {which}: score")
        family_motion._assert_rounded(got["motion"], match.motion, f"motion on {which}: motion")
        for method in ("nearest", "bilinear"):
            key = "advect_" + method
            assert np.array_equal(_bits(got[key]), _bits(want[key])), f"{which} / {key}: {int((_bits(got[key]) != _bits(want[key])).sum())}"

    return Chain(env, "motion", dict(prev=_pair("motion", lambda m: m.prev[None]), next=_pair("motion", lambda m: m.next[None]),
                                     field={x: gs.motion_field(x)[0] for x in gs.WHICH}),
                 dict(q_prev=((1, h, w), "uint8"), q_next=((1, h, w), "uint8"), disp=((1, nby, nbx, 2), "int16"),
                      motion=((1, nby, nbx, 2), "float32"), score=((1, nby, nbx), "float32"),
                      advect_nearest=((L, 1, h, w), "float32"), advect_bilinear=((L, 1, h, w), "float32")), enqueue, check)


# ---- cells -----------------------------------------------------------------------------------------------------------------------
def _cells(env):
    nat, lib = env["native"], env["lib"]
    s = gs.cells("A")
    shape = n, h, w = s.planes.shape
    need = int(lib.rg_components_workspace_bytes(n, h, w))
    bound = gs.CELLS_BOUND
    per_cell = dict(area=((bound,), "int32"), bbox=((bound, 4), "int32"), sum_yx=((bound, 2), "int64"), vmax=((bound,), "float32"),
                    argmax=((bound,), "int32"), vsum=((bound,), "float64"))

    def enqueue(c, stream):
        t, P = c.t, nat.ptr
        return [lib.rg_label_components_f32(P(t["planes"]), P(t["mask"]), n, h, w, s.lo, s.hi, gs.CELLS_CONNECTIVITY, 0, P(t["labels"]),
                                            P(t["cell_ptr"]), P(t["workspace"]), need, stream),
                lib.rg_component_stats_f32(P(t["planes"]), P(t["labels"]), P(t["cell_ptr"]), n, h, w, bound,
                                           *(P(t[k]) for k in ("area", "bbox", "sum_yx", "vmax", "argmax", "vsum")), stream),
                lib.rg_despeckle_select_f32(P(t["planes"]), P(t["labels"]), P(t["cell_ptr"]), P(t["area"]), n, h, w, gs.CELLS_MIN_SIZE,
                                            gs.CELLS_FILL, P(t["despeckled"]), P(t["removed"]), stream)]

    def check(c, got, which):
        """tests/test_gpu_components.py: labels and cell_ptr equal, the table by ``_check_table`` (exact but for vsum, which is
        held to the worst-case bound of a float64 sum in any order), the despeckled planes and the mask bytewise.  n_cells is
        a bound that covers both scenes: the rows of the cells that exist are the contract's, the rows beyond are nobody's.
        With that bound the table and the despeckling need no count on the host, so the three calls are ONE graph: the longest
        run without a host read.  ``vsum`` has no scratch behind it (atomic adds into the output itself, cleared by the
        call's own init kernel); it is held to its bound on every replay, the dirty ones included, and left out of the byte
        comparison only."""
        want = gs.expected("cells", which)
        _, _, table = gs.cells_reference(which)
        assert np.array_equal(got["cell_ptr"], want["cell_ptr"]) and np.array_equal(got["labels"], want["labels"]), which
        rows = int(want["cell_ptr"][-1])
        family_components._check_table({k: got[k][:rows] for k in per_cell}, table, f"cells on {which}")
        assert got["despeckled"].tobytes() == want["despeckled"].tobytes() and got["removed"].tobytes() == want["removed"].tobytes(), which

    def canonical(got):
        """The rows of the cells that exist, and not vsum: the one output that depends on the order of arrival."""
        rows = int(got["cell_ptr"][-1])
        return {k: (a[:rows] if k in per_cell else a) for k, a in got.items() if k != "vsum"}

    outputs = dict(labels=(shape, "int32"), cell_ptr=((n + 1,), "int32"), despeckled=(shape, "float32"), removed=(shape, "uint8"))
    outputs.update(per_cell)
    return Chain(env, "cells", dict(planes=_pair("cells", lambda c: c.planes), mask=_pair("cells", lambda c: c.mask)), outputs, enqueue,
                 check, workspaces=dict(workspace=need), canonical=canonical)


# ---- products --------------------------------------------------------------------------------------------------------------------
def _products(env):
    nat, lib = env["native"], env["lib"]
    s = ps.ppi_scene(gs.PRODUCTS_SCENE)
    nz, ny, nx = s.nz, s.ny, s.nx
    n = ny * nx
    scalars = ps.ppi_scalars(s, True)
    thr, nt = _c(ctypes.c_double, gs.PROFILE_THRESHOLDS), len(gs.PROFILE_THRESHOLDS)
    sin_elev, two_re = gs.COLLAPSE
    flags, lo, hi, fill = gs.GRID_FILTER
    tests = (nat.PlaneTest * len(gs.PLANE_TESTS))()

    def enqueue(c, stream):
        t, P = c.t, nat.ptr
        for k, (plane, t_lo, t_hi, t_flags) in enumerate(gs.PLANE_TESTS):
            tests[k].plane = P(t["top"][0]) if plane == "top" else None
            tests[k].lo, tests[k].hi, tests[k].flags = t_lo, t_hi, t_flags
        return [lib.rg_column_profile_f32(P(t["grid"]), nz, n, 0, nz - 1, P(t["z"]), thr, nt, 1, P(t["top"]), P(t["base"]),
                                          gs.PROFILE_MAX_DBZ, P(t["vil"]), stream),
                lib.rg_elevation_ppi_f32(P(t["grid"]), P(t["xc"]), P(t["yc"]), nz, ny, nx, *scalars, P(t["ppi_stored"]), stream),
                lib.rg_elevation_ppi_plan_f32(P(t["xc"]), P(t["yc"]), nz, ny, nx, *scalars, P(t["sel"]), P(t["w_hi"]), stream),
                lib.rg_elevation_ppi_finish_f32(P(t["sel"]), P(t["w_hi"]), P(t["samples"]), n, 1, P(t["ppi"]), stream),
                lib.rg_collapse_ppi_f32(P(t["grid"]), P(t["x"]), P(t["y"]), P(t["z"]), nz, ny, nx, sin_elev, two_re, P(t["collapsed"]),
                                        P(t["level"]), stream),
                lib.rg_plane_filter_f32(P(t["collapsed"]), None, n, tests, len(gs.PLANE_TESTS), P(t["kept"]), P(t["kept_mask"]), stream),
                lib.rg_grid_filter(P(t["grid"]), 0, nz * n, flags, lo, hi, None, fill, P(t["filtered"]), stream),
                lib.rg_nan_minmax(P(t["filtered"]), 0, nz * n, 1, fill, P(t["minmax_ws"]), P(t["minmax"]), stream)]

    def check(c, got, which):
        """tests/test_gpu_column_profile.py: echo top and base bit for bit (``assert_bits``), VIL within one float32 ulp
        (``assert_vil``).  tests/test_gpu_product_contracts.py: the PPI's plan words equal and its weights, the stored-grid
        plane, the finished plane and the collapsed plane the restatement's bits or NaN on both sides (``_same``); the plane
        filter NaN where masked, the source's bits elsewhere, the mask byte for byte; the grid filter by ``_same``; the four
        numbers of the min / max pass equal.  The filter and the min / max are fed the device's own planes."""
        want, grid = gs.expected("products", which), gs.products(which)["grid"]
        same = family_products._same
        family_profile.assert_bits(got["top"], want["top"], ("replay top", which))
        family_profile.assert_bits(got["base"], want["base"], ("replay base", which))
        family_profile.assert_vil(got["vil"], want["vil"], ("replay vil", which))
        assert np.array_equal(got["sel"], want["sel"]), which
        same(got["w_hi"], want["w_hi"], f"w_hi on {which}")
        same(got["ppi_stored"], want["ppi"], f"rg_elevation_ppi_f32 on {which}")
        assert np.isnan(got["ppi"][got["sel"] == nat.RG_PPI_SEL_NONE]).all(), which
        same(got["ppi"], got["ppi_stored"], f"rg_elevation_ppi_finish_f32 on {which}")
        same(got["collapsed"], want["collapsed"], f"rg_collapse_ppi_f32 on {which}")
        assert np.array_equal(got["level"], want["level"]), which
        masked, _ = ps.plane_filter_reference(got["collapsed"], None, gs.products_tests(got["collapsed"], got["top"][0]))
        assert 0 < masked.sum() < masked.size and np.isnan(got["kept"][masked]).all(), which
        assert (ps.bits(got["kept"])[~masked] == ps.bits(got["collapsed"])[~masked]).all(), which
        assert np.array_equal(got["kept_mask"], masked.astype(np.uint8)), which
        same(got["filtered"], ps.grid_filter_reference(grid, flags, lo, hi, None, fill), f"rg_grid_filter on {which}")
        assert np.array_equal(got["minmax"], ps.minmax_reference(got["filtered"], fill)), (which, got["minmax"].tolist())

    both = lambda a: dict(A=np.ascontiguousarray(a), B=np.ascontiguousarray(a))
    return Chain(env, "products",
                 dict(grid=_pair("products", lambda d: d["grid"]), samples=_pair("products", lambda d: d["samples"]), xc=both(s.xc),
                      yc=both(s.yc), x=both(s.xc.astype(np.float64)), y=both(s.yc.astype(np.float64)), z=both(gs.products_levels())),
                 dict(top=((nt, n), "float32"), base=((nt, n), "float32"), vil=((n,), "float32"), sel=((n,), "int32"),
                      w_hi=((n,), "float64"), ppi=((n,), "float64"), ppi_stored=((n,), "float64"), collapsed=((n,), "float32"),
                      level=((n,), "int32"), kept=((n,), "float32"), kept_mask=((n,), "uint8"), filtered=((nz, ny, nx), "float32"),
                      minmax=((4,), "float64")),
                 enqueue, check, workspaces=dict(minmax_ws=nat.RG_MINMAX_WORKSPACE_BYTES))


# ---- georef ----------------------------------------------------------------------------------------------------------------------
def _georef(env):
    nat, lib = env["native"], env["lib"]
    s = go.scene(gs.GEOREF_SCENE)
    n = s.x.size
    ny, nx = gs.NODE_SHAPE
    placing, nodes = env["georef"].make_georef(s.radar, s.origin), env["georef"].make_georef(s.origin, s.origin)

    def enqueue(c, stream):
        t, P = c.t, nat.ptr
        return [lib.rg_gates_to_frame_f32(P(t["x"]), P(t["y"]), n, placing, P(t["x_frame"]), P(t["y_frame"]), stream),
                lib.rg_gates_to_frame_f32(P(t["x_in_place"]), P(t["y_in_place"]), n, placing, P(t["x_in_place"]), P(t["y_in_place"]),
                                          stream),
                lib.rg_frame_to_lonlat_f64(P(t["xc"]), P(t["yc"]), ny, nx, nodes, P(t["lon"]), P(t["lat"]), stream)]

    def check(c, got, which):
        """tests/test_gpu_georef.py: a placed gate within ``ulp_f32(want) + KERNEL_FLOOR_M`` of the float64 restatement and
        NaN where the gate is not finite (``georef_oracle.kernel_differences``), in place the same bits as out of place
        (test_canaries_and_in_place_at_every_length); the nodes within 1e-10 degrees of longitude and 1e-11 of latitude of the
        host map (test_node_lonlat_against_40_digits)."""
        d, want = gs.georef(which), gs.expected("georef", which)
        fin = np.isfinite(d["x"]) & np.isfinite(d["y"])
        for key, w in zip(("x_frame", "y_frame"), gs.georef_placed(which)):
            assert np.isnan(got[key][~fin]).all() and fin.sum() > 4000, (which, key)
            diff = np.abs(got[key][fin].astype(np.float64) - w[fin].astype(np.float32).astype(np.float64))
            assert (diff <= go.ulp_f32(w[fin]) + go.KERNEL_FLOOR_M).all(), (which, key, float(diff.max()))
        assert got["x_in_place"].tobytes() == got["x_frame"].tobytes() and got["y_in_place"].tobytes() == got["y_frame"].tobytes(), which
        d_lon = np.abs(got["lon"] - want["lon"])
        assert np.minimum(d_lon, 360.0 - d_lon).max() < 1e-10 and np.abs(got["lat"] - want["lat"]).max() < 1e-11, which

    return Chain(env, "georef", dict(x=_pair("georef", lambda d: d["x"]), y=_pair("georef", lambda d: d["y"]),
                                     xc=_pair("georef", lambda d: d["xc"]), yc=_pair("georef", lambda d: d["yc"])),
                 dict(x_frame=((n,), "float32"), y_frame=((n,), "float32"), lon=((ny, nx), "float64"), lat=((ny, nx), "float64")),
                 enqueue, check, in_place=dict(x_in_place=_pair("georef", lambda d: d["x"]), y_in_place=_pair("georef", lambda d: d["y"])))


# ---- gridding --------------------------------------------------------------------------------------------------------------------
def _gridding(env):
    nat, lib, rg = env["native"], env["lib"], env["rg"]
    s = cls.scene(gs.GRIDDING_SCENE)
    nz, ny, nx = s.shape
    nf, stride, n_gates, n_points = gs.GRIDDING_FIELDS, 4, s.n_gates, gs.SECTION_POINTS
    # the search structure is geometry: built once, outside every graph (its build reads counts back on the host)
    search = rg.RoiSearch(s.gx, s.gy, s.gz, s.shape, s.limits, device=env["dev"], **s.search_kw())
    env["torch"].cuda.synchronize()
    closest, weighted = nat.WEIGHTINGS["closest"], nat.WEIGHTINGS[gs.GRIDDING_WEIGHTING]
    nan = float("nan")

    def enqueue(c, stream):
        t, P = c.t, nat.ptr
        fptrs = (ctypes.c_void_p * nf)(*[P(t[f"f{k}"]) for k in range(nf)])
        mptrs = (ctypes.c_void_p * nf)(P(t["m0"]), None, P(t["m2"]))
        head = search.search_args()
        return [lib.rg_pack_fields_f32(nf, fptrs, mptrs, None, n_gates, stride, P(t["packed"]), stream),
                lib.rg_roi_grid_f32(*head, closest, P(t["packed"]), nf, stride, nan, P(t["closest"]), stream),
                lib.rg_roi_grid_f32(*head, weighted, P(t["packed"]), nf, stride, nan, P(t["weighted"]), stream),
                lib.rg_roi_section_f32(*head[:3], P(t["xs"]), P(t["ys"]), head[5], nz, n_points, s.min_radius, s.beam_factor, weighted,
                                       P(t["packed"]), nf, stride, nan, P(t["section"]), stream)]

    def check(c, got, which):
        """tests/test_gpu_closest.py: the closest-gate grid holds the bits of the gate ``oracle.closest_gate_choice`` names on
        every voxel of every field, the fill where it names none.  tests/test_gpu_mean_bounds.py and tests/test_gpu_section.py:
        the weighted grid and the section lie within ``oracle.mean_error_bound`` (``oracle.DELTA_K2``) of the float64 mean of
        the brute-force neighbours, filled exactly where it is (``oracle.bound_ratio <= 1``)."""
        want = gs.expected("gridding", which)
        assert np.array_equal(_bits(got["closest"]), _bits(want["closest"])), f"gridding on {which}: closest"
        delta = oracle.DELTA_K2[gs.GRIDDING_WEIGHTING]
        for k in range(nf):
            assert oracle.bound_ratio(got["weighted"][k], gs.gridding_stats(which, k), delta).max(initial=0.0) <= 1.0, (which, k)
            assert oracle.bound_ratio(got["section"][k], gs.section_stats(which, k), delta).max(initial=0.0) <= 1.0, (which, k)

    inputs = {key: _pair("gridding", lambda d, key=key: d[key]) for key in ("f0", "f1", "f2", "m0", "m2")}
    inputs["xs"] = {w: gs.section_points(w)[0] for w in gs.WHICH}
    inputs["ys"] = {w: gs.section_points(w)[1] for w in gs.WHICH}
    # the packed fields are scratch between the calls of this chain: a workspace, left dirty and filled like one
    return Chain(env, "gridding", inputs, dict(closest=((nf, nz, ny, nx), "float32"), weighted=((nf, nz, ny, nx), "float32"),
                                              section=((nf, nz, n_points), "float32")),
                 enqueue, check, workspaces=dict(packed=n_gates * stride * 4))


# ---- columns ---------------------------------------------------------------------------------------------------------------------
def _columns(env):
    nat, lib, rg, torch = env["native"], env["lib"], env["rg"], env["torch"]
    nz, ny, nx = shape = tuple(sl.WIDE_SHAPE)
    nf, pieces = gs.COLUMNS_FIELDS, gs.COLUMNS_PIECES
    n_vox = nz * ny * nx
    n_gates = int(gs.columns("A")["f0"].size)
    # the CSR, its compact copy with the packed records and the workgroup order are geometry: built once, outside every graph
    geom = rg.GridGeometry(shape, sl.WIDE_LIMITS, *gs.columns_csr(), toa=17000.0)
    csr = geom.device_csr(env["dev"])
    compact = geom.device_compact(env["dev"])
    assert compact is not None and compact.ensure_packed(csr) and compact.local_idx is not None
    g = family_columns._gridder(geom, compact, n_gates, nf, env["dev"])
    assert g.has_columns_kernel
    _, order = g._column_plan(pieces)
    torch.cuda.synchronize()
    stride, window, row_end16 = g.stride, g.window, nat.ptr(compact.row_end16)
    ws_columns = int(lib.rg_csr_columns_workspace_bytes(ny, nx, nf, pieces))
    ws_planes = int(lib.rg_csr_planes_workspace_bytes(ny, nx, nf, pieces, 1, 1))
    assert ws_columns > 0 and ws_planes > 0
    nan = float("nan")
    reqs = []

    def enqueue(c, stream):
        t, P = c.t, nat.ptr
        g.packed = t["packed"]                                               # the 17 leading arguments read the chain's buffer
        lead = g._stream_args(nan)
        fptrs = (ctypes.c_void_p * nf)(*[P(t[f"f{k}"]) for k in range(nf)])
        mptrs = (ctypes.c_void_p * nf)(*[P(t[f"m{k}"]) for k in range(nf)])
        del reqs[:]
        for ex in ("", "_ex"):
            reqs.append(nat.PlaneRequest(out=P(t["planes_out" + ex]), col_max=P(t["planes_max" + ex]), col_arg=P(t["planes_arg" + ex]),
                                         col_min=P(t["planes_min" + ex]), col_lo=0, col_hi=nz - 1))
        tail = lambda ws, nbytes: (window, pieces, P(order), P(t[ws]), nbytes, 0)
        return [lib.rg_pack_fields_f32(nf, fptrs, mptrs, None, n_gates, stride, P(t["packed"]), stream),
                lib.rg_csr_apply_f32_ex(P(csr.indptr), int(csr.is_i64), P(csr.gate_indices), P(csr.weights), n_vox, csr.n_pairs, nx,
                                        P(t["packed"]), nf, stride, n_gates, nan, P(t["k1"]), 0, stream),
                lib.rg_csr_compact_apply_f32(P(csr.indptr), int(csr.is_i64), P(compact.local_idx), P(csr.weights), P(compact.dict_ptr),
                                             P(compact.dict), n_vox, csr.n_pairs, nx, ny, P(t["packed"]), nf, stride, n_gates, nan,
                                             P(t["tile"]), window, 0, stream),
                lib.rg_csr_compact_apply_packed_f32(*lead, P(t["rowwise"]), window, 0, stream),
                lib.rg_csr_compact_apply_packed_f32_ex(*lead, P(t["rowwise_ex"]), window, 0, row_end16, stream),
                lib.rg_csr_compact_apply_columns_f32(*lead, P(t["columns_out"]), None, 0, 0, P(t["columns_max"]), P(t["columns_arg"]), 0,
                                                     nz - 1, *tail("ws_columns", ws_columns), stream),
                lib.rg_csr_compact_apply_columns_f32_ex(*lead, P(t["columns_out_ex"]), None, 0, 0, P(t["columns_max_ex"]),
                                                        P(t["columns_arg_ex"]), 0, nz - 1, *tail("ws_columns", ws_columns), row_end16,
                                                        stream),
                lib.rg_csr_compact_apply_planes_f32(*lead, ctypes.byref(reqs[0]), *tail("ws_planes", ws_planes), stream),
                lib.rg_csr_compact_apply_planes_f32_ex(*lead, ctypes.byref(reqs[1]), *tail("ws_planes", ws_planes), row_end16, stream)]

    def same(got, want, what):
        """NaN in the same voxels and the same bits elsewhere (tests/test_gpu_columns.py)."""
        live = ~np.isnan(want)
        assert np.array_equal(np.isnan(got), ~live) and np.array_equal(_bits(got)[live], _bits(want)[live]), what

    def check(c, got, which):
        """tests/test_gpu_tile_order.py: K1 and the tile kernel over the compact copy bit for bit with
        ``oracle.csr_apply_tile_order``.  tests/test_gpu_columns.py and tests/test_gpu_plane_products.py: the row-wise kernel
        bit for bit with ``oracle.csr_apply_rowwise_order``; the grids of the column and plane modes the same bits for any
        number of level pieces; their COLMAX, first argmax and COLMIN bit for bit with the oracle on that grid."""
        want = gs.expected("columns", which)
        for key in ("k1", "tile"):
            same(got[key].reshape(want["tile"].shape), want["tile"], (which, key))
        for key in ("rowwise", "rowwise_ex", "columns_out", "columns_out_ex", "planes_out", "planes_out_ex"):
            same(got[key].reshape(want["rowwise"].shape), want["rowwise"], (which, key))
        for mode in ("columns", "planes"):
            for ex in ("", "_ex"):
                same(got[f"{mode}_max{ex}"], want["col_max"], (which, mode, ex, "max"))
                assert np.array_equal(got[f"{mode}_arg{ex}"], want["col_arg"]), (which, mode, ex, "arg")
        for ex in ("", "_ex"):
            same(got["planes_min" + ex], want["col_min"], (which, ex, "min"))

    grid, plane, arg = ((nf, n_vox), "float32"), ((nf, ny, nx), "float32"), ((nf, ny, nx), "int32")
    outputs = dict(k1=grid, tile=grid)
    for ex in ("", "_ex"):
        outputs.update({"rowwise" + ex: grid, "columns_out" + ex: grid, "columns_max" + ex: plane, "columns_arg" + ex: arg,
                        "planes_out" + ex: grid, "planes_max" + ex: plane, "planes_arg" + ex: arg, "planes_min" + ex: plane})
    inputs = {key: _pair("columns", lambda d, key=key: d[key]) for key in ("f0", "f1", "m0", "m1")}
    chain = Chain(env, "columns", inputs, outputs, enqueue, check,
                  workspaces=dict(packed=n_gates * stride * 4, ws_columns=ws_columns, ws_planes=ws_planes))
    chain.keep = (geom, g)
    return chain


# ---- mosaic ----------------------------------------------------------------------------------------------------------------------
def _mosaic(env):
    nat, lib, torch = env["native"], env["lib"], env["torch"]
    from radar_processor_amd.mosaic import MosaicSearch, mosaic_section_points
    scene, sel = cbs.tie_scene(), list(gs.MOSAIC_RADARS)
    nz, ny, nx = scene.shape
    xs, ys = gs.mosaic_path()
    n_points, nf, stride = len(xs), 2, 2
    # the per-radar searches and the points in every radar's frame are geometry: built once, outside every graph
    search = MosaicSearch(scene.radars(), scene.shape, scene.limits, scene.min_radius, scene.beam_factor, scene.toa, device=env["dev"])
    offsets = scene.offsets(sel)
    n_total = int(offsets[-1])
    all_points = mosaic_section_points(search, xs, ys)
    points = [tuple(torch.from_numpy(a).to(env["dev"]) for a in all_points[r]) for r in sel]
    table, section_table = search.table(sel, offsets[:-1]), search.section_table(sel, offsets[:-1], points)
    torch.cuda.synchronize()
    weighting, combine = nat.WEIGHTINGS[gs.MOSAIC_WEIGHTING], nat.COMBINES[gs.MOSAIC_COMBINE]
    nan = float("nan")

    def enqueue(c, stream):
        t, P = c.t, nat.ptr
        fptrs = (ctypes.c_void_p * nf)(P(t["f0"]), P(t["f1"]))
        mptrs = (ctypes.c_void_p * nf)(P(t["m0"]), P(t["m1"]))
        lattice = (table, len(sel), nz, ny, nx, search.min_radius, search.beam_factor, weighting, P(t["packed"]), nf, stride, n_total, nan)
        path = (section_table, len(sel), nz, n_points, search.min_radius, search.beam_factor, weighting, P(t["packed"]), nf, stride,
                n_total, nan)
        return [lib.rg_pack_fields_f32(nf, fptrs, mptrs, P(t["shared"]), n_total, stride, P(t["packed"]), stream),
                lib.rg_roi_grid_mosaic_f32(*lattice, P(t["mean"]), stream),
                lib.rg_roi_grid_mosaic_combine_f32(*lattice, P(t["nearest"]), combine, P(t["radar"]), stream),
                lib.rg_roi_section_mosaic_f32(*path, P(t["section_mean"]), stream),
                lib.rg_roi_section_mosaic_combine_f32(*path, P(t["section_nearest"]), combine, P(t["section_radar"]), stream)]

    def check(c, got, which):
        """tests/test_gpu_mosaic.py and tests/test_gpu_mosaic_section.py: the joint mean within ``oracle.mean_error_bound``
        (``oracle.DELTA_K2``) of the float64 mean over the union of both radars' brute-force neighbours, filled exactly where
        it is.  tests/test_gpu_mosaic_combine.py and tests/test_gpu_mosaic_section_combine.py
        (test_values_lie_within_the_bound_of_the_named_radars_float64_mean): the radar map is the nearest radar with a live
        neighbour, the earlier table position on equal distances, 255 and the fill where none has one; every value within
        the bound of the named radar's own float64 mean."""
        delta = oracle.DELTA_K2[gs.MOSAIC_WEIGHTING]
        for section in (False, True):
            tag = "section_" if section else ""
            for slot in range(nf):
                what = (which, tag, slot)
                assert oracle.bound_ratio(got[tag + "mean"][slot], gs.mosaic_stats(which, slot, section), delta).max(initial=0.0) <= 1.0, what
                who, _ = gs.mosaic_nearest(which, slot, section)
                radar, value = got[tag + "radar"][slot].ravel(), got[tag + "nearest"][slot].ravel()
                assert np.array_equal(radar, who) and np.array_equal(np.isnan(value), radar == cbs.NO_RADAR), what
                for position in range(len(sel)):
                    at = radar == position
                    stats = {key: np.asarray(v)[at] for key, v in gs.mosaic_stats(which, slot, section, position).items()}
                    assert at.any() and np.isfinite(stats["m"]).all(), what
                    assert oracle.bound_ratio(value[at], stats, delta).max(initial=0.0) <= 1.0, what + (position,)

    inputs = {key: _pair("mosaic", lambda d, key=key: d[key]) for key in ("f0", "f1", "m0", "m1", "shared")}
    lattice, path = (nf, nz, ny, nx), (nf, nz, n_points)
    chain = Chain(env, "mosaic", inputs,
                  dict(mean=(lattice, "float32"), nearest=(lattice, "float32"), radar=(lattice, "uint8"),
                       section_mean=(path, "float32"), section_nearest=(path, "float32"), section_radar=(path, "uint8")),
                  enqueue, check, workspaces=dict(packed=n_total * stride * 4))
    chain.keep = (search, points, table, section_table)
    return chain


# ---- prologue --------------------------------------------------------------------------------------------------------------------
def _prologue(env):
    nat, lib = env["native"], env["lib"]
    d = gs.prologue("A")
    n_rays, n_gates = d["az"].size, d["ranges"].size
    n = n_rays * n_gates

    def enqueue(c, stream):
        t, P = c.t, nat.ptr
        return [lib.rg_antenna_to_cartesian_f32(P(t["ranges"]), n_gates, P(t["az"]), P(t["el"]), n_rays, P(t["x"]), P(t["y"]), P(t["z"]),
                                                stream)] + \
               [lib.rg_gate_mask_f32(P(t["data"]), n, nat.GATE_OPS[op], a, b, P(t["mask"]), stream) for op, a, b in gs.PROLOGUE_FILTERS]

    def check(c, got, which):
        """tests/test_gpu_parity.py, test_antenna_transform_kernel_vs_oracle_parity_unpinned: a coordinate is the oracle's
        float32 or its neighbour where it does not cancel to zero, and within rtol 1e-6 / atol 1e-3 everywhere.
        tests/test_gpu_prologue.py, test_gate_mask_byte_for_byte: the mask is ``old | pred`` byte for byte."""
        want = gs.expected("prologue", which)
        for key in ("x", "y", "z"):
            ulp = np.abs(got[key].view(np.int32).astype(np.int64) - want[key].view(np.int32).astype(np.int64))
            assert ulp[~(np.abs(want[key]) < 1e-3)].max() <= 1, (which, key)
            np.testing.assert_allclose(got[key], want[key], rtol=1e-6, atol=1e-3)
        assert np.array_equal(got["mask"], want["mask"]), f"prologue on {which}: {int((got['mask'] != want['mask']).sum())} bytes differ"

    inputs = {key: _pair("prologue", lambda p, key=key: p[key]) for key in ("ranges", "az", "el", "data")}
    return Chain(env, "prologue", inputs, dict(x=((n,), "float32"), y=((n,), "float32"), z=((n,), "float32")), enqueue, check,
                 in_place=dict(mask=_pair("prologue", lambda p: p["mask"])))


BUILDERS = dict(verification=_verification, convection=_convection, tracking=_tracking, raster=_raster, accumulation=_accumulation,
                motion=_motion, cells=_cells, products=_products, georef=_georef, gridding=_gridding, columns=_columns, mosaic=_mosaic, prologue=_prologue)


@pytest.mark.parametrize("name", gs.CHAINS)
def test_chain_captured_on_a_replays_on_b_with_dirty_workspaces(env, name):
    _unbroken()                                               # before the builder allocates or builds anything on the device
    _protocol(env, _guard_device(lambda: BUILDERS[name](env)))


# ---- threads ---------------------------------------------------------------------------------------------------------------------
THREAD_CHAINS = ("verification", "convection", "tracking", "raster")
THREAD_RUNS = 3


def test_four_host_threads_each_on_their_own_stream(env):
    """One process, four streams: every thread runs another chain three times on B into its own buffers.  ctypes releases
    the GIL around every call, so the entry points overlap on the host."""
    torch = env["torch"]
    _unbroken()

    def prepare():
        built = [BUILDERS[name](env) for name in THREAD_CHAINS]
        for c in built:
            c.load("B")
            c.poison()
        torch.cuda.synchronize()                              # the copies above ran on the current stream
        return built, [torch.cuda.Stream(device=env["dev"]) for _ in built]

    chains, streams = _guard_device(prepare)
    barrier = threading.Barrier(len(chains))
    failures = []

    def work(chain, stream):
        try:
            barrier.wait(timeout=60)
            for run in range(THREAD_RUNS):
                if run and chain.in_place:                    # every run starts from the scene, restored on the thread's stream
                    with torch.cuda.stream(stream):
                        chain.restore("B")
                statuses = chain.enqueue(int(stream.cuda_stream))
                if any(s != 0 for s in statuses):
                    failures.append((chain.name, statuses, env["lib"].rg_last_error().decode()))
                    return
        except BaseException as exc:                          # reported by the main thread
            failures.append((chain.name, repr(exc)))

    threads = [threading.Thread(target=work, args=(c, st)) for c, st in zip(chains, streams)]
    for th in threads:
        th.start()
    for th in threads:
        th.join(timeout=120)
    assert not any(th.is_alive() for th in threads)
    if failures:
        _STATE["broken"] = f"threads: {failures}"
    assert not failures, failures
    _guard_device(lambda: [st.synchronize() for st in streams])
    for c in chains:
        c.check(c.read(), "B")
        assert c.inputs_unchanged("B"), c.name


# ---- the table -------------------------------------------------------------------------------------------------------------------
CHAINED = {
    "verification": ("rg_contingency_f32", "rg_exceedance_sat_i32", "rg_fss_sums_i32", "rg_box_fraction_f32"),
    "convection": ("rg_echo_table_f32", "rg_disk_background", "rg_convective_centres_f32", "rg_convective_area_u8"),
    "tracking": ("rg_cell_overlap_i32", "rg_relabel_cells_i32"),
    "raster": ("rg_warp_mercator_f32", "rg_overview_f32", "rg_warp_mercator_rgba8", "rg_overview_rgba8", "rg_colormap_rgba"),
    "accumulation": ("rg_rain_rate_f32", "rg_accumulate_advected_f32"),
    "motion": ("rg_motion_quantize_f32", "rg_block_match_u8", "rg_advect_f32"),
    "cells": ("rg_label_components_f32", "rg_component_stats_f32", "rg_despeckle_select_f32"),
    "products": ("rg_column_profile_f32", "rg_elevation_ppi_f32", "rg_elevation_ppi_plan_f32", "rg_elevation_ppi_finish_f32",
                 "rg_collapse_ppi_f32", "rg_plane_filter_f32", "rg_grid_filter", "rg_nan_minmax"),
    "georef": ("rg_gates_to_frame_f32", "rg_frame_to_lonlat_f64"),
    "gridding": ("rg_pack_fields_f32", "rg_roi_grid_f32", "rg_roi_section_f32"),
    "columns": ("rg_csr_apply_f32_ex", "rg_csr_compact_apply_f32", "rg_csr_compact_apply_packed_f32", "rg_csr_compact_apply_packed_f32_ex",
                "rg_csr_compact_apply_columns_f32", "rg_csr_compact_apply_columns_f32_ex", "rg_csr_compact_apply_planes_f32",
                "rg_csr_compact_apply_planes_f32_ex"),
    "mosaic": ("rg_roi_grid_mosaic_f32", "rg_roi_grid_mosaic_combine_f32", "rg_roi_section_mosaic_f32",
               "rg_roi_section_mosaic_combine_f32"),
    "prologue": ("rg_antenna_to_cartesian_f32", "rg_gate_mask_f32"),
}
_BUILD = "a step of a geometry build: the next step needs its count on the host, so it cannot sit inside a per-volume graph"
_PIPELINE = "captured and replayed on new inputs by test_volume_pipeline_graph_replay_equals_eager and its full-size sibling"
EXCLUDED = {
    "rg_stream_read_probe": "the probe of the stream tests themselves: it exists to read back on the host",
    "rg_csr_apply_f32": _PIPELINE, "rg_column_reduce_f32": _PIPELINE, "rg_cappi_lerp_f32": _PIPELINE,
    "rg_geom_bin_gates_f32": _BUILD, "rg_geom_bin_levels_count": _BUILD, "rg_geom_bin_gates_levels_f32": _BUILD,
    "rg_geom_count_f32": _BUILD, "rg_geom_fill_f32": _BUILD, "rg_scan_counts_i64": _BUILD, "rg_csr_compact_count": _BUILD,
    "rg_csr_compact_fill": _BUILD, "rg_csr_compact_pack": _BUILD, "rg_csr_compact_pack_dense": _BUILD, "rg_csr_row_ends16": _BUILD,
    "rg_section_count_f32": _BUILD, "rg_section_fill_f32": _BUILD,
}
