"""The echo-motion scenes and their NumPy restatement themselves (tests/motion_scenes.py, tests/motion_oracle.py), on the CPU:
the restatement finds the motion the scenes were built with, honours the tie rule and the validity rules, its integral-image
sums equal the literal ones, and a nowcast along the estimated motion beats persistence.  Plus the bookkeeping of the ABI.

``ties``: the issue expects ``(0, -2)`` from every block.  The blocks of the lattice's first column start at ``x = 0``, so no
candidate with ``dx < 0`` lies inside the plane for them; among the candidates they do have, the tie rule picks ``(0, 2)``.
Every block is checked: ``(0, -2)`` wherever that candidate exists, ``(0, 2)`` in the first column."""
import ctypes
import os
import re

import numpy as np
import pytest

import motion_oracle as mo
import motion_scenes as ms
import radar_processor_amd as rg
from radar_processor_amd import _native, motion

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _inner_valid(name):
    m = ms.match(name)
    keep = ms.inner(m.valid)
    assert keep.sum() >= 10, f"{name}: only {int(keep.sum())} valid inner blocks"
    return m, keep


def test_an_integer_shift_is_found_exactly():
    m, keep = _inner_valid("shift")
    assert (ms.inner(m.disp)[keep] == np.array([3, -5])).all()
    assert (ms.inner(m.score)[keep] == 1.0).all()                       # the same levels, moved: exactly 1


def test_a_subpixel_shift_within_the_bounds_of_the_issue():
    m, keep = _inner_valid("subpixel")
    err = np.abs(ms.inner(m.motion)[keep] - np.array(ms.scene("subpixel").truth))
    print(f"subpixel: median {np.median(err):.4f} px, max {err.max():.4f} px over {int(keep.sum())} blocks")
    assert np.median(err) <= 0.15
    assert err.max() <= 0.5                                             # what an integer search guarantees unrefined


def test_rim_clips_the_candidates_on_all_four_sides():
    s, m = ms.scene("rim"), ms.match("rim")
    h, w = s.prev.shape
    assert w % 2 == 1 and (h - s.B) % s.S and (w - s.B) % s.S
    q = ms.levels("rim")[0]
    assert q[0].any() and q[-1].any() and q[:, 0].any() and q[:, -1].any()          # echo reaches every edge
    have = ~np.isnan(m.scores[0])                                       # [nby, nbx, dy + R, dx + R]
    valid, R = m.valid[0], s.R
    top = h - s.B - (valid.shape[0] - 1) * s.S                          # the largest dy of the last row of blocks
    right = w - s.B - (valid.shape[1] - 1) * s.S
    assert 0 <= top < R and 0 <= right < R
    assert valid[0].any() and valid[-1].any() and valid[:, 0].any() and valid[:, -1].any()
    assert not have[0][:, :R, :].any() and have[0][valid[0]][:, R, :].any()                      # south: no dy < 0
    assert not have[-1][:, R + top + 1:, :].any() and have[-1][valid[-1]][:, R + top, :].any()   # north: no dy > top
    assert not have[:, 0][:, :, :R].any() and have[:, 0][valid[:, 0]][:, :, R].any()             # west: no dx < 0
    assert not have[:, -1][:, :, R + right + 1:].any() and have[:, -1][valid[:, -1]][:, :, R + right].any()   # east
    assert (ms.inner(m.disp)[ms.inner(m.valid)] == np.array(s.truth)).all()


def test_ties_go_to_the_shortest_shift_then_the_smallest_dy_then_dx():
    m = ms.match("ties")
    assert m.valid.all()
    at_max = (m.scores == m.score[..., None, None]).sum(axis=(-2, -1))
    assert (at_max >= 2).all()
    assert (m.score == 1.0).all()
    assert (m.disp[0, :, 1:] == np.array([0, -2])).all()
    assert (m.disp[0, :, 0] == np.array([0, 2])).all()                  # x0 = 0: no candidate with dx < 0 exists (docstring)


def test_degenerate_blocks_come_out_as_planted():
    for name in ("degenerate_constant", "degenerate_all_nan"):
        m = ms.match(name)
        assert not m.valid.any() and np.isnan(m.score).all() and np.isnan(m.motion).all() and not m.disp.any()
    q = ms.levels("degenerate_constant")[0]
    assert (q == q[0, 0]).all() and q[0, 0] == 1 + int(np.float32(30.0) * np.float32(254.0 / 63.5))
    assert not ms.levels("degenerate_all_nan")[0].any()
    # exactly min_echo - 1 and exactly min_echo echo pixels
    s, m = ms.scene("degenerate_min_echo"), ms.match("degenerate_min_echo")
    counts = [int((s.prev[:, x0:x0 + 16] != 0).sum()) for x0 in (0, 16)]
    assert counts == [s.min_echo - 1, s.min_echo] and m.valid.tolist() == [[[False, True]]]
    assert np.isnan(m.score[0, 0, 0]) and m.score[0, 0, 1] == 1.0
    # the levels at and around lo and hi
    s = ms.scene("degenerate_levels")
    q = ms.levels("degenerate_levels")[0]
    got = [int(q[9 + k, 12 + k]) for k in range(11)]
    assert got == [1, 0, 255, 255, 255, 255, 0, 0, 254, 2, 1]
    assert (q[np.isnan(s.prev)] == 0).all() and (q[s.prev >= 0.0] >= 1).all()
    assert ms.match("degenerate_levels").valid.any()
    # a masked patch: level 0 under the mask, the block it covers is invalid, its neighbours live on
    s, m = ms.scene("degenerate_masked"), ms.match("degenerate_masked")
    qp, qn = ms.levels("degenerate_masked")
    assert not qp[s.mask_prev != 0].any() and not qn[s.mask_next != 0].any()
    assert ms.levels("degenerate_masked", masked=False)[0][s.mask_prev != 0].any()
    assert not m.valid[0, 2, 4] and ms.match("shift").valid[0, 2, 4] and m.valid.sum() >= 40


def test_extremes_and_the_stack():
    m = ms.match("extremes_64_32")
    assert m.scores.shape[-2:] == (65, 65) and m.valid.shape == (1, 9, 10) and m.valid.all()
    free = m.disp[0, :8, 2:, :]                                         # y0 <= 56, x0 >= 16: the candidate (7, -11) lies inside
    assert (free == np.array([7, -11])).all() and (m.score[0, :8, 2:] == 1.0).all()
    m = ms.match("extremes_4_0")
    assert m.scores.shape[-2:] == (1, 1) and m.valid.shape == (1, 1, 2) and not m.disp.any()
    assert (m.motion[m.valid] == 0.0).all()                             # one candidate: no neighbour, no offset
    m = ms.match("extremes_8_1")
    assert m.scores.shape[-2:] == (3, 3) and m.valid.all() and m.disp[0, 0, 0].tolist() == [0, 1]
    m = ms.match("stack")
    assert m.valid.shape == (3, 6, 9)
    assert (ms.inner(m.disp)[0][ms.inner(m.valid)[0]] == np.array([3, -5])).all()


def test_integral_image_sums_equal_the_literal_ones():
    for name in ("rim", "subpixel", "degenerate_min_echo", "extremes_8_1"):
        s, (qp, qn), m = ms.scene(name), ms.levels(name), ms.match(name)
        min_echo = s.B * s.B // 8 if s.min_echo is None else s.min_echo
        for by in range(m.valid.shape[1]):
            for bx in range(m.valid.shape[2]):
                direct, echo, va = mo.block_scores_direct(qp, qn, by, bx, s.B, s.S, s.R)
                assert bool(m.valid[0, by, bx]) == (echo >= min_echo and va > 0)
                if not m.valid[0, by, bx]:
                    direct[:] = np.nan
                assert np.array_equal(direct, m.scores[0, by, bx], equal_nan=True), (name, by, bx)


@pytest.mark.parametrize("kind", sorted(ms.NOWCAST_MOTIONS))
def test_a_nowcast_beats_persistence(kind):
    frames = ms.nowcast_frames(kind, (0.0, 1.0, 2.0, 4.0))
    forecast, filled, _ = mo.nowcast(frames[0], frames[1], (1.0, 3.0), ms.B, ms.S, ms.R)
    assert np.isfinite(filled).all()
    g = ms.NOWCAST_MARGIN

    def core(a):
        return np.nan_to_num(a, nan=0.0)[g:-g, g:-g]

    for k, truth in enumerate((frames[2], frames[3])):
        ours = float(np.abs(core(forecast[k]) - core(truth)).mean())
        persistence = float(np.abs(core(frames[1]) - core(truth)).mean())
        print(f"{kind}, lead {(1, 3)[k]}: nowcast {ours:.3f}, persistence {persistence:.3f}")
        assert ours <= 0.5 * persistence
    # lead 0 is the plane itself, bit for bit
    same = mo.advect(frames[1][None], filled, mo.block_lattice(frames[1].shape, ms.B, ms.S), (0.0,))
    assert same[0, 0].tobytes() == frames[1].tobytes()


def test_fill_replaces_missing_and_weak_vectors_by_the_mean_of_the_rest():
    motion_ = np.array([[[1.0, 2.0], [np.nan, np.nan]], [[3.0, -4.0], [9.0, 9.0]]], dtype=np.float32)
    score = np.array([[0.9, np.nan], [0.5, 0.49]], dtype=np.float32)
    out = mo.fill_motion(motion_, score, 0.5)
    assert out.dtype == np.float32 and out.tolist() == [[[1.0, 2.0], [2.0, -1.0]], [[3.0, -4.0], [2.0, -1.0]]]
    assert not mo.fill_motion(motion_, score, 0.95).any()               # none remains: zero


# ---- bookkeeping -----------------------------------------------------------------------------------------------------------
FUNCTIONS = ("rg_motion_quantize_f32", "rg_block_match_u8", "rg_advect_f32")


def test_abi_bookkeeping_and_exports():
    header = open(os.path.join(REPO, "include", "radargrid_hip.h")).read()
    declared = set(re.findall(r"^(?:int|int64_t|const char\*)\s+(rg_\w+)\s*\(", header, flags=re.M))
    assert "#define RG_VERSION 104" in header and _native.ABI_VERSION == 104
    for macro, value in (("RG_MOTION_MAX_BLOCK", 64), ("RG_MOTION_MAX_SEARCH", 32), ("RG_MAX_LEADS", 16)):
        assert f"#define {macro} {value}" in header and getattr(_native, macro) == value
    body = re.search(r"typedef struct rg_motion_lattice \{(.*?)\} rg_motion_lattice;", header, flags=re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    members = [(kind, m.strip()) for kind, decl in re.findall(r"(double|int32_t)\s+([^;]+);", body) for m in decl.split(",")]
    kinds = {"double": ctypes.c_double, "int32_t": ctypes.c_int32}
    assert [(kinds[k], m) for k, m in members] == [(t, n) for n, t in _native.MotionLattice._fields_]
    assert [m for _, m in members] == list(mo.Lattice._fields) == list(motion.Lattice._fields)
    from radar_processor_amd import build
    assert ("rg_motion.hip", []) in build.SOURCES
    lib = rg.load_library(require_device=False)
    for name in FUNCTIONS:
        assert name in declared and getattr(lib, name).argtypes == _native.SIGNATURES[name][1]
        args = re.search(r"^int %s\((.*?)\);" % name, header, flags=re.S | re.M).group(1).split(",")
        want = []
        for a in args:
            a = " ".join(a.split())
            want.append(_native.MotionLattice if a.startswith("rg_motion_lattice ") else
                        ctypes.POINTER(ctypes.c_double) if a.startswith("const double*") else
                        ctypes.c_void_p if ("*" in a or a.startswith("rg_stream_t")) else
                        ctypes.c_float if a.startswith("float ") else ctypes.c_int32)
        assert want == _native.SIGNATURES[name][1], name
    for name in ("quantize_planes_device", "estimate_motion_device", "fill_motion_device", "advect_device", "nowcast_device",
                 "nowcast", "motion_to_velocity", "MotionGrid"):
        assert name in rg.__all__ and getattr(rg, name) is getattr(motion, name)


def test_null_pointers_are_refused_without_a_device():
    """The first refusal of each entry point, reachable without a GPU (the others need real buffers: tests/test_gpu_motion.py)."""
    lib = rg.load_library(require_device=False)
    lat = _native.MotionLattice(0.0, 0.0, 1.0, 1.0, 4, 4)
    assert lib.rg_motion_quantize_f32(None, None, 1, 4, 4, 0.0, 4.0, None, None) == _native.RG_EINVAL
    assert b"rg_motion_quantize_f32: null pointer" in lib.rg_last_error()
    assert lib.rg_block_match_u8(None, None, 1, 8, 8, 8, 1, 1, 1, None, None, None, None) == _native.RG_EINVAL
    assert b"rg_block_match_u8: null pointer" in lib.rg_last_error()
    assert lib.rg_advect_f32(None, 1, 4, 4, None, lat, None, 1, 1, 0, 0.0, None, None) == _native.RG_EINVAL
    assert b"rg_advect_f32: null pointer" in lib.rg_last_error()
