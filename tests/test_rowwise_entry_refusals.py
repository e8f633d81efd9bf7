"""What the three entry points over the packed records refuse, and with which status: rg_csr_compact_apply_packed_f32,
rg_csr_compact_apply_columns_f32 and rg_csr_compact_apply_planes_f32 share their 17 leading arguments and the checks on them.
Every case starts from an otherwise valid call on a 2 x 4 x 64 grid without pairs and applies exactly ONE fault; the status
and the entry point's own name at the head of rg_last_error() are pinned.  CPU only: the pointers are fake and never
dereferenced, and no call passes validation with n_vox > 0, so nothing is launched."""
import ctypes

import pytest

import radar_processor_amd as rg
from radar_processor_amd import _native

P = 1 << 12                                  # a 16-byte aligned address that is never dereferenced
EINVAL, EALIGN, EUNSUP = _native.RG_EINVAL, _native.RG_EALIGN, _native.RG_EUNSUPPORTED
ENTRIES = ("packed", "columns", "planes")


def stride_for(nf):                          # rg_common.hpp
    return 1 if nf == 1 else 2 if nf == 2 else 4 if nf <= 4 else 8


def call(entry, **kw):
    """(status, rg_last_error(), entry point's name) of one call of `entry` with the valid arguments changed by `kw`."""
    lib = rg.load_library(require_device=False)
    a = dict(indptr=P, is64=0, records=P, rec_ptr=P, rec_order=_native.RG_REC_ORDER_DISPATCH, w_base=120 << 23, dict_ptr=P,
             dict=P, n_vox=2 * 4 * 64, n_pairs=0, line_len=64, lines_per_plane=4, packed=P, n_fields=3, stride=None,
             n_gates=100, fill=0.0)
    own = dict(out=P, window_cap=256, tile=0, lanes_hint=0)
    for k, v in kw.items():
        assert k in a or k in own, k
        (a if k in a else own)[k] = v
    if a["stride"] is None:
        a["stride"] = stride_for(a["n_fields"])
    lead = tuple(a.values())
    if entry == "packed":
        name = "rg_csr_compact_apply_packed_f32"
        assert own["lanes_hint"] == 0
        st = lib.rg_csr_compact_apply_packed_f32(*lead, own["out"], own["window_cap"], own["tile"], None)
    elif entry == "columns":
        name = "rg_csr_compact_apply_columns_f32"
        st = lib.rg_csr_compact_apply_columns_f32(*lead, own["out"], None, 0, 0, None, None, 0, 1, own["window_cap"], 1, None,
                                                  None, 0, own["lanes_hint"], None)
    else:
        name = "rg_csr_compact_apply_planes_f32"
        req = _native.PlaneRequest(out=own["out"], col_lo=0, col_hi=1)
        st = lib.rg_csr_compact_apply_planes_f32(*lead, ctypes.byref(req), own["window_cap"], 1, None, None, 0,
                                                 own["lanes_hint"], None)
    return st, lib.rg_last_error(), name.encode()


# fault -> expected status, for all three entry points
SHARED = [
    (dict(rec_order=2), EINVAL),
    (dict(n_fields=0), EUNSUP),
    (dict(stride=2), EINVAL),                               # three fields take 4 slots per gate
    (dict(n_fields=2, stride=4), EINVAL),
    (dict(indptr=None), EINVAL),
    (dict(dict_ptr=None), EINVAL),
    (dict(rec_ptr=None), EINVAL),
    (dict(n_vox=-1), EINVAL),
    (dict(n_pairs=-1), EINVAL),
    (dict(n_pairs=1, records=None), EINVAL),
    (dict(n_gates=2 ** 31), EUNSUP),
    (dict(n_vox=0x4000000000), EUNSUP),
    (dict(window_cap=-1), EINVAL),
    (dict(window_cap=_native.RG_COMPACT_MAX_WINDOW + 1), EINVAL),
    (dict(records=P + 8), EALIGN),
    (dict(w_base=(120 << 23) | 1), EINVAL),
    (dict(n_vox=100), EINVAL),                              # not planes x 4 lines x 64 rows
]


@pytest.mark.parametrize("entry", ENTRIES)
@pytest.mark.parametrize("fault,status", SHARED, ids=[",".join(f"{k}={v}" for k, v in f.items()) for f, _ in SHARED])
def test_shared_argument_faults(entry, fault, status):
    st, err, name = call(entry, **fault)
    assert st == status, (st, err)
    assert err.startswith(name), err


def test_max_window_is_the_documented_one():
    assert _native.RG_COMPACT_MAX_WINDOW == 8192


@pytest.mark.parametrize("entry", ENTRIES)
def test_valid_call_on_an_empty_grid_is_ok(entry):
    st, err, _ = call(entry, n_vox=0)
    assert st == _native.RG_OK, err


def test_field_count_ceilings():
    """The row-wise kernel takes 1-8 fields, the tile kernel over the records and the column / planes modes 1-4."""
    for entry, kw in (("packed", dict(n_fields=9)), ("packed", dict(n_fields=5, tile=384)), ("columns", dict(n_fields=5)),
                      ("planes", dict(n_fields=5))):
        st, err, name = call(entry, **kw)
        assert st == EUNSUP and err.startswith(name), (entry, kw, st, err)


def test_packed_entry_needs_out():
    st, err, name = call("packed", out=None)
    assert st == EINVAL and err.startswith(name), (st, err)


@pytest.mark.parametrize("entry", ("columns", "planes"))
def test_column_modes_check_the_packed_fields_and_the_lane_split(entry):
    """Only these two refuse null or misaligned packed fields when there are no pairs, and they take the lane split as an
    argument of its own (0, a power of two up to 64, or 71..99)."""
    st, err, name = call(entry, packed=None)
    assert st == EINVAL and err.startswith(name), (st, err)
    st, err, name = call(entry, packed=P + 8)
    assert st == EALIGN and err.startswith(name), (st, err)
    for hint in (3, 65, 70, 100):
        st, err, name = call(entry, lanes_hint=hint)
        assert st == EINVAL and err.startswith(name), (hint, st, err)
