"""Batches and input placements for the stream-ordering tests of ``batch.VolumeBatch.grid_shard``
(tests/test_batch_stream_scenes.py, tests/test_gpu_batch_streams.py).

``grid_shard`` uploads host-resident inputs one group ahead on a copy stream into two persistent staging sets; what orders
the copy stream and the caller's stream is two events per group.  A pass that read another group's staging set must give
another grid, so the volumes here are pairwise different (values and masks), and two disjoint batches A and B exist for
the "which data did the pass read" tests.  The field counts make BOTH paths run four groups of 2 + 2 + 2 + 1 volumes on a
batch of seven: the CSR path fuses 4 field-volumes per pass (2 fields), the CSR-free path 8 (3 fields).

NumPy only: importable without a GPU.  Everything is computed once, shared and read-only."""
from __future__ import annotations

import functools
from typing import Dict, List, Optional, Tuple

import numpy as np

VOLUME = dict(n_elev=4, n_az=90, n_gates=100)
SHAPE = (5, 20, 24)                                           # the grid of tests/test_gpu_batch.py
LIMITS = ((0.0, 6000.0), (-50e3, 50e3), (-60e3, 60e3))
FIELDS = ("DBZH", "ZDR", "RHOHV")
UNMASKED = ("RHOHV",)                                         # handed over with mask=None (the generator masks none of its gates)
SEEDS = {"A": tuple(range(40, 47)), "B": tuple(range(60, 67))}
N_VOLUMES = 7
# path -> (field names, field-volumes one pass fuses).  The GPU file asserts the group counts that follow through ``events=``.
PATHS = {"csr": (("DBZH", "RHOHV"), 4), "fused": (FIELDS, 8)}
# repeated calls on one VolumeBatch: (batch, volume numbers) -- 7, then 2, then 5 volumes
CALLS = (("A", (0, 1, 2, 3, 4, 5, 6)), ("B", (0, 1)), ("A", (2, 3, 4, 5, 6)))
ANCHORED = (("A", 0), ("B", N_VOLUMES - 1))                   # the reference run is held to the oracle on these volumes

# Where one array lives when it is handed to grid_shard:
#   numpy            pageable NumPy (values float32, mask bool): the copy is synchronous with the host
#   pinned           page-locked torch tensor (values float32, mask uint8): the asynchronous copy the class was written for
#   pinned_bool      page-locked bool mask: the copy converts
#   device           contiguous float32 / uint8 tensor on the device: passes through
#   device_bool      bool mask on the device: needs a conversion kernel
#   device_strided   every second element of a float32 buffer on the device: needs a gather
HOST = ("numpy", "pinned", "pinned_bool")
DEVICE = ("device", "device_bool", "device_strided")
KINDS = ("pageable", "pinned_u8", "pinned_bool", "device", "device_convert", "mixed_volumes", "mixed_fields")
_UNIFORM = {"pageable": ("numpy", "numpy"), "pinned_u8": ("pinned", "pinned"), "pinned_bool": ("pinned", "pinned_bool"),
            "device": ("device", "device"), "device_convert": ("device_strided", "device_bool")}
_BY_VOLUME = ("pinned_u8", "device_convert", "pageable")      # mixed_volumes: volume i takes kind i mod 3
_BY_FIELD = {"DBZH": ("pinned", "device_bool"), "ZDR": ("device_strided", "pinned"), "RHOHV": ("numpy", "numpy")}


def placement(kind: str, i: int, name: str) -> Tuple[str, str]:
    """``(where the values live, where the mask lives)`` for field ``name`` of volume ``i`` of its batch."""
    if kind == "mixed_volumes":
        return _UNIFORM[_BY_VOLUME[i % len(_BY_VOLUME)]]
    if kind == "mixed_fields":
        return _BY_FIELD[name]
    return _UNIFORM[kind]


def group_sizes(n_volumes: int, n_fields: int, per_pass: int) -> List[int]:
    """Volumes per group of a call: ``max(1, per_pass // n_fields)`` volumes each, the last group what is left."""
    per = max(1, per_pass // n_fields)
    return [min(per, n_volumes - g0) for g0 in range(0, n_volumes, per)]


@functools.lru_cache(maxsize=None)
def volume(seed: int):
    from radar_processor_amd import synthetic
    return synthetic.make_volume(seed=seed, fields=FIELDS, **VOLUME)


def n_gates() -> int:
    return VOLUME["n_elev"] * VOLUME["n_az"] * VOLUME["n_gates"]


@functools.lru_cache(maxsize=None)
def batch(which: str) -> Tuple[Dict[str, Tuple[np.ndarray, Optional[np.ndarray]]], ...]:
    """``{field: (values float32 [G], mask bool [G] or None)}`` per volume of batch ``which``."""
    out = []
    for seed in SEEDS[which]:
        vol = volume(seed)
        out.append({name: (np.array(np.ma.getdata(vol.fields[name])),
                           None if name in UNMASKED else np.array(np.ma.getmaskarray(vol.fields[name]))) for name in FIELDS})
        for values, mask in out[-1].values():
            values.setflags(write=False)
            if mask is not None:
                mask.setflags(write=False)
    return tuple(out)


def masked_field(which: str, b: int, name: str):
    """The masked array of one field, as the oracle takes it."""
    return volume(SEEDS[which][b]).fields[name]
