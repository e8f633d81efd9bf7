"""A device-layout sidecar whose key matches but whose arrays do not fit the geometry's chunk layout is refused on the host
(``compact_layout.check_sidecar``), before any of its arrays is uploaded: no kernel sees them.  Companion of
``test_gpu_dense_records.py::test_sidecar_without_the_record_format_tag_is_refused_and_rebuilt``, at its shape."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu


def test_sidecar_with_arrays_of_the_wrong_size_is_refused_and_rebuilt(tmp_path, caplog):
    import torch
    import radar_processor_amd as rg
    from radar_processor_amd.gridding import CsrGridder
    rg.load_library()
    rng = np.random.default_rng(3)
    n = 6000
    gx, gy = rng.uniform(-20e3, 20e3, n).astype(np.float32), rng.uniform(-20e3, 20e3, n).astype(np.float32)
    gz = rng.uniform(0.0, 9e3, n).astype(np.float32)
    val = rng.normal(10, 20, n).astype(np.float32)
    shape, limits = (3, 9, 130), ((0.0, 8e3), (-20e3, 20e3), (-20e3, 20e3))
    geom = rg.compute_grid_geometry(gx, gy, gz, shape, limits, str(tmp_path), min_radius=900.0, beam_factor=0.05)
    dev = torch.device("cuda")
    npz, side = str(tmp_path / "g.npz"), str(tmp_path / "g.layout")          # no suffix: numpy.savez appends it
    rg.save_geometry(geom, npz)
    assert rg.save_device_layout(geom, side)
    with np.load(side + ".npz", allow_pickle=False) as data:
        arrays = {k: data[k] for k in data.files}
    assert arrays["rec"].shape[0] > 1 and arrays["dict_ptr"].size > 2
    f_t = torch.from_numpy(val).to(dev)

    def grid(g):
        compact = g.device_compact(dev)
        assert compact is not None and compact.ensure_packed(g.device_csr(dev))
        gr = CsrGridder(g, n, 1, device=dev)
        gr.compact, gr.window, gr.packed_stream = compact, compact.window_for(1, rowwise=True), True
        gr.pack([f_t], [None])
        out = torch.empty((1, gr.n_vox), dtype=torch.float32, device=dev)
        gr.apply(out)
        return out, compact
    want, c0 = grid(geom)
    for name in ("rec", "dict_ptr"):
        bad = str(tmp_path / f"g.short_{name}.npz")
        np.savez(bad, **{k: (v[:-1] if k == name else v) for k, v in arrays.items()})
        loaded = rg.load_geometry(npz)
        caplog.clear()
        with caplog.at_level("WARNING", logger="radar_grid.geometry"):
            assert rg.load_device_layout(loaded, bad) is False
        assert f"({name} has shape" in caplog.text and getattr(loaded, "_compact", None) is None
        assert not loaded.is_device_resident                             # refused before anything went to the device
        got, c1 = grid(loaded)                                           # derived again from the reference arrays
        assert c1 is not c0 and torch.equal(got.view(torch.int32), want.view(torch.int32))
