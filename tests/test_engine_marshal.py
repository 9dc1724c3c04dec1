"""The binding's marshalling path (renderbaby_amd/_marshal.py) on its own: no device, no engine, no library.  What every query
method relies on -- a contiguous array goes by pointer as it stands, anything else is converted, a call of 0 items has None
pointers, every length is held to the call's, a host ``out`` is n contiguous records of its dtype, a tensor is on the form's
device with the record's element type and row -- is checked here once; the device form runs on CPU tensors, which the checks
do not tell from a GPU's."""
import numpy as np
import pytest

from renderbaby_amd import _marshal as m
from renderbaby_amd import abi, engine

# the issue's table: record -> (element dtype of its tensor, row width)
TABLE = {"RAY": (np.float32, 8), "SURFEL": (np.float32, 8), "PROBE": (np.float32, 4), "HIT": (np.float32, 12), "SURFACE": (np.float32, 12),
         "RADIANCE": (np.float32, 4), "LIT": (np.float32, 4), "OPENNESS": (np.int32, 2), "SH9": (np.float32, 28),
         "PROBE_DEPTH": (np.float32, 256)}
N = 3


def _rays(n=N):
    rays = np.zeros(n, dtype=abi.RAY)
    rays["origin"] = np.arange(3 * n, dtype=np.float32).reshape(n, 3)
    rays["dir"] = (0, 0, 1)
    return rays


def test_the_record_table_is_the_issues_and_follows_from_itemsize():
    assert len(m.RECORDS) == len(TABLE)
    for name, (elem, row) in TABLE.items():
        rec = getattr(abi, name)
        assert m.RECORDS[rec] == (np.dtype(elem), row) == m.layout(rec)
        assert row * 4 == rec.itemsize
    for scalar in (np.uint8, np.float32, m.SEEDS):
        assert m.layout(scalar) == (np.dtype(scalar), None)


def test_a_contiguous_array_of_the_dtype_goes_by_pointer_as_it_stands():
    rays, seeds, tmax = _rays(), np.arange(N, dtype=np.uint32), np.ones(N, dtype=np.float32)
    f = m.Form(0, rays, seeds, tmax)
    assert not f.on_device
    for value, dtype in ((rays, abi.RAY), (seeds, m.SEEDS), (tmax, np.float32)):
        a, ptr = f.input("x", value, dtype, N)
        assert a is value and ptr == value.ctypes.data
        a, ptr = f.optional("x", value, dtype, N)
        assert a is value and ptr == value.ctypes.data
    assert f.optional("x", None, m.SEEDS, N) == (None, None)
    out = np.empty(N, dtype=abi.HIT)
    res, ptr = f.output("out", out, abi.HIT, N)
    assert res is out and ptr == out.ctypes.data
    new, ptr = f.output("out", None, abi.HIT, N)
    assert new.dtype == abi.HIT and new.shape == (N,) and ptr == new.ctypes.data
    # an ndarray view over memory numpy does not own (a page-locked buffer) is as good as any
    raw = bytearray(N * abi.HIT.itemsize)
    view = np.frombuffer(raw, dtype=abi.HIT)
    res, ptr = f.output("hits_out", view, abi.HIT, N)
    assert res is view and ptr == view.ctypes.data


def test_anything_else_is_converted():
    rays = _rays(2 * N)
    a, ptr = m.host_in("rays", rays[::2], abi.RAY, N)
    assert a.flags.c_contiguous and ptr == a.ctypes.data != rays.ctypes.data and np.array_equal(a, rays[::2])
    a, ptr = m.host_in("seeds", [5.0, 6.0, 7.0], m.SEEDS, N)
    assert a.dtype == np.uint32 and a.tolist() == [5, 6, 7] and ptr == a.ctypes.data
    a, _ = m.host_in("tmax", np.ones((N, 1), dtype=np.float64), np.float32, N)
    assert a.dtype == np.float32 and a.shape == (N,)
    grid = np.zeros((2, 2), dtype=abi.RAY)
    assert m.host_in("rays", grid, abi.RAY, flat=False)[0] is grid and m.host_in("rays", grid, abi.RAY)[0].shape == (4,)


def test_a_call_of_no_items_has_none_pointers():
    f = m.Form(0)
    assert f.input("rays", _rays(0), abi.RAY)[1] is None
    assert f.optional("seeds", np.zeros(0, np.uint32), m.SEEDS, 0)[1] is None and f.optional("seeds", None, m.SEEDS, 0)[1] is None
    assert f.output("out", None, abi.RADIANCE, 0)[1] is None and f.output("out", np.empty(0, abi.RADIANCE), abi.RADIANCE, 0)[1] is None
    assert m.host_ptr(None) is None and m.host_out("out", None, np.float32, (0, 4, 4))[1] is None


def test_every_length_is_held_to_the_calls():
    f = m.Form(0)
    for bad in (lambda: f.optional("seeds", np.zeros(2, np.uint32), m.SEEDS, N),          # seeds against items
                lambda: f.optional("tmax", np.zeros(2, np.float32), np.float32, N),       # tmax against rays
                lambda: f.output("out", np.empty(2, abi.RADIANCE), abi.RADIANCE, N),      # out against items
                lambda: f.input("coeffs", np.zeros(2, abi.SH9), abi.SH9, N),
                lambda: m.ray_records(np.zeros((N, 3)), np.zeros((2, 3)))):
        with pytest.raises(ValueError):
            bad()
    # coeffs against nx * ny * nz and moments against coeffs, as light_points(_visible) ask: no call is made
    grid = np.zeros(1, dtype=abi.PROBE_GRID)
    grid["counts"], grid["step"] = (N, 1, 1), 1.0
    assert m.grid_records(grid[0])[1] == N
    calls = []
    call = lambda *a: calls.append(a)   # noqa: E731
    surfels = np.zeros(4, dtype=abi.SURFEL)
    vis = np.zeros(1, dtype=abi.LIGHT_VISIBILITY)
    with pytest.raises(ValueError):
        engine._light_points(f, call, grid, np.zeros(2, abi.SH9), surfels, None)
    with pytest.raises(ValueError):
        engine._light_points(f, call, grid, np.zeros(N, abi.SH9), surfels, None, None, np.zeros(2, abi.PROBE_DEPTH), vis)
    assert not calls
    lit = engine._light_points(f, call, grid, np.zeros(N, abi.SH9), surfels, None, None, np.zeros(N, abi.PROBE_DEPTH), vis)
    assert lit.dtype == abi.LIT and lit.shape == (4,) and [c[0] for c in calls] == ["rb_light_points_visible"] and calls[0][5] == 4


def test_a_host_out_is_n_contiguous_records_of_its_dtype():
    for out in ([0.0] * N, np.empty(N, dtype=abi.LIT), np.empty(N, dtype=np.float32), np.empty((N, 1), dtype=abi.RADIANCE),
                np.empty(2 * N, dtype=abi.RADIANCE)[::2], np.empty(N + 1, dtype=abi.RADIANCE)):
        with pytest.raises(ValueError):
            m.host_out("out", out, abi.RADIANCE, N)
    # ``any_shape``: the size is what counts (bake_lightmap's out and sums)
    img = np.empty((N, 4), dtype=np.float32)
    assert m.host_out("out", img, np.float32, (1, N, 4), any_shape=True)[0] is img
    for out in (np.empty((N, 3), dtype=np.float32), np.empty((2 * N, 4), dtype=np.float32)[::2], np.empty((N, 4), dtype=np.float64)):
        with pytest.raises(ValueError):
            m.host_out("out", out, np.float32, (1, N, 4), any_shape=True)


def test_the_device_form_checks_device_dtype_layout_and_shape():
    import torch
    cpu = torch.device("cpu")
    rays = torch.zeros((N, 8), dtype=torch.float32)
    # a tensor on another device than the form's: here a CPU tensor where the engine's device is cuda:0
    f = m.Form(0, rays)
    assert f.on_device
    for bad in (lambda: f.input("rays", rays, abi.RAY), lambda: f.output("out", torch.empty((N, 4)), abi.RADIANCE, N),
                lambda: f.input("rays", _rays(), abi.RAY)):   # (and beside a tensor no numpy array will do)
        with pytest.raises(ValueError):
            bad()
    # with the device right, every other rule on its own
    f = m.Form(cpu, rays)
    t, ptr = f.input("rays", rays, abi.RAY)
    assert t is rays and ptr == rays.data_ptr()
    assert f.input("rays", rays[:0], abi.RAY)[1] is None and f.output("out", None, abi.HIT, 0)[1] is None
    for bad in (rays.double(), torch.zeros((8, N)).t(), torch.zeros((N, 9)), torch.zeros(N * 8), torch.zeros((N, 8), dtype=torch.int32)):
        with pytest.raises(ValueError):
            f.input("rays", bad, abi.RAY)
    with pytest.raises(ValueError):
        f.input("rays", rays, abi.RAY, 2)
    new, ptr = f.output("out", None, abi.OPENNESS, N)
    assert new.dtype == torch.int32 and tuple(new.shape) == (N, 2) and ptr == new.data_ptr()
    out = torch.empty(N, dtype=torch.uint8)
    assert f.output("out", out, np.uint8, N)[0] is out
    for bad in (torch.empty(N), torch.empty((N, 1), dtype=torch.uint8), torch.empty(2, dtype=torch.uint8)):
        with pytest.raises(ValueError):
            f.output("out", bad, np.uint8, N)
    # seeds: 32-bit ids, signed or unsigned
    kinds = [torch.int32] + ([torch.uint32] if hasattr(torch, "uint32") else [])
    for kind in kinds:
        s = torch.zeros(N, dtype=kind)
        assert f.optional("seeds", s, m.SEEDS, N) == (s, s.data_ptr())
    for bad in (torch.zeros(N, dtype=torch.int64), torch.zeros(N), torch.zeros((N, 1), dtype=torch.int32), torch.zeros(2, dtype=torch.int32)):
        with pytest.raises(ValueError):
            f.optional("seeds", bad, m.SEEDS, N)
    # an int32 scalar is not the seeds: no uint32 tensor for it
    if hasattr(torch, "uint32"):
        with pytest.raises(ValueError):
            f.output("owners", torch.zeros(N, dtype=torch.uint32), np.int32, N)


def test_a_staged_call_uploads_numpy_and_gives_numpy_back():
    import torch
    cpu = torch.device("cpu")
    sh = np.zeros(N, dtype=abi.SH9)
    sh["sum"] = np.arange(N * 27, dtype=np.float32).reshape(N, 9, 3)
    f = m.Form(cpu, sh, None, staged=True)
    assert f.on_device and not f.tensors
    t, ptr = f.input("sh", sh, abi.SH9)
    assert tuple(t.shape) == (N, 28) and t.dtype == torch.float32 and ptr == t.data_ptr()
    back = f.result(t, abi.SH9)
    assert isinstance(back, np.ndarray) and back.dtype == abi.SH9 and np.array_equal(back, sh)
    with pytest.raises(ValueError):
        f.output("out", np.empty(N, dtype=abi.SH9), abi.SH9, N)   # the results of a device form are tensors
    # a tensor in: used where it lies, a tensor back; ``out`` may be the input itself
    src = torch.zeros((N, 28))
    f = m.Form(cpu, src, src, staged=True)
    assert f.tensors and f.input("sh", src, abi.SH9)[0] is src and f.output("out", src, abi.SH9, N)[0] is src and f.result(src, abi.SH9) is src
    # a host form gives its arrays back as they are
    assert m.Form(cpu).result(sh, abi.SH9) is sh


def test_the_recurring_records():
    import torch
    o, d = np.arange(6, dtype=np.float64).reshape(2, 3), np.ones((2, 3), dtype=np.float32)
    rays = m.ray_records(o, d)
    assert rays.dtype == abi.RAY and np.array_equal(rays["origin"], o) and np.array_equal(rays["dir"], d)
    surf = m.surfel_records(o, d)
    assert surf.dtype == abi.SURFEL and surf.tobytes() == rays.tobytes()
    assert m.surfel_records(surf) is surf and m.surfel_records(torch.zeros((2, 8))).shape == (2, 8)
    t = m.ray_records(torch.from_numpy(o).float(), torch.from_numpy(d))
    assert tuple(t.shape) == (2, 8) and t.numpy().tobytes() == rays.tobytes()
    rec = m.probe_records(o)
    assert rec.dtype == abi.PROBE and np.array_equal(rec["pos"], o) and not rec["_pad"].any()
    assert m.probe_records(torch.from_numpy(o).float()).numpy().tobytes() == rec.tobytes()
    for bad in (lambda: m.ray_records(torch.zeros((2, 3)), d), lambda: m.ray_records(torch.zeros((2, 3)).double(), torch.zeros((2, 3)).double()),
                lambda: m.probe_records(torch.zeros((2, 3)).double())):
        with pytest.raises(ValueError):
            bad()
