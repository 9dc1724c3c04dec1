"""Direct light with the emitters picked per grid cell (rb_emitter_grid_cdf / rb_light_rays_grid / rb_direct_light_grid and their
device forms), the part that needs no device: the library exports the five entry points with the
prototypes rb_abi.h states, the C++ mirror compiles against them, and the engine-less forms refuse every bad argument --
rb_light_rays' whole list, rb_light_points' of the grid, the entry cap, a NULL grid, a row of tables that decreases or ends
above 2^24 -- before they touch a device (device = -1: the call would otherwise use the current one), with their outputs
unwritten."""
import os
import subprocess
import textwrap

import numpy as np
import pytest

from renderbaby_amd import _lib, abi
from tests.test_direct_abi import INVALID_OPTIONS, NULL_ARGUMENT, REFUSALS, ROOT, _params, _surfels, _table
from tests.test_direct_cdf_abi import BAD_TABLES, _u32
from tests.test_probe_light_abi import GRID_REFUSALS, _grid

SYMBOLS = ("rb_emitter_grid_cdf", "rb_emitter_grid_cdf_device", "rb_light_rays_grid", "rb_direct_light_grid", "rb_direct_light_grid_device")
CAP = 1 << 26


def test_library_exports_the_symbols():
    lib = _lib.load()
    for name in SYMBOLS:
        assert name in _lib.EXPORTS
        getattr(lib, name)
    assert abi.MAX_GRID_ENTRIES == CAP


def test_prototypes_from_a_compiled_c_program(tmp_path):
    proto = tmp_path / "proto.c"
    proto.write_text(textwrap.dedent('''
        #include "rb_abi.h"
        _Static_assert(RB_MAX_GRID_ENTRIES == (1u << 26), "the entry cap");
        int (*f0)(int32_t, const rb_emitter*, size_t, const rb_probe_grid*, uint32_t*) = rb_emitter_grid_cdf;
        int (*f1)(rb_engine*, const rb_emitter*, size_t, const rb_probe_grid*, uint32_t*) = rb_emitter_grid_cdf_device;
        int (*f2)(int32_t, const rb_emitter*, const rb_probe_grid*, const uint32_t*, size_t, const rb_surfel*, const uint32_t*, size_t,
                  const rb_light_params*, uint32_t, uint32_t, rb_ray*, float*, float*) = rb_light_rays_grid;
        int (*f3)(rb_engine*, const rb_emitter*, const rb_probe_grid*, const uint32_t*, size_t, const rb_surfel*, const uint32_t*, size_t,
                  const rb_light_params*, uint32_t, uint32_t, rb_radiance*) = rb_direct_light_grid;
        int (*f4)(rb_engine*, const rb_emitter*, const rb_probe_grid*, const uint32_t*, size_t, const rb_surfel*, const uint32_t*, size_t,
                  const rb_light_params*, uint32_t, uint32_t, rb_radiance*) = rb_direct_light_grid_device;
    '''))
    subprocess.check_call(["gcc", "-std=c11", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), "-c", str(proto), "-o", str(tmp_path / "proto.o")])


def test_python_mirror_has_the_calls():
    from renderbaby_amd import Engine, bake, direct, engine
    import inspect
    assert callable(Engine.emitter_grid) and callable(engine.emitter_grid_cdf) and callable(bake.pick_grid)
    for name in ("grid", "tables"):
        assert inspect.signature(engine.light_rays).parameters[name].default is None
        assert inspect.signature(direct.rays).parameters[name].default is None
    for fn in (direct.emitter_bounds, direct.grid_weights, direct.emitter_grid_cdf, direct.grid_cell):
        assert callable(fn)
    eng = Engine.__new__(Engine)
    pts = np.zeros((2, 3), np.float32)
    for bad in (("grid",), ("cells", _grid()), ("grid", _grid(), None, None)):
        with pytest.raises(ValueError, match="pick"):
            Engine.direct_light(eng, pts, pts, 1, pick=bad)
    g = bake.pick_grid(_table(), (4, 1, 2), points=[(-3, 0, 0), (3, 0, 8)])
    assert list(g["counts"]) == [4, 1, 2] and list(g["origin"]) == [-3, 0, -1] and list(g["step"]) == [1.5, 6, 4.5]


def _call(n=4, first_sample=0, samples=2, params="default", n_emit=2, emitters=True, surfels=True, seeds_in=False, rays=True, tmax=True,
          contrib=True, grid="default", tables="ramp"):
    """rb_light_rays_grid as tests.test_direct_abi._call calls rb_light_rays; ``tables``: "ramp" (1, 2 in each of the grid's
    eight rows), None (made for the call) or an array; ``grid``: "default" (2 x 2 x 2 cells), None or a record"""
    lib = _lib.load()
    prm = _params() if isinstance(params, str) else params
    g = _grid() if isinstance(grid, str) else grid
    sf, ids, tab = _surfels(4), np.arange(4, dtype=np.uint32), _table()
    t_in = np.tile(np.arange(1, 3, dtype=np.uint32), 8) if isinstance(tables, str) else tables
    m = max(min(n * samples, 1 << 16), 1)
    r, t, c = np.full(m, 7, dtype=abi.RAY), np.full(m, 7, dtype=np.float32), np.full((m, 4), 7, dtype=np.float32)
    rc = lib.rb_light_rays_grid(-1, tab.ctypes.data if emitters else None, None if g is None else g.ctypes.data,
                                None if t_in is None else t_in.ctypes.data, n_emit, sf.ctypes.data if surfels else None,
                                ids.ctypes.data if seeds_in else None, n, None if prm is None else prm.ctypes.data, first_sample, samples,
                                r.ctypes.data if rays else None, t.ctypes.data if tmax else None, c.ctypes.data if contrib else None)
    assert (t == 7).all() and (c == 7).all() and (r["_pad0"] == 7).all(), "a refused call wrote its outputs"
    return rc


def _build(n_emit=2, emitters=True, grid="default", out=True):
    """rb_emitter_grid_cdf on device -1; nothing may be written"""
    g = _grid() if isinstance(grid, str) else grid
    tab, res = _table(), np.full(16, 7, dtype=np.uint32)
    rc = _lib.load().rb_emitter_grid_cdf(-1, tab.ctypes.data if emitters else None, n_emit, None if g is None else g.ctypes.data,
                                         res.ctypes.data if out else None)
    assert (res == 7).all(), "a refused call wrote its output"
    return rc


# rb_light_rays' refusals are rb_light_rays_grid's, with a caller's tables and with tables made for the call
@pytest.mark.parametrize("tables", ["ramp", None], ids=["caller's tables", "made for the call"])
@pytest.mark.parametrize("name,kw", REFUSALS, ids=[r[0] for r in REFUSALS])
def test_light_rays_refusals_before_a_device_is_touched(name, kw, tables):
    assert _call(tables=tables, **kw) == INVALID_OPTIONS, name
    assert _lib.load().rb_last_error(None)


# the grid's cap (rows * max(N, 1) <= 2^26) on top of rb_light_points' list; n_emit = 2 unless stated
CAP_REFUSALS = [("rows alone above the cap", dict(counts=(1 << 13, 1 << 13, 2)), 0), ("rows * N one row above the cap", dict(counts=((CAP >> 1) + 1, 1, 1)), 2),
                ("rows * N far above", dict(counts=(1 << 10, 1 << 10, 1 << 10)), 2), ("one row of 2^24 emitters, 5 rows", dict(counts=(5, 1, 1)), 1 << 24)]


@pytest.mark.parametrize("name,kw", GRID_REFUSALS, ids=[r[0] for r in GRID_REFUSALS])
def test_grid_refusals_before_a_device_is_touched(name, kw):
    for tables in ("ramp", None):
        assert _call(grid=_grid(**kw), tables=tables) == INVALID_OPTIONS, name
        assert _call(grid=_grid(**kw), tables=tables, n=0) == INVALID_OPTIONS, name   # as bad parameters are: in an empty call too
    assert _build(grid=_grid(**kw)) == INVALID_OPTIONS, name
    assert _build(grid=_grid(**kw), n_emit=0) == INVALID_OPTIONS, name
    assert _lib.load().rb_last_error(None)


@pytest.mark.parametrize("name,kw,n_emit", CAP_REFUSALS, ids=[r[0] for r in CAP_REFUSALS])
def test_the_entry_cap(name, kw, n_emit):
    assert _call(grid=_grid(**kw), tables=None, n_emit=n_emit) == INVALID_OPTIONS, name
    assert _build(grid=_grid(**kw), n_emit=n_emit) == INVALID_OPTIONS, name
    assert b"2^26" in _lib.load().rb_last_error(None)


def test_the_cap_itself_is_taken():
    # (n == 0 and n_emit == 0: no device is asked for and no table is read)
    assert _call(grid=_grid(counts=(CAP, 1, 1)), tables=None, n_emit=0, n=0) == 0
    assert _call(grid=_grid(counts=(CAP >> 1, 1, 1)), tables=None, n_emit=2, n=0) == 0
    assert _call(grid=_grid(counts=(4, 1, 1)), tables=None, n_emit=1 << 24, n=0) == 0
    assert _build(grid=_grid(counts=(CAP, 1, 1)), n_emit=0, emitters=False, out=False) == 0


@pytest.mark.parametrize("name,table", BAD_TABLES, ids=[b[0] for b in BAD_TABLES])
def test_bad_host_rows_are_refused(name, table):
    good = np.arange(1, 3, dtype=np.uint32)
    for row in (0, 3, 7):   # the bad row first, in the middle, last
        tables = np.tile(good, 8)
        tables[2 * row:2 * row + 2] = table
        assert _call(tables=tables) == INVALID_OPTIONS, (name, row)
        assert _call(tables=tables, n=0) == INVALID_OPTIONS, (name, row)
        assert b"cdf" in _lib.load().rb_last_error(None)
    # rows need not agree with one another: a total that falls from one row to the next is fine
    assert _call(tables=np.tile(_u32(9, 9, 1, 2), 4), n=0) == 0


def test_null_arguments_and_empty_calls():
    assert _call(grid=None) == NULL_ARGUMENT and _call(grid=None, n=0) == NULL_ARGUMENT and _call(grid=None, tables=None) == NULL_ARGUMENT
    assert _call(params=None) == NULL_ARGUMENT
    assert _call(surfels=False) == NULL_ARGUMENT
    assert _call(rays=False) == NULL_ARGUMENT
    assert _call(tmax=False) == NULL_ARGUMENT
    assert _call(contrib=False) == NULL_ARGUMENT
    assert _call(emitters=False) == NULL_ARGUMENT          # n_emit > 0 without a table
    assert _call(emitters=False, tables=None) == NULL_ARGUMENT
    assert _call(emitters=False, n=0) == NULL_ARGUMENT
    # n == 0 is RB_OK in every form -- no device is asked for --, and the good edges of a row are taken
    assert _call(n=0) == 0 and _call(n=0, tables=None) == 0 and _call(n=0, surfels=False, rays=False, tmax=False, contrib=False) == 0
    assert _call(n=0, params=None) == 0 and _call(n=0, n_emit=0, emitters=False) == 0 and _call(n=0, n_emit=0, emitters=False, tables=None) == 0
    assert _call(n=0, tables=np.tile(_u32(0, 0), 8)) == 0 and _call(n=0, tables=np.tile(_u32(0, 1 << 24), 8)) == 0
    assert _call(n=0, samples=0) == INVALID_OPTIONS and _call(n=0, params=_params(flags=1)) == INVALID_OPTIONS
    # rb_emitter_grid_cdf: an empty table is RB_OK; NULL arrays, a NULL grid and too long a table are refused, the output unwritten
    assert _build(n_emit=0) == 0 and _build(n_emit=0, emitters=False, out=False) == 0
    assert _build(grid=None) == NULL_ARGUMENT and _build(grid=None, n_emit=0) == NULL_ARGUMENT
    assert _build(emitters=False) == NULL_ARGUMENT and _build(out=False) == NULL_ARGUMENT
    assert _build(n_emit=(1 << 24) + 1, grid=_grid(counts=(1, 1, 1))) == INVALID_OPTIONS
    # the engine forms refuse a NULL engine before they look at anything else
    lib = _lib.load()
    sf, prm, tab, g = _surfels(), _params(), _table(), _grid()
    tables = np.tile(_u32(1, 2), 8)
    rad = np.full(4, 7, dtype=abi.RADIANCE)
    for fn in (lib.rb_direct_light_grid, lib.rb_direct_light_grid_device):
        assert fn(None, tab.ctypes.data, g.ctypes.data, tables.ctypes.data, 2, sf.ctypes.data, None, 4, prm.ctypes.data, 0, 1, rad.ctypes.data) == NULL_ARGUMENT
        assert fn(None, None, g.ctypes.data, None, 2, sf.ctypes.data, None, 4, prm.ctypes.data, 0, 1, rad.ctypes.data) == NULL_ARGUMENT
        assert fn(None, None, None, None, 0, None, None, 0, None, 0, 0, None) == NULL_ARGUMENT
    assert (rad["weight"] == 7).all()
    out = np.full(16, 7, dtype=np.uint32)
    assert lib.rb_emitter_grid_cdf_device(None, None, 2, g.ctypes.data, out.ctypes.data) == NULL_ARGUMENT and (out == 7).all()


def test_cpp_mirror_compiles(tmp_path):
    src = tmp_path / "c.cpp"
    src.write_text(textwrap.dedent('''
        #include "renderbaby/engine.hpp"
        using namespace renderbaby;
        int use(Engine& e, const rb_surfel* d_surfels, rb_emitter* d_table, uint32_t* d_tables, rb_radiance* d_rad) {
            std::vector<rb_surfel> s(3);
            rb_probe_grid g{};
            g.step[0] = g.step[1] = g.step[2] = 1.0f;
            g.counts[0] = 4; g.counts[1] = 1; g.counts[2] = 2;
            std::vector<rb_emitter> t = e.scene_emitters();
            std::vector<uint32_t> rows = Engine::emitter_grid_cdf(t, g, -1);
            std::vector<rb_radiance> a = e.direct_light_grid(s, g, 16, t.size());
            std::vector<rb_radiance> b = e.direct_light_grid(s, g, 16, 0, 7, nullptr, Engine::light_params(), t);
            std::vector<rb_radiance> c = e.direct_light_grid(s, g, 16, 0, 7, nullptr, Engine::light_params(), t, rows);
            const rb_light_params p = Engine::light_params();
            e.emitter_grid_cdf_device(nullptr, t.size(), g, d_tables);
            e.emitter_grid_cdf_device(d_table, 8, g, d_tables);
            e.direct_light_grid_device(nullptr, g, d_tables, t.size(), d_surfels, nullptr, 3, p, d_rad, 16, 7);
            e.direct_light_grid_device(d_table, g, nullptr, 8, d_surfels, nullptr, 3, p, d_rad, 16);
            e.sync();
            return (int)(a.size() + b.size() + c.size() + rows.size());
        }
        int main() { return 0; }
    '''))
    lib_dir = os.path.join(ROOT, "renderbaby_amd")
    subprocess.check_call(["g++", "-std=c++17", "-Wall", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(tmp_path / "c"),
                           "-L", lib_dir, "-l:librenderbaby_hip.so", f"-Wl,-rpath,{lib_dir}"])
