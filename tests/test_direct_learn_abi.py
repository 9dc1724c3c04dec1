"""Per-cell emitter tables that learn visibility (rb_direct_light_grid_tally / rb_emitter_grid_learned and their device forms;
DESIGN.md section 25), the part that needs no device: the library exports the four entry points with the prototypes rb_abi.h
states and the record is 8 bytes, the C++ mirror compiles against them, and the engine-less build refuses every bad argument
-- rb_emitter_grid_cdf's whole list, a bad prior, a NULL tally -- before it touches a device (device = -1: the call would
otherwise use the current one), with its output unwritten and the tally as it was."""
import os
import subprocess
import textwrap

import numpy as np
import pytest

from renderbaby_amd import _lib, abi
from tests.test_direct_abi import INVALID_OPTIONS, NULL_ARGUMENT, ROOT, _params, _surfels, _table
from tests.test_direct_grid_abi import CAP, CAP_REFUSALS
from tests.test_probe_light_abi import GRID_REFUSALS, _grid

SYMBOLS = ("rb_direct_light_grid_tally", "rb_direct_light_grid_tally_device", "rb_emitter_grid_learned", "rb_emitter_grid_learned_device")
BAD_PRIORS = [0.0, -0.0, -1.0, float("nan"), float("inf"), float("-inf"), 16777218.0, 3.0e38]


def test_library_exports_the_symbols():
    lib = _lib.load()
    for name in SYMBOLS:
        assert name in _lib.EXPORTS
        getattr(lib, name)
    assert abi.GRID_TALLY.itemsize == 8 and abi.GRID_TALLY.names == ("tried", "seen") and abi.GRID_TALLY.fields["seen"][1] == 4
    assert abi.MAX_PRIOR == 16777216.0


def test_prototypes_from_a_compiled_c_program(tmp_path):
    proto = tmp_path / "proto.c"
    proto.write_text(textwrap.dedent('''
        #include <stddef.h>
        #include "rb_abi.h"
        _Static_assert(sizeof(rb_grid_tally) == 8, "the record");
        _Static_assert(offsetof(rb_grid_tally, tried) == 0 && offsetof(rb_grid_tally, seen) == 4, "tried, seen");
        int (*f0)(rb_engine*, const rb_emitter*, const rb_probe_grid*, const uint32_t*, size_t, const rb_surfel*, const uint32_t*, size_t,
                  const rb_light_params*, uint32_t, uint32_t, rb_radiance*, rb_grid_tally*) = rb_direct_light_grid_tally;
        int (*f1)(rb_engine*, const rb_emitter*, const rb_probe_grid*, const uint32_t*, size_t, const rb_surfel*, const uint32_t*, size_t,
                  const rb_light_params*, uint32_t, uint32_t, rb_radiance*, rb_grid_tally*) = rb_direct_light_grid_tally_device;
        int (*f2)(int32_t, const rb_emitter*, size_t, const rb_probe_grid*, const rb_grid_tally*, float, uint32_t*) = rb_emitter_grid_learned;
        int (*f3)(rb_engine*, const rb_emitter*, size_t, const rb_probe_grid*, const rb_grid_tally*, float, uint32_t*) = rb_emitter_grid_learned_device;
    '''))
    subprocess.check_call(["gcc", "-std=c11", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), "-c", str(proto), "-o", str(tmp_path / "proto.o")])


def test_python_mirror_has_the_calls():
    import inspect
    from renderbaby_amd import Engine, bake, direct, engine
    assert callable(engine.emitter_grid_learned) and callable(bake.learn_grid)
    for fn in (direct.count, direct.tally, direct.seen_share):
        assert callable(fn)
    assert inspect.signature(Engine.direct_light).parameters["tally"].default is None
    assert inspect.signature(Engine.emitter_grid).parameters["tally"].default is None
    assert inspect.signature(direct.grid_weights).parameters["tally"].default is None
    assert inspect.signature(direct.emitter_grid_cdf).parameters["tally"].default is None
    eng = Engine.__new__(Engine)
    pts = np.zeros((2, 3), np.float32)
    kept = np.zeros(16, dtype=abi.GRID_TALLY)
    with pytest.raises(ValueError, match="tally"):
        Engine.direct_light(eng, pts, pts, 1, pick="power", tally=kept)   # a tally goes with a grid
    with pytest.raises(ValueError, match="tally"):
        Engine.direct_light(eng, pts, pts, 1, tally=kept)
    with pytest.raises(ValueError, match="out"):
        Engine.direct_light(eng, pts, pts, 1, pick=("grid", _grid()), out=False)   # no sums and no tally: nothing to do


def _build(n_emit=2, emitters=True, grid="default", out=True, tally=True, prior=1.0):
    """rb_emitter_grid_learned on device -1; neither the output nor the tally may be written"""
    g = _grid() if isinstance(grid, str) else grid
    tab, res = _table(), np.full(16, 7, dtype=np.uint32)
    kept = np.full(16, 5, dtype=np.uint32).view(abi.GRID_TALLY)
    rc = _lib.load().rb_emitter_grid_learned(-1, tab.ctypes.data if emitters else None, n_emit, None if g is None else g.ctypes.data,
                                             kept.ctypes.data if tally else None, prior, res.ctypes.data if out else None)
    assert (res == 7).all() and (kept.view(np.uint32) == 5).all(), "a refused call wrote its output or the tally"
    return rc


@pytest.mark.parametrize("name,kw", GRID_REFUSALS, ids=[r[0] for r in GRID_REFUSALS])
def test_grid_refusals_before_a_device_is_touched(name, kw):
    assert _build(grid=_grid(**kw)) == INVALID_OPTIONS, name
    assert _build(grid=_grid(**kw), n_emit=0) == INVALID_OPTIONS, name
    assert _lib.load().rb_last_error(None)


@pytest.mark.parametrize("name,kw,n_emit", CAP_REFUSALS, ids=[r[0] for r in CAP_REFUSALS])
def test_the_entry_cap(name, kw, n_emit):
    assert _build(grid=_grid(**kw), n_emit=n_emit) == INVALID_OPTIONS, name
    assert b"2^26" in _lib.load().rb_last_error(None)


@pytest.mark.parametrize("prior", BAD_PRIORS, ids=[str(p) for p in BAD_PRIORS])
def test_a_bad_prior_is_refused(prior):
    assert _build(prior=prior) == INVALID_OPTIONS
    assert b"prior" in _lib.load().rb_last_error(None)
    assert _build(prior=prior, n_emit=0) == INVALID_OPTIONS   # as bad parameters are: in an empty call too


def test_null_arguments_and_empty_calls():
    assert _build(grid=None) == NULL_ARGUMENT and _build(grid=None, n_emit=0) == NULL_ARGUMENT
    assert _build(emitters=False) == NULL_ARGUMENT and _build(out=False) == NULL_ARGUMENT and _build(tally=False) == NULL_ARGUMENT
    assert _build(n_emit=(1 << 24) + 1, grid=_grid(counts=(1, 1, 1))) == INVALID_OPTIONS
    # an empty table is RB_OK without a device, with or without the arrays; the good ends of the prior are taken
    assert _build(n_emit=0) == 0 and _build(n_emit=0, emitters=False, out=False, tally=False) == 0
    assert _build(n_emit=0, prior=16777216.0) == 0 and _build(n_emit=0, prior=1e-45) == 0
    assert _build(grid=_grid(counts=(CAP, 1, 1)), n_emit=0, emitters=False, out=False, tally=False) == 0
    # the engine forms refuse a NULL engine before they look at anything else
    lib = _lib.load()
    sf, prm, tab, g = _surfels(), _params(), _table(), _grid()
    tables = np.tile(np.arange(1, 3, dtype=np.uint32), 8)
    rad = np.full(4, 7, dtype=abi.RADIANCE)
    kept = np.full(32, 5, dtype=np.uint32).view(abi.GRID_TALLY)
    for fn in (lib.rb_direct_light_grid_tally, lib.rb_direct_light_grid_tally_device):
        assert fn(None, tab.ctypes.data, g.ctypes.data, tables.ctypes.data, 2, sf.ctypes.data, None, 4, prm.ctypes.data, 0, 1, rad.ctypes.data,
                  kept.ctypes.data) == NULL_ARGUMENT
        assert fn(None, None, g.ctypes.data, None, 2, sf.ctypes.data, None, 4, prm.ctypes.data, 0, 1, None, kept.ctypes.data) == NULL_ARGUMENT
        assert fn(None, None, None, None, 0, None, None, 0, None, 0, 0, None, None) == NULL_ARGUMENT
    out = np.full(16, 7, dtype=np.uint32)
    assert lib.rb_emitter_grid_learned_device(None, None, 2, g.ctypes.data, kept.ctypes.data, 1.0, out.ctypes.data) == NULL_ARGUMENT
    assert (rad["weight"] == 7).all() and (out == 7).all() and (kept.view(np.uint32) == 5).all()


def test_cpp_mirror_compiles(tmp_path):
    src = tmp_path / "c.cpp"
    src.write_text(textwrap.dedent('''
        #include "renderbaby/engine.hpp"
        using namespace renderbaby;
        static_assert(sizeof(rb_grid_tally) == 8, "the record");
        int use(Engine& e, const rb_surfel* d_surfels, rb_emitter* d_table, uint32_t* d_tables, rb_radiance* d_rad, rb_grid_tally* d_tally) {
            std::vector<rb_surfel> s(3);
            rb_probe_grid g{};
            g.step[0] = g.step[1] = g.step[2] = 1.0f;
            g.counts[0] = 4; g.counts[1] = 1; g.counts[2] = 2;
            std::vector<rb_emitter> t = e.scene_emitters();
            std::vector<rb_grid_tally> kept(t.size() * 8);
            std::vector<rb_radiance> a = e.direct_light_grid_tally(s, g, 16, kept, t.size());
            std::vector<uint32_t> rows = Engine::emitter_grid_learned(t, g, kept, 0.5f, -1);
            std::vector<rb_radiance> b = e.direct_light_grid_tally(s, g, 16, kept, 0, 7, nullptr, Engine::light_params(), t, rows);
            std::vector<rb_radiance> c = e.direct_light_grid_tally(s, g, 16, kept, 0, 7, nullptr, Engine::light_params(), t, rows, false);
            const rb_light_params p = Engine::light_params();
            e.direct_light_grid_tally_device(nullptr, g, d_tables, t.size(), d_surfels, nullptr, 3, p, d_rad, d_tally, 16, 7);
            e.direct_light_grid_tally_device(d_table, g, nullptr, 8, d_surfels, nullptr, 3, p, nullptr, d_tally, 16);
            e.emitter_grid_learned_device(nullptr, t.size(), g, d_tally, 1.0f, d_tables);
            e.emitter_grid_learned_device(d_table, 8, g, d_tally, 2.0f, d_tables);
            e.sync();
            return (int)(a.size() + b.size() + c.size() + rows.size());
        }
        int main() { return 0; }
    '''))
    lib_dir = os.path.join(ROOT, "renderbaby_amd")
    subprocess.check_call(["g++", "-std=c++17", "-Wall", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(tmp_path / "c"),
                           "-L", lib_dir, "-l:librenderbaby_hip.so", f"-Wl,-rpath,{lib_dir}"])
