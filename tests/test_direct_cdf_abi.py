"""Direct light with a weighted pick (rb_emitter_cdf / rb_scene_emitter_cdf / rb_light_rays_cdf / rb_direct_light_cdf; DESIGN.md
section 23), the part that needs no device: the library exports the six entry points with the prototypes rb_abi.h states, the
C++ mirror compiles against them, and the engine-less forms refuse every bad argument -- rb_light_rays' whole list, and a table
of weights that decreases or ends above 2^24 -- before they touch a device (device = -1: the call would otherwise use the
current one), with their outputs unwritten."""
import ctypes as C
import os
import subprocess
import textwrap

import numpy as np
import pytest

from renderbaby_amd import _lib, abi
from tests.test_direct_abi import INVALID_OPTIONS, NULL_ARGUMENT, REFUSALS, ROOT, _params, _surfels, _table

SYMBOLS = ("rb_emitter_cdf", "rb_scene_emitter_cdf", "rb_scene_emitter_cdf_device", "rb_light_rays_cdf", "rb_direct_light_cdf",
           "rb_direct_light_cdf_device")


def test_library_exports_the_symbols():
    lib = _lib.load()
    for name in SYMBOLS:
        assert name in _lib.EXPORTS
        getattr(lib, name)


def test_prototypes_from_a_compiled_c_program(tmp_path):
    proto = tmp_path / "proto.c"
    proto.write_text(textwrap.dedent('''
        #include "rb_abi.h"
        int (*f0)(int32_t, const rb_emitter*, size_t, uint32_t*) = rb_emitter_cdf;
        int (*f1)(rb_engine*, uint32_t*, size_t, size_t*) = rb_scene_emitter_cdf;
        int (*f2)(rb_engine*, uint32_t*, size_t, uint32_t*) = rb_scene_emitter_cdf_device;
        int (*f3)(int32_t, const rb_emitter*, const uint32_t*, size_t, const rb_surfel*, const uint32_t*, size_t, const rb_light_params*, uint32_t,
                  uint32_t, rb_ray*, float*, float*) = rb_light_rays_cdf;
        int (*f4)(rb_engine*, const rb_emitter*, const uint32_t*, size_t, const rb_surfel*, const uint32_t*, size_t, const rb_light_params*,
                  uint32_t, uint32_t, rb_radiance*) = rb_direct_light_cdf;
        int (*f5)(rb_engine*, const rb_emitter*, const uint32_t*, size_t, const rb_surfel*, const uint32_t*, size_t, const rb_light_params*,
                  uint32_t, uint32_t, rb_radiance*) = rb_direct_light_cdf_device;
    '''))
    subprocess.check_call(["gcc", "-std=c11", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), "-c", str(proto), "-o", str(tmp_path / "proto.o")])


def test_python_mirror_has_the_calls():
    from renderbaby_amd import Engine, _marshal, bake, direct, engine
    import inspect
    assert callable(Engine.scene_emitter_cdf) and callable(engine.emitter_cdf)
    assert inspect.signature(Engine.direct_light).parameters["pick"].default == "uniform"
    assert inspect.signature(engine.light_rays).parameters["cdf"].default is None
    assert inspect.signature(direct.rays).parameters["cdf"].default is None
    for fn in (bake.direct_irradiance, bake.lightmap_direct):
        assert inspect.signature(fn).parameters["pick"].default == "uniform"
    assert callable(direct.emitter_weights) and callable(direct.emitter_cdf) and callable(direct.pick_cdf)
    assert _marshal.layout(_marshal.CDF) == (np.dtype(np.uint32), None)


def _call(n=4, first_sample=0, samples=2, params="default", n_emit=2, emitters=True, surfels=True, seeds_in=False, rays=True, tmax=True,
          contrib=True, cdf="ramp"):
    """rb_light_rays_cdf as tests.test_direct_abi._call calls rb_light_rays; ``cdf``: "ramp" (1, 2), None (by power) or an array"""
    lib = _lib.load()
    prm = _params() if isinstance(params, str) else params
    sf, ids, tab = _surfels(4), np.arange(4, dtype=np.uint32), _table()
    table = np.arange(1, 3, dtype=np.uint32) if isinstance(cdf, str) else cdf
    m = max(min(n * samples, 1 << 16), 1)
    r, t, c = np.full(m, 7, dtype=abi.RAY), np.full(m, 7, dtype=np.float32), np.full((m, 4), 7, dtype=np.float32)
    rc = lib.rb_light_rays_cdf(-1, tab.ctypes.data if emitters else None, None if table is None else table.ctypes.data, n_emit,
                               sf.ctypes.data if surfels else None, ids.ctypes.data if seeds_in else None, n,
                               None if prm is None else prm.ctypes.data, first_sample, samples, r.ctypes.data if rays else None,
                               t.ctypes.data if tmax else None, c.ctypes.data if contrib else None)
    assert (t == 7).all() and (c == 7).all() and (r["_pad0"] == 7).all(), "a refused call wrote its outputs"
    return rc


def _u32(*v):
    return np.array(v, dtype=np.uint32)


BAD_TABLES = [("decreasing", _u32(2, 1)), ("last above 2^24", _u32(1, (1 << 24) + 1)), ("first above the last", _u32(1 << 24, 5)),
              ("wrapped", _u32(0xFFFFFFFF, 0)), ("both above 2^24", _u32(1 << 30, 1 << 31))]


# rb_light_rays' refusals are rb_light_rays_cdf's, with a caller's table and with the table by power.  (The two n_emit cases
# point at a table of two entries; the count is refused before the table is read.)
@pytest.mark.parametrize("cdf", ["ramp", None], ids=["caller's table", "by power"])
@pytest.mark.parametrize("name,kw", REFUSALS, ids=[r[0] for r in REFUSALS])
def test_refusals_before_a_device_is_touched(name, kw, cdf):
    assert _call(cdf=cdf, **kw) == INVALID_OPTIONS, name
    assert _lib.load().rb_last_error(None)


@pytest.mark.parametrize("name,table", BAD_TABLES, ids=[b[0] for b in BAD_TABLES])
def test_bad_host_tables_are_refused(name, table):
    assert _call(cdf=table) == INVALID_OPTIONS, name
    assert _call(cdf=table, n=0) == INVALID_OPTIONS, name   # as bad parameters are: refused in an empty call too
    assert b"cdf" in _lib.load().rb_last_error(None)


def test_null_arguments_and_empty_calls():
    assert _call(params=None) == NULL_ARGUMENT
    assert _call(surfels=False) == NULL_ARGUMENT
    assert _call(rays=False) == NULL_ARGUMENT
    assert _call(tmax=False) == NULL_ARGUMENT
    assert _call(contrib=False) == NULL_ARGUMENT
    assert _call(emitters=False) == NULL_ARGUMENT          # n_emit > 0 without a table
    assert _call(emitters=False, cdf=None) == NULL_ARGUMENT
    assert _call(emitters=False, n=0) == NULL_ARGUMENT
    # n == 0 is RB_OK in every form -- no device is asked for --, and the good edges of a table are taken
    assert _call(n=0) == 0 and _call(n=0, cdf=None) == 0 and _call(n=0, surfels=False, rays=False, tmax=False, contrib=False) == 0
    assert _call(n=0, params=None) == 0 and _call(n=0, n_emit=0, emitters=False) == 0 and _call(n=0, n_emit=0, emitters=False, cdf=None) == 0
    assert _call(n=0, cdf=_u32(0, 0)) == 0 and _call(n=0, cdf=_u32(5, 5)) == 0 and _call(n=0, cdf=_u32(0, 1 << 24)) == 0
    assert _call(n=0, samples=0) == INVALID_OPTIONS and _call(n=0, params=_params(flags=1)) == INVALID_OPTIONS
    lib = _lib.load()
    tab, out = _table(), np.full(2, 7, dtype=np.uint32)
    # rb_emitter_cdf: an empty table is RB_OK; NULL arrays and too long a table are refused, the output unwritten
    assert lib.rb_emitter_cdf(-1, None, 0, None) == 0 and lib.rb_emitter_cdf(-1, tab.ctypes.data, 0, out.ctypes.data) == 0
    assert lib.rb_emitter_cdf(-1, None, 2, out.ctypes.data) == NULL_ARGUMENT
    assert lib.rb_emitter_cdf(-1, tab.ctypes.data, 2, None) == NULL_ARGUMENT
    assert lib.rb_emitter_cdf(-1, tab.ctypes.data, (1 << 24) + 1, out.ctypes.data) == INVALID_OPTIONS
    assert (out == 7).all()
    # the engine forms refuse a NULL engine before they look at anything else
    sf, prm, cdf = _surfels(), _params(), _u32(1, 2)
    rad = np.full(4, 7, dtype=abi.RADIANCE)
    for fn in (lib.rb_direct_light_cdf, lib.rb_direct_light_cdf_device):
        assert fn(None, tab.ctypes.data, cdf.ctypes.data, 2, sf.ctypes.data, None, 4, prm.ctypes.data, 0, 1, rad.ctypes.data) == NULL_ARGUMENT
        assert fn(None, None, cdf.ctypes.data, 2, sf.ctypes.data, None, 4, prm.ctypes.data, 0, 1, rad.ctypes.data) == NULL_ARGUMENT
        assert fn(None, None, None, 0, None, None, 0, None, 0, 0, None) == NULL_ARGUMENT
    assert (rad["weight"] == 7).all()
    count = C.c_size_t(7)
    assert lib.rb_scene_emitter_cdf(None, out.ctypes.data, 2, C.byref(count)) == NULL_ARGUMENT and count.value == 7
    assert lib.rb_scene_emitter_cdf_device(None, None, 0, None) == NULL_ARGUMENT


def test_python_refuses_weights_without_emitters():
    """``pick`` as a table goes with ``emitters``; the check needs no engine state beyond the object"""
    from renderbaby_amd import Engine
    eng = Engine.__new__(Engine)
    pts = np.zeros((2, 3), np.float32)
    with pytest.raises(ValueError, match="pick"):
        Engine.direct_light(eng, pts, pts, 1, pick=_u32(1, 2))
    with pytest.raises(ValueError, match="pick"):
        Engine.direct_light(eng, pts, pts, 1, pick="brightest")


def test_cpp_mirror_compiles(tmp_path):
    src = tmp_path / "c.cpp"
    src.write_text(textwrap.dedent('''
        #include "renderbaby/engine.hpp"
        using namespace renderbaby;
        int use(Engine& e, const rb_surfel* d_surfels, rb_emitter* d_table, uint32_t* d_cdf, uint32_t* d_count, rb_radiance* d_rad) {
            std::vector<rb_surfel> s(3);
            std::vector<rb_emitter> t = e.scene_emitters();
            std::vector<uint32_t> w = e.scene_emitter_cdf();
            std::vector<uint32_t> mine = Engine::emitter_cdf(t, -1);
            std::vector<rb_radiance> a = e.direct_light_cdf(s, 16);
            std::vector<rb_radiance> b = e.direct_light_cdf(s, 16, 7, nullptr, Engine::light_params(), t);
            std::vector<rb_radiance> c = e.direct_light_cdf(s, 16, 7, nullptr, Engine::light_params(), t, mine);
            const rb_light_params p = Engine::light_params();
            e.scene_emitter_cdf_device(d_cdf, 8, d_count);
            e.direct_light_cdf_device(nullptr, nullptr, 0, d_surfels, nullptr, 3, p, d_rad, 16, 7);
            e.direct_light_cdf_device(d_table, nullptr, 8, d_surfels, nullptr, 3, p, d_rad, 16);
            e.direct_light_cdf_device(d_table, d_cdf, 8, d_surfels, nullptr, 3, p, d_rad, 16);
            e.sync();
            return (int)(a.size() + b.size() + c.size() + w.size() + w[0]);
        }
        int main() { return 0; }
    '''))
    lib_dir = os.path.join(ROOT, "renderbaby_amd")
    subprocess.check_call(["g++", "-std=c++17", "-Wall", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(tmp_path / "c"),
                           "-L", lib_dir, "-l:librenderbaby_hip.so", f"-Wl,-rpath,{lib_dir}"])
