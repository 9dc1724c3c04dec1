"""Probe visibility (rb_bake_probe_depth / rb_probe_moments / rb_light_points_visible and their device forms; DESIGN.md section
20), the part that needs no device: the library exports the entry points; rb_probe_depth and rb_light_visibility are what
rb_abi.h states -- seen from a compiled C program and from the Python mirror --; every bad argument is refused before a device
is touched (device = -1: the call would otherwise use the current one) and a NULL engine before anything else; the C++ mirror
compiles."""
import os
import subprocess
import textwrap

import numpy as np
import pytest

from renderbaby_amd import _lib, abi, probes
from tests.test_probe_light_abi import GRID_REFUSALS, INVALID_OPTIONS, LIMIT, NULL_ARGUMENT, _grid

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMBOLS = ("rb_bake_probe_depth", "rb_bake_probe_depth_device", "rb_last_probe_depth_project_ms", "rb_probe_moments",
           "rb_probe_moments_device", "rb_light_points_visible", "rb_light_points_visible_device")
LAYOUT = {"sizeof(rb_probe_depth)": 1024, "offsetof(rb_probe_depth, texel)": 0, "sizeof(((rb_probe_depth*)0)->texel[0])": 16,
          "sizeof(rb_light_visibility)": 16, "offsetof(rb_light_visibility, normal_bias)": 0,
          "offsetof(rb_light_visibility, min_visibility)": 4, "offsetof(rb_light_visibility, flags)": 8,
          "offsetof(rb_light_visibility, _pad)": 12, "RB_VIS_NO_WRAP": 1, "RB_VIS_NO_DEPTH": 2}


def test_library_exports_the_symbols():
    lib = _lib.load()
    for name in SYMBOLS:
        assert name in _lib.EXPORTS
        getattr(lib, name)


def test_layout_and_prototypes_from_a_compiled_c_program(tmp_path):
    lines = [f'printf("{n}=%lu\\n", (unsigned long)({n}));' for n in LAYOUT]
    src = tmp_path / "layout.c"
    src.write_text("#include <stdio.h>\n#include <stddef.h>\n#include \"rb_abi.h\"\nint main(void) {\n" + "\n".join(lines) + "\nreturn 0; }\n")
    exe = tmp_path / "layout"
    subprocess.check_call(["gcc", "-std=c11", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)])
    proto = tmp_path / "proto.c"
    proto.write_text(textwrap.dedent('''
        #include "rb_abi.h"
        int (*f0)(rb_engine*, const rb_probe*, const uint32_t*, size_t, uint32_t, uint32_t, float, rb_probe_depth*) = rb_bake_probe_depth;
        int (*f1)(rb_engine*, const rb_probe*, const uint32_t*, size_t, uint32_t, uint32_t, float, rb_probe_depth*) = rb_bake_probe_depth_device;
        int (*f2)(int32_t, const rb_probe_depth*, size_t, rb_probe_depth*, float*) = rb_probe_moments;
        int (*f3)(rb_engine*, const rb_probe_depth*, size_t, rb_probe_depth*, float*) = rb_probe_moments_device;
        int (*f4)(int32_t, const rb_probe_grid*, const rb_sh9*, const rb_probe_depth*, const rb_surfel*, size_t, const rb_light_visibility*,
                  rb_lit*) = rb_light_points_visible;
        int (*f5)(rb_engine*, const rb_probe_grid*, const rb_sh9*, const rb_probe_depth*, const rb_surfel*, size_t, const rb_light_visibility*,
                  rb_lit*) = rb_light_points_visible_device;
        int (*f6)(rb_engine*, float*) = rb_last_probe_depth_project_ms;
    '''))
    subprocess.check_call(["gcc", "-std=c11", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), "-c", str(proto), "-o", str(tmp_path / "proto.o")])
    got = dict(line.rsplit("=", 1) for line in subprocess.check_output([str(exe)], text=True).splitlines())
    assert {k: int(v) for k, v in got.items()} == LAYOUT


def test_python_mirror_agrees():
    assert abi.PROBE_DEPTH.itemsize == LAYOUT["sizeof(rb_probe_depth)"] == abi.SIZES["probe_depth"][1]
    assert abi.LIGHT_VISIBILITY.itemsize == LAYOUT["sizeof(rb_light_visibility)"] == abi.SIZES["light_visibility"][1]
    assert abi.PROBE_DEPTH.fields["texel"][0].shape == (64, 4)
    for field in ("normal_bias", "min_visibility", "flags", "_pad"):
        assert abi.LIGHT_VISIBILITY.fields[field][1] == LAYOUT[f"offsetof(rb_light_visibility, {field})"], field
    assert (abi.VIS_NO_WRAP, abi.VIS_NO_DEPTH) == (1, 2)
    from renderbaby_amd import Engine, engine
    for name in ("bake_probe_depth", "probe_moments", "light_points_visible", "last_probe_depth_project_ms"):
        assert callable(getattr(Engine, name)), name
    assert callable(engine.probe_moments) and callable(engine.light_points_visible)
    for name in ("oct_texel", "oct_centres", "depth_project", "moments", "light_visible"):
        assert callable(getattr(probes, name)), name
    p = probes.visibility_params(normal_bias=0.25, min_visibility=0.5, wrap=False, depth=False)
    assert p.dtype == abi.LIGHT_VISIBILITY and (p["normal_bias"], p["min_visibility"], p["flags"], p["_pad"]) == (0.25, 0.5, 3, 0)


def _params(**kw):
    p = np.zeros(1, dtype=abi.LIGHT_VISIBILITY)
    for k, v in kw.items():
        p[k] = v
    return p


PARAM_REFUSALS = [
    ("a NaN normal_bias", dict(normal_bias=np.nan)),
    ("an infinite normal_bias", dict(normal_bias=-np.inf)),
    ("a negative min_visibility", dict(min_visibility=-0.001)),
    ("min_visibility above 1", dict(min_visibility=1.001)),
    ("a NaN min_visibility", dict(min_visibility=np.nan)),
    ("an unknown flag bit", dict(flags=4)),
    ("the top flag bit", dict(flags=0x80000001)),
    ("the pad word", dict(_pad=1)),
]


def _visible(fn, first, grid=None, prm=None, m=4, null_grid=False, null_prm=False, coeffs=True, moments=True, points=True, out=True):
    """one call of rb_light_points_visible (first = -1) or its device form (first = NULL); nothing may be written"""
    g = _grid() if grid is None else grid
    p = _params() if prm is None else prm
    co, mom = np.zeros(8, dtype=abi.SH9), np.zeros(8, dtype=abi.PROBE_DEPTH)
    pts, res = np.zeros(4, dtype=abi.SURFEL), np.full(4, 7, dtype=abi.LIT)
    rc = fn(first, None if null_grid else g.ctypes.data, co.ctypes.data if coeffs else None, mom.ctypes.data if moments else None,
            pts.ctypes.data if points else None, m, None if null_prm else p.ctypes.data, res.ctypes.data if out else None)
    assert (res.view(np.float32) == 7).all(), "a refused call wrote its output"
    return rc


@pytest.mark.parametrize("name,kw", PARAM_REFUSALS, ids=[r[0] for r in PARAM_REFUSALS])
def test_parameter_refusals_before_a_device_is_touched(name, kw):
    lib = _lib.load()
    assert _visible(lib.rb_light_points_visible, -1, prm=_params(**kw)) == INVALID_OPTIONS, name
    assert lib.rb_last_error(None)
    assert _visible(lib.rb_light_points_visible, -1, prm=_params(**kw), m=0) == INVALID_OPTIONS, name


def test_the_blend_keeps_rb_light_points_refusals():
    lib = _lib.load()
    lv = lib.rb_light_points_visible
    for name, kw in GRID_REFUSALS:
        assert _visible(lv, -1, _grid(**kw)) == INVALID_OPTIONS, name
    assert _visible(lv, -1, m=LIMIT + 1) == INVALID_OPTIONS and _visible(lv, -1, m=1 << 40) == INVALID_OPTIONS
    assert _visible(lv, -1, null_grid=True) == NULL_ARGUMENT and _visible(lv, -1, null_prm=True) == NULL_ARGUMENT
    assert _visible(lv, -1, null_prm=True, m=0) == NULL_ARGUMENT
    for missing in ("coeffs", "moments", "points", "out"):
        assert _visible(lv, -1, **{missing: False}) == NULL_ARGUMENT, missing
    assert _visible(lv, -1, prm=_params(flags=abi.VIS_NO_WRAP), moments=False) == NULL_ARGUMENT   # the depth test would read them
    assert _visible(lv, -1, m=0) == 0 and _visible(lv, -1, m=0, coeffs=False, moments=False, points=False, out=False) == 0
    for ok in (dict(min_visibility=0.0), dict(min_visibility=1.0), dict(normal_bias=-3e38, flags=3)):
        assert _visible(lv, -1, prm=_params(**ok), m=0) == 0, ok


def test_moments_and_bake_refusals_null_arguments_and_empty_calls():
    lib = _lib.load()
    maps, out, share = np.zeros(2, dtype=abi.PROBE_DEPTH), np.full(2, 7, dtype=abi.PROBE_DEPTH), np.full(2, 7, dtype=np.float32)
    pm = lib.rb_probe_moments
    assert pm(-1, maps.ctypes.data, LIMIT + 1, out.ctypes.data, share.ctypes.data) == INVALID_OPTIONS
    assert pm(-1, maps.ctypes.data, 1 << 40, out.ctypes.data, None) == INVALID_OPTIONS
    assert pm(-1, None, 2, out.ctypes.data, share.ctypes.data) == NULL_ARGUMENT and pm(-1, maps.ctypes.data, 2, None, share.ctypes.data) == NULL_ARGUMENT
    assert pm(-1, maps.ctypes.data, 0, out.ctypes.data, share.ctypes.data) == 0 and pm(-1, None, 0, None, None) == 0
    assert (out.view(np.float32) == 7).all() and (share == 7).all()
    # a NULL engine is refused before anything else, whatever else is wrong with the call
    assert lib.rb_probe_moments_device(None, maps.ctypes.data, 2, out.ctypes.data, None) == NULL_ARGUMENT
    assert lib.rb_probe_moments_device(None, None, 0, None, None) == NULL_ARGUMENT
    ld = lib.rb_light_points_visible_device
    assert _visible(ld, None) == NULL_ARGUMENT and _visible(ld, None, m=0) == NULL_ARGUMENT
    assert _visible(ld, None, prm=_params(flags=8)) == NULL_ARGUMENT and _visible(ld, None, _grid(flags=1)) == NULL_ARGUMENT
    pos = np.zeros(2, dtype=abi.PROBE)
    for fn in (lib.rb_bake_probe_depth, lib.rb_bake_probe_depth_device):
        for reach in (1.0, 0.0, np.nan):
            assert fn(None, pos.ctypes.data, None, 2, 0, 4, reach, out.ctypes.data) == NULL_ARGUMENT
        assert fn(None, None, None, 0, 0, 0, 1.0, None) == NULL_ARGUMENT
    ms = np.full(1, 7, dtype=np.float32)
    assert lib.rb_last_probe_depth_project_ms(None, ms.ctypes.data_as(_lib.C.POINTER(_lib.C.c_float))) == NULL_ARGUMENT and ms[0] == 7
    assert (out.view(np.float32) == 7).all()


def test_cpp_mirror_compiles(tmp_path):
    src = tmp_path / "p.cpp"
    src.write_text(textwrap.dedent('''
        #include "renderbaby/engine.hpp"
        using namespace renderbaby;
        static_assert(sizeof(rb_probe_depth) == 1024 && sizeof(rb_light_visibility) == 16, "layouts");
        float use(Engine& e, const rb_probe* d_probes, rb_probe_depth* d_maps, float* d_share, const rb_sh9* d_coeffs, const rb_surfel* d_points,
                  rb_lit* d_out) {
            rb_probe_grid g{};
            g.step[0] = g.step[1] = g.step[2] = 1.0f;
            g.counts[0] = g.counts[1] = g.counts[2] = 2;
            rb_light_visibility vis{};
            vis.normal_bias = 0.01f;
            vis.flags = RB_VIS_NO_WRAP;
            std::vector<rb_probe_depth> sums = e.bake_probe_depth(std::vector<rb_probe>(8), 64, 2.5f, 0, nullptr);
            std::vector<float> share;
            std::vector<rb_probe_depth> maps = Engine::probe_moments(sums, &share);
            std::vector<rb_lit> lit = Engine::light_points_visible(g, std::vector<rb_sh9>(8), maps, std::vector<rb_surfel>(3), vis, 0);
            e.bake_probe_depth_device(d_probes, nullptr, 8, d_maps, 64, 2.5f);
            e.probe_moments_device(d_maps, 8, d_maps, d_share);
            e.probe_moments_device(d_maps, 8, d_maps);
            e.light_points_visible_device(g, d_coeffs, d_maps, d_points, 3, vis, d_out);
            e.sync();
            return lit[0].value[2] + lit[0].weight + share[0];
        }
    '''))
    subprocess.check_call(["g++", "-std=c++17", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), "-c", str(src), "-o", str(tmp_path / "p.o")])
