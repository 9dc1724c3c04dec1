"""Lightmap texels made on the device (rb_lightmap_surfels / rb_lightmap_resolve / rb_bake_lightmap), the
part that needs no device: the library exports the six entry points; rb_lightmap_params and the constants are what rb_abi.h
states -- seen from a compiled C program and from the Python mirror --, the C++ mirror compiles against them, and the engine-less
forms refuse every bad argument before they touch a device (device = -1: the call would otherwise use the current one)."""
import os
import subprocess
import textwrap

import numpy as np
import pytest

from renderbaby_amd import _lib, abi, lightmap

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMBOLS = ("rb_lightmap_surfels", "rb_lightmap_surfels_device", "rb_lightmap_resolve", "rb_bake_lightmap", "rb_bake_lightmap_device",
           "rb_last_lightmap_ms")
LAYOUT = {"sizeof(rb_lightmap_params)": 32, "offsetof(rb_lightmap_params, width)": 0, "offsetof(rb_lightmap_params, height)": 4,
          "offsetof(rb_lightmap_params, mesh)": 8, "offsetof(rb_lightmap_params, flags)": 12, "offsetof(rb_lightmap_params, offset)": 16,
          "offsetof(rb_lightmap_params, dilate)": 20, "offsetof(rb_lightmap_params, _reserved)": 24,
          "RB_LIGHTMAP_ALL_MESHES": 0xFFFFFFFF, "RB_LIGHTMAP_NO_OWNER": 0xFFFFFFFF, "RB_LIGHTMAP_FLIP": 1,
          "RB_LIGHTMAP_MAX_SIDE": 16384, "RB_LIGHTMAP_MAX_DILATE": 64, "sizeof(rb_surfel)": 32, "sizeof(rb_radiance)": 16}
INVALID_OPTIONS, NULL_ARGUMENT = 18, 15


def test_library_exports_the_symbols():
    lib = _lib.load()
    for name in SYMBOLS:
        assert name in _lib.EXPORTS
        getattr(lib, name)


def test_layout_and_constants_from_a_compiled_c_program(tmp_path):
    lines = [f'printf("{n}=%lu\\n", (unsigned long)({n}));' for n in LAYOUT]
    src = tmp_path / "layout.c"
    src.write_text("#include <stdio.h>\n#include <stddef.h>\n#include \"rb_abi.h\"\nint main(void) {\n" + "\n".join(lines) + "\nreturn 0; }\n")
    exe = tmp_path / "layout"
    subprocess.check_call(["gcc", "-std=c11", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)])
    proto = tmp_path / "proto.c"
    proto.write_text(textwrap.dedent('''
        #include "rb_abi.h"
        int (*f0)(int32_t, const rb_gpu_triangle*, size_t, const float*, size_t, const rb_lightmap_params*, rb_surfel*, uint32_t*) = rb_lightmap_surfels;
        int (*f1)(rb_engine*, const rb_lightmap_params*, rb_surfel*, uint32_t*) = rb_lightmap_surfels_device;
        int (*f2)(int32_t, uint32_t, uint32_t, const rb_radiance*, uint32_t, float*) = rb_lightmap_resolve;
        int (*f3)(rb_engine*, const rb_lightmap_params*, uint32_t, uint32_t, float*, rb_radiance*) = rb_bake_lightmap;
        int (*f4)(rb_engine*, const rb_lightmap_params*, uint32_t, uint32_t, float*, rb_radiance*) = rb_bake_lightmap_device;
        int (*f5)(rb_engine*, float*, float*) = rb_last_lightmap_ms;
    '''))
    subprocess.check_call(["gcc", "-std=c11", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), "-c", str(proto), "-o", str(tmp_path / "proto.o")])
    got = dict(line.rsplit("=", 1) for line in subprocess.check_output([str(exe)], text=True).splitlines())
    assert {k: int(v) for k, v in got.items()} == LAYOUT


def test_python_mirror_agrees():
    for key, want in LAYOUT.items():
        if key.startswith("offsetof(rb_lightmap_params"):
            assert abi.LIGHTMAP_PARAMS.fields[key[9:-1].split(", ")[1]][1] == want, key
    assert abi.LIGHTMAP_PARAMS.itemsize == LAYOUT["sizeof(rb_lightmap_params)"] == abi.SIZES["lightmap_params"][1]
    assert (abi.LIGHTMAP_ALL_MESHES, abi.LIGHTMAP_NO_OWNER, abi.LIGHTMAP_FLIP) == (0xFFFFFFFF, 0xFFFFFFFF, 1)
    assert (abi.LIGHTMAP_MAX_SIDE, abi.LIGHTMAP_MAX_DILATE) == (LAYOUT["RB_LIGHTMAP_MAX_SIDE"], LAYOUT["RB_LIGHTMAP_MAX_DILATE"])
    assert lightmap.NO_OWNER == LAYOUT["RB_LIGHTMAP_NO_OWNER"]
    from renderbaby_amd import Engine, engine
    assert callable(Engine.lightmap_surfels) and callable(Engine.bake_lightmap) and callable(Engine.last_lightmap_ms)
    assert callable(engine.lightmap_surfels_device) and callable(engine.lightmap_resolve)
    for name in ("texel_space", "edge", "owners", "surfels", "resolve"):
        assert callable(getattr(lightmap, name))


def _params(**fields):
    p = np.zeros(1, dtype=abi.LIGHTMAP_PARAMS)
    p["width"], p["height"], p["mesh"], p["offset"], p["dilate"] = 4, 3, abi.LIGHTMAP_ALL_MESHES, 1e-3, 2
    for k, v in fields.items():
        p[k][0] = v
    return p


def _surfels(params="default", n_tris=2, tris=True, n_uvs=12, uvs=True, out=True, owners=True):
    """rb_lightmap_surfels on device -1 with arrays large enough for a 4 x 3 atlas; a refused call must leave them alone"""
    lib = _lib.load()
    prm = _params() if isinstance(params, str) else params
    t, uv = np.zeros(2, dtype=abi.GPU_TRIANGLE), np.zeros(12, dtype=np.float32)
    s, o = np.full(12, 7, dtype=np.uint32).repeat(8).view(abi.SURFEL), np.full(12, 7, dtype=np.uint32)
    rc = lib.rb_lightmap_surfels(-1, t.ctypes.data if tris else None, n_tris, uv.ctypes.data if uvs else None, n_uvs,
                                 None if prm is None else prm.ctypes.data, s.ctypes.data if out else None, o.ctypes.data if owners else None)
    return rc, s, o


def _resolve(width=4, height=3, dilate=2, sums=True, out=True):
    lib = _lib.load()
    s, o = np.zeros(12, dtype=abi.RADIANCE), np.full(48, 7, dtype=np.float32)
    rc = lib.rb_lightmap_resolve(-1, width, height, s.ctypes.data if sums else None, dilate, o.ctypes.data if out else None)
    assert (o == 7).all(), "a refused call wrote its output"
    return rc


REFUSALS = [
    ("width 0", dict(width=0)),
    ("height 0", dict(height=0)),
    ("width above 16384", dict(width=16385)),
    ("height above 16384", dict(height=16385)),
    ("width far above", dict(width=0xFFFFFFFF)),
    ("dilate above 64", dict(dilate=65)),
    ("an unknown flag", dict(flags=2)),
    ("a high flag bit", dict(flags=0x80000001)),
    ("_reserved[0]", dict(_reserved=(1, 0))),
    ("_reserved[1]", dict(_reserved=(0, 1))),
    ("offset negative", dict(offset=-1e-3)),
    ("offset NaN", dict(offset=np.nan)),
    ("offset Inf", dict(offset=np.inf)),
]


@pytest.mark.parametrize("name,fields", REFUSALS, ids=[r[0] for r in REFUSALS])
def test_surfels_refusals_before_a_device_is_touched(name, fields):
    rc, s, o = _surfels(params=_params(**fields))
    assert rc == INVALID_OPTIONS, name
    assert _lib.load().rb_last_error(None)
    assert (s.view(np.uint32) == 7).all() and (o == 7).all(), "a refused call wrote its outputs"


def test_surfels_null_arguments_and_the_empty_scene():
    assert abi.ERR[NULL_ARGUMENT] == "NullArgument" and abi.ERR[INVALID_OPTIONS] == "InvalidOptions"
    assert _surfels(params=None)[0] == NULL_ARGUMENT
    assert _surfels(out=False)[0] == NULL_ARGUMENT
    assert _surfels(tris=False)[0] == NULL_ARGUMENT
    assert _surfels(uvs=False)[0] == NULL_ARGUMENT
    assert _surfels(n_tris=(1 << 31) - 63)[0] == INVALID_OPTIONS and _surfels(n_uvs=1 << 32)[0] == INVALID_OPTIONS
    # n_tris == 0 is RB_OK with an all-empty map -- no device is needed to say so --, and bad parameters are still refused
    for kw in (dict(n_tris=0), dict(n_tris=0, tris=False, n_uvs=0, uvs=False), dict(n_tris=0, owners=False)):
        rc, s, o = _surfels(**kw)
        assert rc == 0 and (s.view(np.uint32) == 0).all()
        assert (o == (7 if kw.get("owners") is False else abi.LIGHTMAP_NO_OWNER)).all()
    assert _surfels(n_tris=0, params=_params(width=0))[0] == INVALID_OPTIONS
    # the engine forms refuse a NULL engine before they look at anything else
    lib = _lib.load()
    prm, buf = _params(), np.zeros(64, dtype=np.float32)
    assert lib.rb_lightmap_surfels_device(None, prm.ctypes.data, buf.ctypes.data, None) == NULL_ARGUMENT
    assert lib.rb_bake_lightmap(None, prm.ctypes.data, 0, 1, buf.ctypes.data, None) == NULL_ARGUMENT
    assert lib.rb_bake_lightmap_device(None, None, 0, 0, None, None) == NULL_ARGUMENT
    assert lib.rb_last_lightmap_ms(None, None, None) == NULL_ARGUMENT


def test_resolve_refusals_before_a_device_is_touched():
    for kw in (dict(width=0), dict(height=0), dict(width=16385), dict(height=16385), dict(width=0xFFFFFFFF, height=0xFFFFFFFF), dict(dilate=65),
               dict(dilate=0xFFFFFFFF)):
        assert _resolve(**kw) == INVALID_OPTIONS, kw
        assert _lib.load().rb_last_error(None)
    assert _resolve(sums=False) == NULL_ARGUMENT and _resolve(out=False) == NULL_ARGUMENT


def test_cpp_mirror_compiles(tmp_path):
    src = tmp_path / "c.cpp"
    src.write_text(textwrap.dedent('''
        #include "renderbaby/engine.hpp"
        using namespace renderbaby;
        static_assert(sizeof(rb_lightmap_params) == 32 && RB_LIGHTMAP_FLIP == 1u, "the record");
        int use(Engine& e, rb_surfel* d_surfels, uint32_t* d_owners, float* d_rgba, rb_radiance* d_sums) {
            const rb_lightmap_params p = Engine::lightmap_params(64, 32, 0, true, 1e-3f, 2);
            std::vector<rb_radiance> sums;
            std::vector<float> a = e.bake_lightmap(p, 16, 0, &sums);
            std::vector<float> b = e.bake_lightmap(Engine::lightmap_params(8, 8), 4);
            e.lightmap_surfels_device(p, d_surfels, d_owners);
            e.lightmap_surfels_device(p, d_surfels);
            e.bake_lightmap_device(p, d_rgba, d_sums, 16, 7);
            e.sync();
            return (int)(a.size() + b.size() + sums.size());
        }
        int main() { return 0; }
    '''))
    lib_dir = os.path.join(ROOT, "renderbaby_amd")
    subprocess.check_call(["g++", "-std=c++17", "-Wall", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(tmp_path / "c"),
                           "-L", lib_dir, "-l:librenderbaby_hip.so", f"-Wl,-rpath,{lib_dir}"])
