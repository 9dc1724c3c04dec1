"""Direct light at surface points (rb_scene_emitters / rb_light_rays / rb_direct_light), the part that
needs no device: the library exports the six entry points; rb_emitter, rb_light_params and RB_MAX_EMITTERS are what rb_abi.h
states -- seen from a compiled C program and from the Python mirror --, the C++ mirror compiles against them, and rb_light_rays
refuses every bad argument before it touches a device (device = -1: the call would otherwise use the current one)."""
import os
import subprocess
import textwrap

import numpy as np
import pytest

from renderbaby_amd import _lib, abi, direct, hemisphere
from tests.test_hemisphere_abi import REFUSALS as HEMI_REFUSALS

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMBOLS = ("rb_scene_emitters", "rb_scene_emitters_device", "rb_light_rays", "rb_direct_light", "rb_direct_light_device")
LAYOUT = {"sizeof(rb_emitter)": 64, "offsetof(rb_emitter, a)": 0, "offsetof(rb_emitter, kind)": 12, "offsetof(rb_emitter, b)": 16,
          "offsetof(rb_emitter, prim)": 28, "offsetof(rb_emitter, c)": 32, "offsetof(rb_emitter, area)": 44,
          "offsetof(rb_emitter, emissive)": 48, "offsetof(rb_emitter, _pad)": 60,
          "sizeof(rb_light_params)": 32, "offsetof(rb_light_params, offset)": 0, "offsetof(rb_light_params, shorten)": 4,
          "offsetof(rb_light_params, mask)": 8, "offsetof(rb_light_params, flags)": 12, "offsetof(rb_light_params, _reserved)": 16,
          "RB_MAX_EMITTERS": 1 << 24, "RB_HEMI_PIECE_ITEMS": 1 << 23, "RB_HIT_TRIANGLE": 2, "RB_HIT_SPHERE": 3, "RB_HIT_LIGHT": 4,
          "RB_OCCL_VISIBLE": 0}
MIRROR = {"rb_emitter": abi.EMITTER, "rb_light_params": abi.LIGHT_PARAMS}
INVALID_OPTIONS, NULL_ARGUMENT = 18, 15
M32 = 0xFFFFFFFF


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
        int (*f0)(rb_engine*, rb_emitter*, size_t, size_t*) = rb_scene_emitters;
        int (*f1)(rb_engine*, rb_emitter*, size_t, uint32_t*) = rb_scene_emitters_device;
        int (*f2)(int32_t, const rb_emitter*, size_t, const rb_surfel*, const uint32_t*, size_t, const rb_light_params*, uint32_t, uint32_t, rb_ray*,
                  float*, float*) = rb_light_rays;
        int (*f3)(rb_engine*, const rb_emitter*, size_t, const rb_surfel*, const uint32_t*, size_t, const rb_light_params*, uint32_t, uint32_t,
                  rb_radiance*) = rb_direct_light;
        int (*f4)(rb_engine*, const rb_emitter*, size_t, const rb_surfel*, const uint32_t*, size_t, const rb_light_params*, uint32_t, uint32_t,
                  rb_radiance*) = rb_direct_light_device;
    '''))
    subprocess.check_call(["gcc", "-std=c11", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), "-c", str(proto), "-o", str(tmp_path / "proto.o")])
    got = dict(line.rsplit("=", 1) for line in subprocess.check_output([str(exe)], text=True).splitlines())
    assert {k: int(v) for k, v in got.items()} == LAYOUT


def test_python_mirror_agrees():
    for key, want in LAYOUT.items():
        if key.startswith("sizeof"):
            assert MIRROR[key[7:-1]].itemsize == want == abi.SIZES[key[10:-1]][1], key
        elif key.startswith("offsetof"):
            struct, field = key[9:-1].split(", ")
            assert MIRROR[struct].fields[field][1] == want, key
    assert abi.MAX_EMITTERS == LAYOUT["RB_MAX_EMITTERS"] and float(np.float32(abi.MAX_EMITTERS)) == abi.MAX_EMITTERS
    assert (abi.HIT_TRIANGLE, abi.HIT_SPHERE, abi.HIT_LIGHT) == (2, 3, 4) == direct.KINDS
    from renderbaby_amd import Engine, _marshal, bake, engine
    assert callable(Engine.scene_emitters) and callable(Engine.direct_light) and callable(engine.light_rays)
    assert callable(bake.direct_irradiance) and callable(bake.lightmap_direct)
    assert callable(direct.scene_emitters) and callable(direct.rays) and callable(direct.fold)
    assert _marshal.layout(abi.EMITTER) == (np.dtype(np.float32), 16)
    p = direct.params()
    assert p["offset"][0] == np.float32(1e-3) and p["shorten"][0] == np.float32(1e-3) and p["mask"][0] == abi.MASK_ALL and not p["flags"][0]


def _surfels(n=4):
    return hemisphere.surfels(np.arange(3 * n, dtype=np.float32).reshape(n, 3), np.tile(np.float32([0, 1, 0]), (n, 1)))


def _table(n=2):
    e = np.zeros(n, dtype=abi.EMITTER)
    e["kind"], e["a"], e["b"], e["area"], e["emissive"] = abi.HIT_SPHERE, (0, 5, 0), (1, 0, 0), 12.566371, (1, 1, 1)
    return e


def _params(**fields):
    p = np.zeros(1, dtype=abi.LIGHT_PARAMS)
    p["offset"], p["shorten"], p["mask"] = 1e-3, 1e-3, abi.MASK_ALL
    for k, v in fields.items():
        p[k][0] = v
    return p


def _call(n=4, first_sample=0, samples=2, params="default", n_emit=2, emitters=True, surfels=True, seeds_in=False, rays=True, tmax=True, contrib=True):
    lib = _lib.load()
    prm = _params() if isinstance(params, str) else params
    sf, ids, tab = _surfels(4), np.arange(4, dtype=np.uint32), _table()
    m = max(min(n * samples, 1 << 16), 1)
    r, t, c = np.full(m, 7, dtype=abi.RAY), np.full(m, 7, dtype=np.float32), np.full((m, 4), 7, dtype=np.float32)
    rc = lib.rb_light_rays(-1, tab.ctypes.data if emitters else None, n_emit, sf.ctypes.data if surfels else None,
                           ids.ctypes.data if seeds_in else None, n, None if prm is None else prm.ctypes.data, first_sample, samples,
                           r.ctypes.data if rays else None, t.ctypes.data if tmax else None, c.ctypes.data if contrib else None)
    assert (t == 7).all() and (c == 7).all() and (r["_pad0"] == 7).all(), "a refused call wrote its outputs"
    return rc


def _light_fields(kw):
    """a refusal of rb_hemisphere_rays as one of rb_light_rays: its rb_hemi_params fields carried over"""
    kw = dict(kw)
    if "params" in kw:
        h = kw["params"]
        kw["params"] = _params(offset=h["offset"][0], flags=h["flags"][0], _reserved=tuple(h["_reserved"][0]))
    return kw


# rb_openness_hemisphere's list -- what rb_hemisphere_rays refuses, and a mask above RB_MASK_ALL in the engine forms --, plus:
REFUSALS = [(name, _light_fields(kw)) for name, kw in HEMI_REFUSALS] + [
    ("shorten negative", dict(params=_params(shorten=-1e-6))),
    ("shorten above 0.5", dict(params=_params(shorten=np.nextafter(np.float32(0.5), np.float32(1))))),
    ("shorten NaN", dict(params=_params(shorten=np.nan))),
    ("shorten Inf", dict(params=_params(shorten=np.inf))),
    ("shorten -Inf", dict(params=_params(shorten=-np.inf))),
    ("n_emit above 2^24", dict(n_emit=(1 << 24) + 1)),
    ("n_emit far above 2^24", dict(n_emit=1 << 40)),
]
MASK_REFUSALS = [("mask above RB_MASK_ALL", dict(mask=16)), ("a high mask bit", dict(mask=0x80000001))]


@pytest.mark.parametrize("name,kw", REFUSALS, ids=[r[0] for r in REFUSALS])
def test_refusals_before_a_device_is_touched(name, kw):
    assert _call(**kw) == INVALID_OPTIONS, name
    assert _lib.load().rb_last_error(None)


def test_null_arguments_and_empty_calls():
    assert len(REFUSALS) == len(HEMI_REFUSALS) + 7
    assert _call(params=None) == NULL_ARGUMENT
    assert _call(surfels=False) == NULL_ARGUMENT
    assert _call(rays=False) == NULL_ARGUMENT
    assert _call(tmax=False) == NULL_ARGUMENT
    assert _call(contrib=False) == NULL_ARGUMENT
    assert _call(emitters=False) == NULL_ARGUMENT          # n_emit > 0 without a table
    assert _call(emitters=False, n=0) == NULL_ARGUMENT
    # the edges of shorten are taken: the refusal is not theirs (n == 0: no device is asked for)
    assert _call(n=0, params=_params(shorten=0.0)) == 0 and _call(n=0, params=_params(shorten=0.5)) == 0 and _call(n=0, params=_params(shorten=-0.0)) == 0
    assert _call(n=0, n_emit=1 << 24) == 0
    # n == 0 is RB_OK, with or without the arrays and the parameters -- and bad parameters are still refused
    assert _call(n=0) == 0 and _call(n=0, surfels=False, rays=False, tmax=False, contrib=False) == 0 and _call(n=0, seeds_in=True) == 0
    assert _call(n=0, params=None) == 0 and _call(n=0, n_emit=0, emitters=False) == 0
    assert _call(n=0, samples=0) == INVALID_OPTIONS and _call(n=0, params=_params(flags=2)) == INVALID_OPTIONS
    assert _call(n=0, params=_params(shorten=0.75)) == INVALID_OPTIONS
    # the generator reads no mask
    assert _call(n=0, params=_params(mask=99)) == 0
    # the engine forms refuse a NULL engine before they look at anything else
    lib = _lib.load()
    sf, prm, tab = _surfels(), _params(), _table()
    out = np.zeros(4, dtype=abi.RADIANCE)
    for fn in (lib.rb_direct_light, lib.rb_direct_light_device):
        assert fn(None, tab.ctypes.data, 2, sf.ctypes.data, None, 4, prm.ctypes.data, 0, 1, out.ctypes.data) == NULL_ARGUMENT
        assert fn(None, None, 0, None, None, 0, None, 0, 0, None) == NULL_ARGUMENT
    import ctypes as C
    count = C.c_size_t(7)
    assert lib.rb_scene_emitters(None, tab.ctypes.data, 2, C.byref(count)) == NULL_ARGUMENT and count.value == 7
    assert lib.rb_scene_emitters_device(None, None, 0, None) == NULL_ARGUMENT


def test_cpp_mirror_compiles(tmp_path):
    src = tmp_path / "c.cpp"
    src.write_text(textwrap.dedent('''
        #include "renderbaby/engine.hpp"
        using namespace renderbaby;
        static_assert(sizeof(rb_emitter) == 64 && sizeof(rb_light_params) == 32, "the records");
        static_assert(RB_MAX_EMITTERS == (1u << 24), "the table");
        int use(Engine& e, const rb_surfel* d_surfels, rb_emitter* d_table, uint32_t* d_count, rb_radiance* d_rad) {
            std::vector<rb_surfel> s(3);
            std::vector<rb_emitter> t = e.scene_emitters();
            std::vector<rb_radiance> a = e.direct_light(s, 16);
            std::vector<rb_radiance> b = e.direct_light(s, 16, 7, nullptr, Engine::light_params(0.0f, 0.01f, RB_MASK_ALL & ~RB_MASK_LIGHTS), t);
            const rb_light_params p = Engine::light_params();
            e.scene_emitters_device(d_table, 8, d_count);
            e.direct_light_device(nullptr, 0, d_surfels, nullptr, 3, p, d_rad, 16, 7);
            e.direct_light_device(d_table, 8, d_surfels, nullptr, 3, p, d_rad, 16);
            e.sync();
            return (int)(a.size() + b.size() + t.size() + t[0].kind + t[0].prim);
        }
        int main() { return 0; }
    '''))
    lib_dir = os.path.join(ROOT, "renderbaby_amd")
    subprocess.check_call(["g++", "-std=c++17", "-Wall", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(tmp_path / "c"),
                           "-L", lib_dir, "-l:librenderbaby_hip.so", f"-Wl,-rpath,{lib_dir}"])
