"""Hemisphere rays made on the device (rb_hemisphere_rays / rb_trace_hemisphere / rb_openness_hemisphere; DESIGN.md section
16), the part that needs no device: the library exports the five entry points; rb_surfel, rb_hemi_params, rb_openness and
RB_HEMI_PIECE_ITEMS are what rb_abi.h states -- seen from a compiled C program and from the Python mirror --, the C++ mirror
compiles against them, and rb_hemisphere_rays refuses every bad argument before it touches a device (device = -1: the call
would otherwise use the current one)."""
import os
import subprocess
import textwrap

import numpy as np
import pytest

from renderbaby_amd import _lib, abi, hemisphere

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMBOLS = ("rb_hemisphere_rays", "rb_trace_hemisphere", "rb_trace_hemisphere_device", "rb_openness_hemisphere",
           "rb_openness_hemisphere_device")
LAYOUT = {"sizeof(rb_surfel)": 32, "offsetof(rb_surfel, pos)": 0, "offsetof(rb_surfel, _pad0)": 12, "offsetof(rb_surfel, normal)": 16,
          "offsetof(rb_surfel, _pad1)": 28, "offsetof(rb_ray, origin)": 0, "offsetof(rb_ray, dir)": 16,
          "sizeof(rb_hemi_params)": 32, "offsetof(rb_hemi_params, offset)": 0, "offsetof(rb_hemi_params, radius)": 4,
          "offsetof(rb_hemi_params, mask)": 8, "offsetof(rb_hemi_params, flags)": 12, "offsetof(rb_hemi_params, _reserved)": 16,
          "sizeof(rb_openness)": 8, "offsetof(rb_openness, open)": 0, "offsetof(rb_openness, valid)": 4,
          "RB_HEMI_PIECE_ITEMS": 1 << 23, "RB_CAMERA_PIECE_ITEMS": 1 << 23, "RB_MASK_ALL": 15, "RB_MASK_LIGHTS": 8}
MIRROR = {"rb_surfel": abi.SURFEL, "rb_hemi_params": abi.HEMI_PARAMS, "rb_openness": abi.OPENNESS, "rb_ray": abi.RAY}
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
        int (*f0)(int32_t, const rb_surfel*, const uint32_t*, size_t, const rb_hemi_params*, uint32_t, uint32_t, rb_ray*, uint32_t*) = rb_hemisphere_rays;
        int (*f1)(rb_engine*, const rb_surfel*, const uint32_t*, size_t, const rb_hemi_params*, uint32_t, uint32_t, rb_radiance*) = rb_trace_hemisphere;
        int (*f2)(rb_engine*, const rb_surfel*, const uint32_t*, size_t, const rb_hemi_params*, uint32_t, uint32_t, rb_radiance*) = rb_trace_hemisphere_device;
        int (*f3)(rb_engine*, const rb_surfel*, const uint32_t*, size_t, const rb_hemi_params*, uint32_t, uint32_t, rb_openness*) = rb_openness_hemisphere;
        int (*f4)(rb_engine*, const rb_surfel*, const uint32_t*, size_t, const rb_hemi_params*, uint32_t, uint32_t, rb_openness*) = rb_openness_hemisphere_device;
    '''))
    subprocess.check_call(["gcc", "-std=c11", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), "-c", str(proto), "-o", str(tmp_path / "proto.o")])
    got = dict(line.rsplit("=", 1) for line in subprocess.check_output([str(exe)], text=True).splitlines())
    assert {k: int(v) for k, v in got.items()} == LAYOUT


def test_python_mirror_agrees():
    for key, want in LAYOUT.items():
        if key.startswith("sizeof"):
            assert MIRROR[key[7:-1]].itemsize == want, key
        elif key.startswith("offsetof"):
            struct, field = key[9:-1].split(", ")
            assert MIRROR[struct].fields[field][1] == want, key
    assert abi.HEMI_PIECE_ITEMS == LAYOUT["RB_HEMI_PIECE_ITEMS"] == abi.CAMERA_PIECE_ITEMS
    assert abi.HEMI_PIECE_ITEMS // 65536 >= 64   # a piece holds a whole block of 64 surfels at the largest sample count
    assert (abi.MASK_ALL, abi.MASK_LIGHTS) == (LAYOUT["RB_MASK_ALL"], LAYOUT["RB_MASK_LIGHTS"])
    from renderbaby_amd import Engine, aov, bake, engine
    assert callable(Engine.trace_hemisphere) and callable(Engine.openness) and callable(engine.hemisphere_rays_device)
    assert callable(bake.irradiance_device) and callable(aov.ambient_occlusion_device)
    assert callable(hemisphere.frame) and callable(hemisphere.draws) and callable(hemisphere.rays)


def _surfels(n=4):
    return hemisphere.surfels(np.arange(3 * n, dtype=np.float32).reshape(n, 3), np.tile(np.float32([0, 1, 0]), (n, 1)))


def _params(**fields):
    p = np.zeros(1, dtype=abi.HEMI_PARAMS)
    p["offset"] = 1e-3
    for k, v in fields.items():
        p[k][0] = v
    return p


def _call(n=4, first_sample=0, samples=2, params="default", surfels=True, seeds_in=False, rays=True, seeds=True):
    lib = _lib.load()
    prm = _params() if isinstance(params, str) else params
    sf, ids = _surfels(4), np.arange(4, dtype=np.uint32)
    m = max(min(n * samples, 1 << 16), 1)
    r, s = np.full(m, 7, dtype=abi.RAY), np.full(m, 7, dtype=np.uint32)
    rc = lib.rb_hemisphere_rays(-1, sf.ctypes.data if surfels else None, ids.ctypes.data if seeds_in else None, n,
                                None if prm is None else prm.ctypes.data, first_sample, samples,
                                r.ctypes.data if rays else None, s.ctypes.data if seeds else None)
    assert (s == 7).all() and (r["_pad0"] == 7).all(), "a refused call wrote its outputs"
    return rc


REFUSALS = [
    ("samples 0", dict(samples=0)),
    ("samples above 65536", dict(samples=65537)),
    ("first_sample + samples overflows", dict(first_sample=M32, samples=1)),
    ("first_sample + samples overflows by one", dict(first_sample=M32 - 1, samples=2)),
    ("n above 2^31 - 64", dict(n=(1 << 31) - 63, samples=1)),
    ("n far above 2^31", dict(n=1 << 40, samples=1)),
    ("n * samples above 2^31 - 64", dict(n=1 << 15, samples=65536)),
    ("n * samples one above 2^31 - 64", dict(n=((1 << 31) - 64) // 2 + 1, samples=2)),
    ("offset negative", dict(params=_params(offset=-1e-3))),
    ("offset NaN", dict(params=_params(offset=np.nan))),
    ("offset Inf", dict(params=_params(offset=np.inf))),
    ("flags", dict(params=_params(flags=1))),
    ("a high flag bit", dict(params=_params(flags=0x80000000))),
    ("_reserved[0]", dict(params=_params(_reserved=(1, 0, 0, 0)))),
    ("_reserved[3]", dict(params=_params(_reserved=(0, 0, 0, 1)))),
]
# what the engine forms of openness refuse besides (rb_hemisphere_rays reads neither field)
OPENNESS_REFUSALS = [("radius NaN", dict(radius=np.nan)), ("mask above RB_MASK_ALL", dict(mask=16)), ("a high mask bit", dict(mask=0x80000001))]


@pytest.mark.parametrize("name,kw", REFUSALS, ids=[r[0] for r in REFUSALS])
def test_refusals_before_a_device_is_touched(name, kw):
    assert _call(**kw) == INVALID_OPTIONS, name
    assert _lib.load().rb_last_error(None)


def test_null_arguments_and_empty_calls():
    assert abi.ERR[NULL_ARGUMENT] == "NullArgument" and abi.ERR[INVALID_OPTIONS] == "InvalidOptions"
    assert _call(params=None) == NULL_ARGUMENT
    assert _call(surfels=False) == NULL_ARGUMENT
    assert _call(rays=False) == NULL_ARGUMENT
    assert _call(seeds=False) == NULL_ARGUMENT
    # n == 0 is RB_OK, with or without the arrays and the parameters -- and bad parameters are still refused
    assert _call(n=0) == 0 and _call(n=0, surfels=False, rays=False, seeds=False) == 0 and _call(n=0, seeds_in=True) == 0
    assert _call(n=0, params=None) == 0 and _call(n=0, params=None, surfels=False, rays=False, seeds=False) == 0
    assert _call(n=0, samples=0) == INVALID_OPTIONS and _call(n=0, params=_params(flags=2)) == INVALID_OPTIONS
    # the generator reads neither radius nor mask
    assert _call(n=0, params=_params(radius=np.nan, mask=99)) == 0
    # the engine forms refuse a NULL engine before they look at anything else
    lib = _lib.load()
    sf, prm = _surfels(), _params()
    out, cnt = np.zeros(4, dtype=abi.RADIANCE), np.zeros(4, dtype=abi.OPENNESS)
    for fn, o in ((lib.rb_trace_hemisphere, out), (lib.rb_trace_hemisphere_device, out), (lib.rb_openness_hemisphere, cnt),
                  (lib.rb_openness_hemisphere_device, cnt)):
        assert fn(None, sf.ctypes.data, None, 4, prm.ctypes.data, 0, 1, o.ctypes.data) == NULL_ARGUMENT
        assert fn(None, None, None, 0, None, 0, 0, None) == NULL_ARGUMENT


def test_cpp_mirror_compiles(tmp_path):
    src = tmp_path / "c.cpp"
    src.write_text(textwrap.dedent('''
        #include "renderbaby/engine.hpp"
        using namespace renderbaby;
        static_assert(sizeof(rb_surfel) == sizeof(rb_ray) && sizeof(rb_hemi_params) == 32 && sizeof(rb_openness) == 8, "the records");
        static_assert(RB_HEMI_PIECE_ITEMS == (1u << 23), "the piece");
        int use(Engine& e, const rb_surfel* d_surfels, rb_radiance* d_rad, rb_openness* d_open) {
            std::vector<rb_surfel> s(3);
            std::vector<rb_radiance> a = e.trace_hemisphere(s, 16);
            std::vector<rb_radiance> b = e.trace_hemisphere(s, 16, 7, nullptr, 0.0f);
            std::vector<rb_openness> c = e.openness(s, 16, 1.0f);
            const rb_hemi_params p = Engine::hemi_params(1e-3f, 2.0f, RB_MASK_ALL);
            e.trace_hemisphere_device(d_surfels, nullptr, 3, p, d_rad, 16, 7);
            e.openness_device(d_surfels, nullptr, 3, p, d_open, 16);
            e.sync();
            return (int)(a.size() + b.size() + c.size() + c[0].open + c[0].valid);
        }
        int main() { return 0; }
    '''))
    lib_dir = os.path.join(ROOT, "renderbaby_amd")
    subprocess.check_call(["g++", "-std=c++17", "-Wall", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(tmp_path / "c"),
                           "-L", lib_dir, "-l:librenderbaby_hip.so", f"-Wl,-rpath,{lib_dir}"])
