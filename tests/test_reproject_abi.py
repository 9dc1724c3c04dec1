"""The temporal reprojection's ABI, the part that needs no device: the library exports the entry points,
rb_view and rb_reproject_params have the stated sizes and offsets -- seen from a compiled C program, from ctypes and from the
numpy mirror --, the C++ mirror compiles against them, the defaults are the model's, every refusal of the engine-less form
happens before anything touches a device, and rb_view_from_camera equals the model bit for bit."""
import ctypes as C
import os
import subprocess
import textwrap

import numpy as np
import pytest

from renderbaby_amd import Engine, _lib, abi, engine, temporal

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMBOLS = ("rb_view_from_camera", "rb_reproject_default_params", "rb_reproject_buffers", "rb_reproject_device", "rb_denoise_history",
           "rb_denoise_history_device", "rb_history_read", "rb_history_reset", "rb_last_reproject_ms")
LAYOUT = {"sizeof(rb_view)": 64, "sizeof(rb_reproject_params)": 32,
          "offsetof(rb_view, pos)": 0, "offsetof(rb_view, cx)": 12, "offsetof(rb_view, right)": 16, "offsetof(rb_view, cy)": 28,
          "offsetof(rb_view, up)": 32, "offsetof(rb_view, sx)": 44, "offsetof(rb_view, fwd)": 48, "offsetof(rb_view, sy)": 60,
          "offsetof(rb_reproject_params, sigma_depth)": 0, "offsetof(rb_reproject_params, normal_min)": 4,
          "offsetof(rb_reproject_params, albedo_floor)": 8, "offsetof(rb_reproject_params, max_history)": 12,
          "offsetof(rb_reproject_params, flags)": 16, "offsetof(rb_reproject_params, _reserved)": 20}
NULL_ARGUMENT, INVALID_OPTIONS = 15, 18


class View(C.Structure):
    _fields_ = [("pos", C.c_float * 3), ("cx", C.c_float), ("right", C.c_float * 3), ("cy", C.c_float), ("up", C.c_float * 3),
                ("sx", C.c_float), ("fwd", C.c_float * 3), ("sy", C.c_float)]


class ReprojectParams(C.Structure):
    _fields_ = [("sigma_depth", C.c_float), ("normal_min", C.c_float), ("albedo_floor", C.c_float), ("max_history", C.c_float),
                ("flags", C.c_uint32), ("_reserved", C.c_uint32 * 3)]


def test_library_exports_the_symbols():
    lib = _lib.load()
    for name in SYMBOLS:
        assert name in _lib.EXPORTS
        getattr(lib, name)


def test_layouts_from_a_compiled_c_program(tmp_path):
    lines = [f'printf("{n}=%u\\n", (unsigned){n});' for n in LAYOUT]
    src = tmp_path / "layout.c"
    src.write_text("#include <stdio.h>\n#include <stddef.h>\n#include \"rb_abi.h\"\nint main(void) {\n" + "\n".join(lines) + "\nreturn 0; }\n")
    exe = tmp_path / "layout"
    subprocess.check_call(["gcc", "-std=c11", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)])
    proto = tmp_path / "proto.c"
    proto.write_text(textwrap.dedent('''
        #include "rb_abi.h"
        int (*f0)(const rb_camera*, uint32_t, uint32_t, rb_view*) = rb_view_from_camera;
        int (*f1)(rb_reproject_params*) = rb_reproject_default_params;
        int (*f2)(int32_t, const rb_reproject_params*, uint32_t, uint32_t, const rb_view*, const float*, const rb_guide*, const rb_guide*,
                  const float*, float*) = rb_reproject_buffers;
        int (*f3)(rb_engine*, const rb_reproject_params*, uint32_t, uint32_t, const rb_view*, const float*, const rb_guide*, const rb_guide*,
                  const float*, float*) = rb_reproject_device;
        int (*f4)(rb_engine*, const rb_reproject_params*, const rb_denoise_params*, uint8_t*, float*) = rb_denoise_history;
        int (*f5)(rb_engine*, const rb_reproject_params*, const rb_denoise_params*, uint8_t*, float*) = rb_denoise_history_device;
        int (*f6)(rb_engine*, float*) = rb_history_read;
        int (*f7)(rb_engine*) = rb_history_reset;
        int (*f8)(rb_engine*, float*) = rb_last_reproject_ms;
    '''))
    subprocess.check_call(["gcc", "-std=c11", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), "-c", str(proto), "-o", str(tmp_path / "proto.o")])
    got = dict(line.rsplit("=", 1) for line in subprocess.check_output([str(exe)], text=True).splitlines())
    assert {k: int(v) for k, v in got.items()} == LAYOUT


def test_ctypes_and_numpy_mirrors_agree():
    assert C.sizeof(View) == abi.VIEW.itemsize == 64 and C.sizeof(ReprojectParams) == abi.REPROJECT_PARAMS.itemsize == 32
    assert abi.FRAME_RECORD.itemsize == 16 and abi.SIZES["view"] == (abi.VIEW, 64) and abi.SIZES["reproject_params"] == (abi.REPROJECT_PARAMS, 32)
    for key, want in LAYOUT.items():
        if key.startswith("offsetof"):
            struct, field = key[len("offsetof("):-1].split(", ")
            dt, ct = (abi.VIEW, View) if struct == "rb_view" else (abi.REPROJECT_PARAMS, ReprojectParams)
            assert dt.fields[field][1] == want == getattr(ct, field).offset, key
    for name in ("reproject", "denoise_history", "history", "history_reset", "last_reproject_ms"):
        assert callable(getattr(Engine, name))
    for name in ("view_from_camera", "reproject_defaults", "reproject_buffers"):
        assert callable(getattr(engine, name))
    for name in ("view_from_camera", "default_params", "params", "check_params", "reproject", "merge"):
        assert callable(getattr(temporal, name))


def test_defaults_are_the_models_and_the_issues():
    d = engine.reproject_defaults()
    assert d.tobytes() == temporal.default_params().tobytes()
    temporal.check_params(d)
    assert [d[k] for k in ("sigma_depth", "normal_min", "albedo_floor", "max_history")] == [np.float32(0.02), np.float32(0.9), np.float32(0.01), np.float32(32)]
    assert int(d["flags"]) == 0 and not d["_reserved"].any()
    p = ReprojectParams()
    assert _lib.load().rb_reproject_default_params(C.byref(p)) == 0 and bytes(p) == d.tobytes()
    assert _lib.load().rb_reproject_default_params(None) == NULL_ARGUMENT


def _args(n=1):
    p = np.ascontiguousarray(temporal.default_params()).reshape(1)
    v = np.zeros(1, abi.VIEW)
    v["right"], v["up"], v["fwd"], v["sx"], v["sy"] = (1, 0, 0), (0, 1, 0), (0, 0, 1), 1, 1
    prev4, out4, cur4 = np.full((n, 4), 2.0, np.float32), np.full((n, 4), 7.0, np.float32), np.full((n, 4), 1.0, np.float32)
    g = np.zeros(n, abi.GUIDE)
    return p, v, prev4, g, cur4, out4


def test_every_refusal_comes_before_a_device_is_touched():
    """(this machine has no device: a call that got as far as one would fail with another code)"""
    lib = _lib.load()
    p, v, prev4, g, cur4, out4 = _args()

    def call(p=p, w=1, h=1, v=v, prev4=prev4, pg=g, cg=g, cur4=cur4, out4=out4, device=-1):
        ptr = lambda a: None if a is None else a.ctypes.data   # noqa: E731
        return lib.rb_reproject_buffers(device, ptr(p), w, h, ptr(v), ptr(prev4), ptr(pg), ptr(cg), ptr(cur4), ptr(out4))
    for kw in (dict(p=None), dict(v=None), dict(prev4=None), dict(pg=None), dict(cg=None), dict(out4=None)):
        assert call(**kw) == NULL_ARGUMENT, kw
    for kw in (dict(sigma_depth=0.0), dict(sigma_depth=-1.0), dict(sigma_depth=np.nan), dict(sigma_depth=np.inf), dict(normal_min=1.5),
               dict(normal_min=-1.5), dict(normal_min=np.nan), dict(albedo_floor=0.0), dict(albedo_floor=np.inf), dict(max_history=0.5),
               dict(max_history=np.inf), dict(max_history=np.nan), dict(flags=1), dict(_reserved=(0, 0, 1)), dict(_reserved=(1, 0, 0))):
        bad = np.ascontiguousarray(temporal.params(**kw)).reshape(1)
        assert call(p=bad) == INVALID_OPTIONS, kw
        with pytest.raises(ValueError):
            temporal.check_params(bad[0])
    assert b"max_history" in lib.rb_last_error(None) or b"reserved" in lib.rb_last_error(None)
    for field in ("pos", "right", "up", "fwd", "cx", "cy", "sx", "sy"):
        for value in (np.nan, np.inf):
            bad = v.copy()
            if bad[field].ndim > 1:
                bad[field][0, 1] = value
            else:
                bad[field] = value
            assert call(v=bad) == INVALID_OPTIONS, (field, value)
    assert call(w=1 << 16, h=1 << 15) == INVALID_OPTIONS   # w * h = 2^31
    assert call(w=0xFFFFFFFF, h=0xFFFFFFFF) == INVALID_OPTIONS
    # an empty frame is nothing to do -- once the arguments are there and valid
    assert call(w=0, h=5) == 0 and call(w=5, h=0) == 0 and call(w=0, h=0, cur4=None) == 0
    assert call(w=0, h=5, out4=None) == NULL_ARGUMENT
    assert (out4 == 7.0).all()
    # the engine forms: a NULL handle
    assert lib.rb_reproject_device(None, p.ctypes.data, 1, 1, v.ctypes.data, prev4.ctypes.data, g.ctypes.data, g.ctypes.data, None, out4.ctypes.data) == NULL_ARGUMENT
    dp = np.ascontiguousarray(engine.denoise_defaults()).reshape(1)
    rgba = (C.c_uint8 * 4)(7, 7, 7, 7)
    assert lib.rb_denoise_history(None, p.ctypes.data, dp.ctypes.data, rgba, None) == NULL_ARGUMENT
    assert lib.rb_denoise_history_device(None, p.ctypes.data, dp.ctypes.data, rgba, None) == NULL_ARGUMENT
    ms = C.c_float(5.0)
    assert lib.rb_history_read(None, out4.ctypes.data) == NULL_ARGUMENT and lib.rb_history_reset(None) == NULL_ARGUMENT
    assert lib.rb_last_reproject_ms(None, C.byref(ms)) == NULL_ARGUMENT and ms.value == 5.0 and list(rgba) == [7] * 4
    assert lib.rb_view_from_camera(None, 4, 4, v.ctypes.data) == NULL_ARGUMENT
    assert lib.rb_view_from_camera(np.zeros(1, abi.CAMERA).ctypes.data, 4, 4, None) == NULL_ARGUMENT


def _cameras():
    rng = np.random.Generator(np.random.PCG64(11))
    dirs = [(0, 0, -1), (0, 1, 0), (0, -1, 0), (1, 0, 0), (0.3, -0.2, -0.9), (1e-20, 0, 1e-20)] + [tuple(rng.normal(0, 1, 3)) for _ in range(4)]
    cams = np.zeros(len(dirs), abi.CAMERA)
    cams["dir"] = np.asarray(dirs, np.float32)
    cams["pos"] = rng.normal(0, 5, (len(dirs), 3)).astype(np.float32)
    cams["pane_distance"] = rng.uniform(0.5, 2.0, len(dirs)).astype(np.float32)
    cams["pane_width"] = rng.uniform(0.5, 3.0, len(dirs)).astype(np.float32)
    return cams


def test_view_from_camera_equals_the_model_bit_for_bit():
    cams = _cameras()
    assert len(cams) == 10
    finite = []
    for i, cam in enumerate(cams):
        for w in (1, 2, 33, 1920):
            for h in (1, 2, 33, 1920):
                got, want = engine.view_from_camera(cam, w, h), temporal.view_from_camera(cam, w, h)
                same = np.array_equal(np.frombuffer(got.tobytes(), np.uint32), np.frombuffer(want.tobytes(), np.uint32))
                # (a NaN the arithmetic generates has no fixed sign or payload: section 13's exception)
                a, b = np.frombuffer(got.tobytes(), np.float32), np.frombuffer(want.tobytes(), np.float32)
                assert same or (np.array_equal(np.isnan(a), np.isnan(b)) and np.array_equal(a[~np.isnan(a)].view(np.uint32), b[~np.isnan(b)].view(np.uint32))), (i, w, h, got, want)
                finite.append(bool(np.isfinite(a).all()))
    # dir along y, up or down, has no basis: its views are not finite; the others are
    per_cam = np.asarray(finite).reshape(10, 16)
    assert not per_cam[1].any() and not per_cam[2].any() and per_cam[[0, 3, 4, 6, 7, 8, 9]].all()
    # a uniforms record brings its own size
    from renderbaby_amd import scenes
    u = scenes.cornell(width=33, height=17).uniforms
    assert engine.view_from_camera(u).tobytes() == temporal.view_from_camera(u).tobytes() == engine.view_from_camera(u["camera"][0], 33, 17).tobytes()


def test_cpp_mirror_compiles(tmp_path):
    src = tmp_path / "r.cpp"
    src.write_text(textwrap.dedent('''
        #include "renderbaby/engine.hpp"
        using namespace renderbaby;
        static_assert(sizeof(rb_view) == 64 && sizeof(rb_reproject_params) == 32, "layouts");
        int use(Engine& e, const rb_camera& cam, uint8_t* d_rgba, float* d_a, rb_guide* d_g) {
            rb_reproject_params rp = Engine::reproject_defaults();
            rb_view v = Engine::view_from_camera(cam, 64, 48);
            std::vector<float> linear, prev4(4);
            std::vector<rb_guide> g(1);
            std::vector<float> out = Engine::reproject_buffers(rp, 1, 1, v, prev4, g, g, &prev4);
            std::vector<uint8_t> a = e.denoise_history(), b = e.denoise_history(rp, Engine::denoise_defaults(), &linear);
            e.denoise_history_device(rp, Engine::denoise_defaults(), d_rgba);
            e.reproject(rp, 1, 1, v, d_a, d_g, d_g, nullptr, d_a);
            std::vector<float> f = e.history();
            e.history_reset();
            e.sync();
            return (int)(a.size() + b.size() + f.size() + out.size()) + (int)e.last_reproject_ms();
        }
        int main() { return 0; }
    '''))
    lib_dir = os.path.join(ROOT, "renderbaby_amd")
    subprocess.check_call(["g++", "-std=c++17", "-Wall", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(tmp_path / "r"),
                           "-L", lib_dir, "-l:librenderbaby_hip.so", f"-Wl,-rpath,{lib_dir}"])
