"""Camera rays made on the device (rb_camera_rays / rb_trace_camera), the part that needs no device: the
library exports the three entry points, rb_camera_ex, the kinds, the flag and RB_CAMERA_PIECE_ITEMS are what rb_abi.h states
-- seen from a compiled C program and from the Python mirror --, the C++ mirror compiles against them, and rb_camera_rays
refuses every bad argument before it touches a device (device = -1: the call would otherwise use the current one)."""
import os
import subprocess
import textwrap

import numpy as np
import pytest

from renderbaby_amd import _lib, abi, camera

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMBOLS = ("rb_camera_rays", "rb_trace_camera", "rb_trace_camera_device")
LAYOUT = {"sizeof(rb_camera_ex)": 96, "offsetof(rb_camera_ex, kind)": 0, "offsetof(rb_camera_ex, width)": 4,
          "offsetof(rb_camera_ex, height)": 8, "offsetof(rb_camera_ex, flags)": 12, "offsetof(rb_camera_ex, pos)": 16,
          "offsetof(rb_camera_ex, tan_half_fov)": 28, "offsetof(rb_camera_ex, right)": 32, "offsetof(rb_camera_ex, half_width)": 44,
          "offsetof(rb_camera_ex, up)": 48, "offsetof(rb_camera_ex, half_height)": 60, "offsetof(rb_camera_ex, forward)": 64,
          "offsetof(rb_camera_ex, lens_radius)": 76, "offsetof(rb_camera_ex, focus_distance)": 80,
          "offsetof(rb_camera_ex, _reserved)": 84, "RB_CAM_PERSPECTIVE": 1, "RB_CAM_ORTHO": 2, "RB_CAM_EQUIRECT": 3,
          "RB_CAM_NO_JITTER": 1, "RB_CAMERA_PIECE_ITEMS": 1 << 23}
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
        int (*f0)(int32_t, const rb_camera_ex*, uint64_t, size_t, uint32_t, uint32_t, rb_ray*, uint32_t*) = rb_camera_rays;
        int (*f1)(rb_engine*, const rb_camera_ex*, uint64_t, size_t, uint32_t, uint32_t, rb_radiance*) = rb_trace_camera;
        int (*f2)(rb_engine*, const rb_camera_ex*, uint64_t, size_t, uint32_t, uint32_t, rb_radiance*) = rb_trace_camera_device;
    '''))
    subprocess.check_call(["gcc", "-std=c11", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), "-c", str(proto), "-o", str(tmp_path / "proto.o")])
    got = dict(line.rsplit("=", 1) for line in subprocess.check_output([str(exe)], text=True).splitlines())
    assert {k: int(v) for k, v in got.items()} == LAYOUT


def test_python_mirror_agrees():
    dt = abi.CAMERA_EX
    assert dt.itemsize == LAYOUT["sizeof(rb_camera_ex)"]
    for key, off in LAYOUT.items():
        if key.startswith("offsetof"):
            assert dt.fields[key.split(", ")[1].rstrip(")")][1] == off, key
    assert (abi.CAM_PERSPECTIVE, abi.CAM_ORTHO, abi.CAM_EQUIRECT, abi.CAM_NO_JITTER) == (1, 2, 3, 1)
    assert abi.CAMERA_PIECE_ITEMS == LAYOUT["RB_CAMERA_PIECE_ITEMS"]
    assert abi.CAMERA_PIECE_ITEMS // 65536 >= 64   # a piece holds a whole block of 64 pixels at the largest sample count
    assert abi.CAMERA_PIECE_ITEMS * (32 + 16) <= 512 << 20   # record and colour scratch within what rb_trace_rays may hold
    from renderbaby_amd import Engine, bake, engine
    assert callable(Engine.trace_camera) and callable(engine.camera_rays_device) and callable(bake.render_camera)
    assert callable(camera.make) and callable(camera.rays)


def _cam(kind="perspective", **kw):
    args = dict(width=8, height=4, pos=(0, 1, 3), aperture=0.2, focus_distance=2.0)
    args.update(kw)
    return np.ascontiguousarray(camera.make(kind, **args)).reshape(1)


def _call(cam, first_pixel=0, n=4, first_sample=0, samples=2, rays=True, seeds=True):
    lib = _lib.load()
    m = max(min(n * samples, 1 << 16), 1)
    r, s = np.full(m, 7, dtype=abi.RAY), np.full(m, 7, dtype=np.uint32)
    rc = lib.rb_camera_rays(-1, None if cam is None else cam.ctypes.data, first_pixel, n, first_sample, samples,
                            r.ctypes.data if rays else None, s.ctypes.data if seeds else None)
    assert (s == 7).all() and (r["_pad0"] == 7).all(), "a refused call wrote its outputs"
    return rc


def _with(cam, **fields):
    c = cam.copy()
    for k, v in fields.items():
        c[k][0] = v
    return c


REFUSALS = [
    ("unknown kind 0", lambda c: (_with(c, kind=0), {})),
    ("unknown kind 4", lambda c: (_with(c, kind=4), {})),
    ("unknown flag bit", lambda c: (_with(c, flags=2), {})),
    ("unknown flag bits beside the known one", lambda c: (_with(c, flags=0x80000001), {})),
    ("width 0", lambda c: (_with(c, width=0), {})),
    ("height 0", lambda c: (_with(c, height=0), {})),
    ("width above 2^24", lambda c: (_with(c, width=(1 << 24) + 1, height=1), {})),
    ("height above 2^24", lambda c: (_with(c, width=1, height=(1 << 24) + 1), {})),
    ("width * height = 2^31", lambda c: (_with(c, width=1 << 16, height=1 << 15), {})),
    ("range starts behind the image", lambda c: (c, dict(first_pixel=33, n=1))),
    ("range ends behind the image", lambda c: (c, dict(first_pixel=30, n=3))),
    ("range wraps around 64 bits", lambda c: (c, dict(first_pixel=(1 << 64) - 1, n=2))),
    ("samples 0", lambda c: (c, dict(samples=0))),
    ("samples above 65536", lambda c: (c, dict(samples=65537))),
    ("first_sample + samples overflows", lambda c: (c, dict(first_sample=M32, samples=1))),
    ("first_sample + samples overflows by one", lambda c: (c, dict(first_sample=M32 - 1, samples=2))),
    ("n_pixels * samples above 2^31 - 64", lambda c: (_with(c, width=1 << 15, height=1 << 15), dict(n=1 << 15, samples=65536))),
    ("NaN tan_half_fov", lambda c: (_with(c, tan_half_fov=np.nan), {})),
    ("Inf right", lambda c: (_with(c, right=(np.inf, 0, 0)), {})),
    ("NaN up", lambda c: (_with(c, up=(0, np.nan, 0)), {})),
    ("-Inf forward", lambda c: (_with(c, forward=(0, 0, -np.inf)), {})),
    ("Inf focus_distance", lambda c: (_with(c, focus_distance=np.inf), {})),
    ("NaN lens_radius", lambda c: (_with(c, lens_radius=np.nan), {})),
    ("NaN half_width of a perspective camera", lambda c: (_with(c, half_width=np.nan), {})),
    ("tan_half_fov 0", lambda c: (_with(c, tan_half_fov=0.0), {})),
    ("tan_half_fov negative", lambda c: (_with(c, tan_half_fov=-1.0), {})),
    ("lens_radius negative", lambda c: (_with(c, lens_radius=-0.1), {})),
    ("focus_distance 0 with a lens", lambda c: (_with(c, focus_distance=0.0), {})),
    ("focus_distance negative with a lens", lambda c: (_with(c, focus_distance=-2.0), {})),
    ("ortho: half_width 0", lambda c: (_with(c, kind=abi.CAM_ORTHO, half_width=0.0), {})),
    ("ortho: half_height negative", lambda c: (_with(c, kind=abi.CAM_ORTHO, half_height=-1.0), {})),
    ("_reserved[0]", lambda c: (_with(c, _reserved=(1, 0, 0)), {})),
    ("_reserved[2]", lambda c: (_with(c, _reserved=(0, 0, 1)), {})),
]


@pytest.mark.parametrize("name,make", REFUSALS, ids=[r[0] for r in REFUSALS])
def test_refusals_before_a_device_is_touched(name, make):
    cam, kw = make(_cam())
    assert _call(cam, **kw) == INVALID_OPTIONS, name
    assert _lib.load().rb_last_error(None)


def test_null_arguments_and_empty_ranges():
    cam = _cam()
    assert abi.ERR[NULL_ARGUMENT] == "NullArgument"
    assert _call(None) == NULL_ARGUMENT
    assert _call(cam, rays=False) == NULL_ARGUMENT
    assert _call(cam, seeds=False) == NULL_ARGUMENT
    # n_pixels == 0 is RB_OK, with or without pointers, at either end of the image -- and a bad camera is still refused
    assert _call(cam, n=0) == 0 and _call(cam, first_pixel=32, n=0) == 0
    assert _call(None, n=0, rays=False, seeds=False) == 0 and _call(cam, n=0, rays=False, seeds=False) == 0
    assert _call(_with(cam, kind=9), n=0) == INVALID_OPTIONS and _call(cam, first_pixel=33, n=0) == INVALID_OPTIONS
    # the engine forms refuse a NULL engine before they look at anything else
    lib = _lib.load()
    out = np.zeros(4, dtype=abi.RADIANCE)
    for fn in (lib.rb_trace_camera, lib.rb_trace_camera_device):
        assert fn(None, cam.ctypes.data, 0, 4, 0, 1, out.ctypes.data) == NULL_ARGUMENT
        assert fn(None, None, 0, 0, 0, 0, None) == NULL_ARGUMENT


def test_cpp_mirror_compiles(tmp_path):
    src = tmp_path / "c.cpp"
    src.write_text(textwrap.dedent('''
        #include "renderbaby/engine.hpp"
        using namespace renderbaby;
        static_assert(sizeof(rb_camera_ex) == 96 && RB_CAMERA_PIECE_ITEMS == (1u << 23), "rb_camera_ex, the piece");
        int use(Engine& e, rb_radiance* d_out) {
            rb_camera_ex cam{};
            cam.kind = RB_CAM_PERSPECTIVE;
            cam.flags = RB_CAM_NO_JITTER;
            cam.width = 8; cam.height = 4;
            std::vector<rb_radiance> a = e.trace_camera(cam, 16);
            std::vector<rb_radiance> b = e.trace_camera(cam, 16, 7, 8, 8);
            e.trace_camera_device(cam, 0, 32, d_out, 16, 7);
            e.sync();
            return (int)(a.size() + b.size());
        }
        int main() { return 0; }
    '''))
    lib_dir = os.path.join(ROOT, "renderbaby_amd")
    subprocess.check_call(["g++", "-std=c++17", "-Wall", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(tmp_path / "c"),
                           "-L", lib_dir, "-l:librenderbaby_hip.so", f"-Wl,-rpath,{lib_dir}"])
