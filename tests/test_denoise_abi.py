"""The denoiser's ABI, the part that needs no device: the library exports the entry points, rb_guide and
rb_denoise_params have the stated sizes and offsets -- seen from a compiled C program and from the Python mirror -- the C++
mirror compiles against them, the defaults are the model's, and a NULL engine or NULL params is refused before anything
touches a device."""
import ctypes as C
import os
import subprocess
import textwrap

import numpy as np

from renderbaby_amd import _lib, abi, denoise, engine

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMBOLS = ("rb_denoise_default_params", "rb_denoise_buffers", "rb_denoise", "rb_denoise_device", "rb_denoise_guides",
           "rb_last_denoise_ms")
LAYOUT = {"sizeof(rb_guide)": 48, "sizeof(rb_denoise_params)": 32,
          "offsetof(rb_guide, normal)": 0, "offsetof(rb_guide, t)": 12, "offsetof(rb_guide, pos)": 16, "offsetof(rb_guide, cls)": 28,
          "offsetof(rb_guide, albedo)": 32, "offsetof(rb_guide, _pad)": 44,
          "offsetof(rb_denoise_params, iterations)": 0, "offsetof(rb_denoise_params, normal_power_log2)": 4,
          "offsetof(rb_denoise_params, sigma_depth)": 8, "offsetof(rb_denoise_params, sigma_color)": 12,
          "offsetof(rb_denoise_params, albedo_floor)": 16, "offsetof(rb_denoise_params, flags)": 20,
          "offsetof(rb_denoise_params, _reserved)": 24}
NULL_ARGUMENT = 15


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
    # the prototypes as the header's users see them: a typed function pointer takes no other signature (compiled, not linked)
    proto = tmp_path / "proto.c"
    proto.write_text(textwrap.dedent('''
        #include "rb_abi.h"
        int (*f0)(rb_denoise_params*) = rb_denoise_default_params;
        int (*f1)(int32_t, const rb_denoise_params*, uint32_t, uint32_t, const float*, const rb_guide*, float*, uint8_t*) = rb_denoise_buffers;
        int (*f2)(rb_engine*, const rb_denoise_params*, uint8_t*, float*) = rb_denoise;
        int (*f3)(rb_engine*, const rb_denoise_params*, uint8_t*, float*) = rb_denoise_device;
        int (*f4)(rb_engine*, rb_guide*) = rb_denoise_guides;
        int (*f5)(rb_engine*, float*, float*) = rb_last_denoise_ms;
    '''))
    subprocess.check_call(["gcc", "-std=c11", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), "-c", str(proto), "-o", str(tmp_path / "proto.o")])
    got = dict(line.rsplit("=", 1) for line in subprocess.check_output([str(exe)], text=True).splitlines())
    assert {k: int(v) for k, v in got.items()} == LAYOUT


def test_python_mirror_agrees():
    assert abi.GUIDE.itemsize == 48 and abi.DENOISE_PARAMS.itemsize == 32
    for key, want in LAYOUT.items():
        if key.startswith("offsetof"):
            struct, field = key[len("offsetof("):-1].split(", ")
            dt = abi.GUIDE if struct == "rb_guide" else abi.DENOISE_PARAMS
            assert dt.fields[field][1] == want, key
    from renderbaby_amd import Engine
    for name in ("denoise", "denoise_guides", "last_denoise_ms"):
        assert callable(getattr(Engine, name))
    assert callable(denoise.filter) and callable(denoise.guides_from_records) and callable(engine.denoise_buffers)


def test_defaults_are_the_models_and_valid():
    d = engine.denoise_defaults()
    assert d.tobytes() == denoise.default_params().tobytes()
    denoise.check_params(d)
    assert 0 < int(d["iterations"]) <= 8 and int(d["flags"]) == 0
    assert _lib.load().rb_denoise_default_params(None) == NULL_ARGUMENT


def test_null_engine_or_params_is_refused_without_a_device():
    lib = _lib.load()
    assert abi.ERR[NULL_ARGUMENT] == "NullArgument"
    p = np.ascontiguousarray(denoise.default_params()).reshape(1)
    rgba, lin = (C.c_uint8 * 4)(7, 7, 7, 7), (C.c_float * 4)(3.0, 3.0, 3.0, 3.0)
    guides = np.zeros(1, abi.GUIDE)
    assert lib.rb_denoise(None, p.ctypes.data, rgba, lin) == NULL_ARGUMENT
    assert lib.rb_denoise(None, None, None, None) == NULL_ARGUMENT
    assert lib.rb_denoise_device(None, p.ctypes.data, rgba, None) == NULL_ARGUMENT
    assert lib.rb_denoise_guides(None, guides.ctypes.data) == NULL_ARGUMENT
    ms = C.c_float(5.0)
    assert lib.rb_last_denoise_ms(None, C.byref(ms), None) == NULL_ARGUMENT
    # the engine-less core: NULL params, colour, guides or both outputs -- before any device is touched (this machine has none)
    assert lib.rb_denoise_buffers(-1, None, 1, 1, lin, guides.ctypes.data, lin, rgba) == NULL_ARGUMENT
    assert lib.rb_denoise_buffers(-1, p.ctypes.data, 1, 1, None, guides.ctypes.data, lin, rgba) == NULL_ARGUMENT
    assert lib.rb_denoise_buffers(-1, p.ctypes.data, 1, 1, lin, None, lin, rgba) == NULL_ARGUMENT
    assert lib.rb_denoise_buffers(-1, p.ctypes.data, 1, 1, lin, guides.ctypes.data, None, None) == NULL_ARGUMENT
    # bad parameters are refused before a device is touched as well, and an empty frame is nothing to do
    bad = p.copy()
    bad["iterations"] = 9
    assert lib.rb_denoise_buffers(-1, bad.ctypes.data, 1, 1, lin, guides.ctypes.data, lin, rgba) == 18
    assert b"iterations" in lib.rb_last_error(None)
    assert lib.rb_denoise_buffers(-1, p.ctypes.data, 0, 5, lin, guides.ctypes.data, lin, rgba) == 0
    assert list(rgba) == [7, 7, 7, 7] and list(lin) == [3.0] * 4 and ms.value == 5.0


def test_cpp_mirror_compiles(tmp_path):
    src = tmp_path / "d.cpp"
    src.write_text(textwrap.dedent('''
        #include "renderbaby/engine.hpp"
        using namespace renderbaby;
        static_assert(sizeof(rb_guide) == 48 && sizeof(rb_denoise_params) == 32, "layouts");
        int use(Engine& e, uint8_t* d_rgba, float* d_linear) {
            rb_denoise_params p = Engine::denoise_defaults();
            p.iterations = 3;
            std::vector<float> linear;
            std::vector<uint8_t> a = e.denoise(), b = e.denoise(p, &linear);
            std::vector<rb_guide> g = e.denoise_guides();
            e.denoise_device(p, d_rgba, d_linear);
            e.sync();
            return (int)(a.size() + b.size() + g.size() + linear.size());
        }
        int main() { return 0; }
    '''))
    lib_dir = os.path.join(ROOT, "renderbaby_amd")
    subprocess.check_call(["g++", "-std=c++17", "-Wall", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(tmp_path / "d"),
                           "-L", lib_dir, "-l:librenderbaby_hip.so", f"-Wl,-rpath,{lib_dir}"])
