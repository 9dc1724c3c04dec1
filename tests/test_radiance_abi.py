"""Path-traced radiance along given rays (rb_trace_rays), the part that needs no device: the library
exports the two entry points, rb_radiance and RB_TRACE_PIECE_ITEMS are what rb_abi.h states -- seen from a compiled C program
and from the Python mirror -- the C++ mirror compiles against them, and a NULL engine is refused before anything touches a
device."""
import os
import subprocess
import textwrap

import numpy as np

from renderbaby_amd import _lib, abi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMBOLS = ("rb_trace_rays", "rb_trace_rays_device")
LAYOUT = {"sizeof(rb_radiance)": 16, "offsetof(rb_radiance, sum)": 0, "offsetof(rb_radiance, weight)": 12, "RB_TRACE_PIECE_ITEMS": 1 << 24}


def test_library_exports_both_symbols():
    lib = _lib.load()
    for name in SYMBOLS:
        assert name in _lib.EXPORTS
        getattr(lib, name)


def test_layout_and_piece_size_from_a_compiled_c_program(tmp_path):
    lines = [f'printf("{n}=%lu\\n", (unsigned long)({n}));' for n in LAYOUT]
    src = tmp_path / "layout.c"
    src.write_text("#include <stdio.h>\n#include <stddef.h>\n#include \"rb_abi.h\"\nint main(void) {\n" + "\n".join(lines) + "\nreturn 0; }\n")
    exe = tmp_path / "layout"
    subprocess.check_call(["gcc", "-std=c11", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)])
    # the prototypes as the header's users see them: a typed function pointer takes no other signature (compiled, not linked)
    proto = tmp_path / "proto.c"
    proto.write_text(textwrap.dedent('''
        #include "rb_abi.h"
        int (*f0)(rb_engine*, const rb_ray*, const uint32_t*, size_t, uint32_t, uint32_t, rb_radiance*) = rb_trace_rays;
        int (*f1)(rb_engine*, const rb_ray*, const uint32_t*, size_t, uint32_t, uint32_t, rb_radiance*) = rb_trace_rays_device;
    '''))
    subprocess.check_call(["gcc", "-std=c11", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), "-c", str(proto), "-o", str(tmp_path / "proto.o")])
    got = dict(line.rsplit("=", 1) for line in subprocess.check_output([str(exe)], text=True).splitlines())
    assert {k: int(v) for k, v in got.items()} == LAYOUT


def test_python_mirror_agrees():
    assert abi.RADIANCE.itemsize == 16 and abi.RADIANCE.fields["sum"][1] == 0 and abi.RADIANCE.fields["weight"][1] == 12
    assert abi.RADIANCE["sum"].shape == (3,) and abi.RADIANCE["weight"] == np.float32
    assert abi.TRACE_PIECE_ITEMS == LAYOUT["RB_TRACE_PIECE_ITEMS"]
    assert abi.TRACE_PIECE_ITEMS // 65536 >= 64   # a piece holds a whole block of 64 rays at the largest sample count
    from renderbaby_amd import Engine, bake
    for name in ("trace_rays", "trace_ray_records"):
        assert callable(getattr(Engine, name))
    for name in ("irradiance", "camera_rays", "render_rays"):
        assert callable(getattr(bake, name))


def test_null_engine_is_refused_without_a_device():
    lib = _lib.load()
    rays, out = (abi.Ray * 1)(), np.full(1, 7, dtype=abi.RADIANCE)
    null_arg = 15
    assert abi.ERR[null_arg] == "NullArgument"
    assert lib.rb_trace_rays(None, rays, None, 1, 0, 1, out.ctypes.data) == null_arg
    assert lib.rb_trace_rays(None, None, None, 0, 0, 0, None) == null_arg
    assert lib.rb_trace_rays_device(None, rays, None, 1, 0, 1, out.ctypes.data) == null_arg
    assert out["weight"][0] == 7


def test_cpp_mirror_compiles(tmp_path):
    src = tmp_path / "r.cpp"
    src.write_text(textwrap.dedent('''
        #include "renderbaby/engine.hpp"
        using namespace renderbaby;
        static_assert(sizeof(rb_radiance) == 16 && RB_TRACE_PIECE_ITEMS == (1u << 24), "rb_radiance, the piece");
        int use(Engine& e, const rb_ray* d_rays, const uint32_t* d_seeds, rb_radiance* d_out) {
            std::vector<rb_ray> rays{rb_ray{{0, 0, 0}, 0, {0, 0, -1}, 0}};
            std::vector<rb_radiance> a = e.trace_rays(rays);
            std::vector<rb_radiance> b = e.trace_rays(rays, {42u}, 16, 7);
            e.trace_rays_device(d_rays, d_seeds, 1, d_out, 16, 7);
            e.sync();
            return (int)(a.size() + b.size()) + (int)a[0].weight;
        }
        int main() { return 0; }
    '''))
    lib_dir = os.path.join(ROOT, "renderbaby_amd")
    subprocess.check_call(["g++", "-std=c++17", "-Wall", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(tmp_path / "r"),
                           "-L", lib_dir, "-l:librenderbaby_hip.so", f"-Wl,-rpath,{lib_dir}"])
