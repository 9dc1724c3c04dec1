"""Any-hit occlusion queries and the device forms, the part that needs no device: the library exports the entry points, the
result bytes and stage masks are the ones rb_abi.h states -- seen from a compiled C program and from the Python mirror -- the
C++ mirror compiles against them, and a NULL engine is refused before anything touches a device."""
import ctypes as C
import os
import subprocess
import textwrap

from renderbaby_amd import _lib, abi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMBOLS = ("rb_occluded", "rb_occluded_device", "rb_cast_rays_device")
ENUMS = {"RB_OCCL_VISIBLE": 0, "RB_OCCL_OCCLUDED": 1, "RB_OCCL_INVALID": 255, "RB_MASK_GROUND": 1, "RB_MASK_TRIANGLES": 2,
         "RB_MASK_SPHERES": 4, "RB_MASK_LIGHTS": 8, "RB_MASK_ALL": 15}


def test_library_exports_the_three_symbols():
    lib = _lib.load()
    for name in SYMBOLS:
        assert name in _lib.EXPORTS
        getattr(lib, name)


def test_enum_values_from_a_compiled_c_program(tmp_path):
    lines = [f'printf("{n} %u\\n", (unsigned){n});' for n in ENUMS]
    src = tmp_path / "enums.c"
    src.write_text("#include <stdio.h>\n#include <stddef.h>\n#include \"rb_abi.h\"\nint main(void) {\n" + "\n".join(lines) + "\nreturn 0; }\n")
    exe = tmp_path / "enums"
    subprocess.check_call(["gcc", "-std=c11", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)])
    # the prototypes as the header's users see them: a typed function pointer takes no other signature (compiled, not linked)
    proto = tmp_path / "proto.c"
    proto.write_text(textwrap.dedent('''
        #include "rb_abi.h"
        int (*f0)(rb_engine*, const rb_ray*, const float*, size_t, uint32_t, uint8_t*) = rb_occluded;
        int (*f1)(rb_engine*, const rb_ray*, const float*, size_t, uint32_t, uint8_t*) = rb_occluded_device;
        int (*f2)(rb_engine*, const rb_ray*, size_t, rb_hit*, rb_surface*) = rb_cast_rays_device;
    '''))
    subprocess.check_call(["gcc", "-std=c11", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), "-c", str(proto), "-o", str(tmp_path / "proto.o")])
    got = dict(line.split(" ", 1) for line in subprocess.check_output([str(exe)], text=True).splitlines())
    assert {k: int(v) for k, v in got.items()} == ENUMS


def test_python_mirror_agrees():
    assert (abi.OCCL_VISIBLE, abi.OCCL_OCCLUDED, abi.OCCL_INVALID) == (0, 1, 255)
    assert (abi.MASK_GROUND, abi.MASK_TRIANGLES, abi.MASK_SPHERES, abi.MASK_LIGHTS, abi.MASK_ALL) == (1, 2, 4, 8, 15)
    assert abi.MASK_GROUND | abi.MASK_TRIANGLES | abi.MASK_SPHERES | abi.MASK_LIGHTS == abi.MASK_ALL
    from renderbaby_amd import Engine, aov
    for name in ("occluded", "occluded_records", "cast_rays", "cast_ray_records"):
        assert callable(getattr(Engine, name))
    assert callable(aov.ambient_occlusion)


def test_null_engine_is_refused_without_a_device():
    lib = _lib.load()
    rays, hits, out, tmax = (abi.Ray * 1)(), (abi.Hit * 1)(), (C.c_uint8 * 1)(7), (C.c_float * 1)(1.0)
    null_arg = 15
    assert abi.ERR[null_arg] == "NullArgument"
    assert lib.rb_occluded(None, rays, tmax, 1, abi.MASK_ALL, out) == null_arg
    assert lib.rb_occluded(None, None, None, 0, 0, None) == null_arg
    assert lib.rb_occluded_device(None, rays, None, 1, abi.MASK_ALL, out) == null_arg
    assert lib.rb_cast_rays_device(None, rays, 1, hits, None) == null_arg
    assert out[0] == 7


def test_cpp_mirror_compiles(tmp_path):
    src = tmp_path / "o.cpp"
    src.write_text(textwrap.dedent('''
        #include "renderbaby/engine.hpp"
        using namespace renderbaby;
        static_assert(RB_OCCL_VISIBLE == 0 && RB_OCCL_OCCLUDED == 1 && RB_OCCL_INVALID == 255, "result bytes");
        static_assert(RB_MASK_ALL == (RB_MASK_GROUND | RB_MASK_TRIANGLES | RB_MASK_SPHERES | RB_MASK_LIGHTS), "masks");
        int use(Engine& e, const rb_ray* d_rays, const float* d_tmax, uint8_t* d_out, rb_hit* d_hits) {
            std::vector<rb_ray> rays{rb_ray{{0, 0, 0}, 0, {0, 0, -1}, 0}};
            std::vector<uint8_t> a = e.occluded(rays);
            std::vector<uint8_t> b = e.occluded(rays, {2.5f}, RB_MASK_ALL & ~RB_MASK_LIGHTS);
            e.occluded_device(d_rays, d_tmax, 1, d_out);
            e.cast_rays_device(d_rays, 1, d_hits);
            e.sync();
            return (int)(a.size() + b.size());
        }
        int main() { return 0; }
    '''))
    lib_dir = os.path.join(ROOT, "renderbaby_amd")
    subprocess.check_call(["g++", "-std=c++17", "-Wall", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(tmp_path / "o"),
                           "-L", lib_dir, "-l:librenderbaby_hip.so", f"-Wl,-rpath,{lib_dir}"])
