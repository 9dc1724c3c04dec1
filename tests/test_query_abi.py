"""Closest-hit queries, the part that needs no device: the library exports the entry points, the record layouts are the
ones rb_abi.h states -- seen from a compiled C program, from the ctypes mirrors and from the numpy dtypes -- and NULL
arguments are refused before anything touches a device."""
import ctypes as C
import os
import subprocess
import textwrap

from renderbaby_amd import _lib, abi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# (struct, field) -> offset, from the issue's layout
OFFSETS = {
    ("rb_ray", "origin"): 0, ("rb_ray", "dir"): 16,
    ("rb_hit", "t"): 0, ("rb_hit", "kind"): 4, ("rb_hit", "prim"): 8, ("rb_hit", "mesh"): 12, ("rb_hit", "u"): 16,
    ("rb_hit", "v"): 20, ("rb_hit", "normal"): 32,
    ("rb_surface", "albedo"): 0, ("rb_surface", "flags"): 12, ("rb_surface", "emissive"): 16,
    ("rb_surface", "texture_index"): 28, ("rb_surface", "uv"): 32,
}
SIZES = {"rb_ray": 32, "rb_hit": 48, "rb_surface": 48}
CTYPES = {"rb_ray": abi.Ray, "rb_hit": abi.Hit, "rb_surface": abi.Surface}
DTYPES = {"rb_ray": abi.RAY, "rb_hit": abi.HIT, "rb_surface": abi.SURFACE}


def test_library_exports_the_query_entry_points():
    lib = _lib.load()
    for name in ("rb_cast_rays", "rb_render_hits", "rb_pick", "rb_last_query_kernel_name"):
        assert name in _lib.EXPORTS
        getattr(lib, name)


def test_layouts_from_a_compiled_c_program(tmp_path):
    lines = [f'printf("{s} %zu\\n", sizeof({s}));' for s in SIZES]
    lines += [f'printf("{s}.{f} %zu\\n", offsetof({s}, {f}));' for (s, f) in OFFSETS]
    lines += ['printf("kinds %u %u %u %u %u %u\\n", (unsigned)RB_HIT_NONE, (unsigned)RB_HIT_GROUND, (unsigned)RB_HIT_TRIANGLE, '
              '(unsigned)RB_HIT_SPHERE, (unsigned)RB_HIT_LIGHT, (unsigned)RB_HIT_INVALID);']
    src = tmp_path / "layout.c"
    src.write_text("#include <stdio.h>\n#include <stddef.h>\n#include \"rb_abi.h\"\nint main(void) {\n" + "\n".join(lines)
                   + "\nreturn 0; }\n")
    exe = tmp_path / "layout"
    subprocess.check_call(["gcc", "-std=c11", "-Wall", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)])
    got = dict(line.split(" ", 1) for line in subprocess.check_output([str(exe)], text=True).splitlines())
    for s, n in SIZES.items():
        assert int(got[s]) == n, (s, got[s])
    for (s, f), off in OFFSETS.items():
        assert int(got[f"{s}.{f}"]) == off, (s, f, got[f"{s}.{f}"])
    assert got["kinds"] == "0 1 2 3 4 4294967295"


def test_layouts_of_the_python_mirrors():
    for s, n in SIZES.items():
        assert C.sizeof(CTYPES[s]) == n and DTYPES[s].itemsize == n, s
    for (s, f), off in OFFSETS.items():
        assert getattr(CTYPES[s], f).offset == off, (s, f)
        assert DTYPES[s].fields[f][1] == off, (s, f)
    assert (abi.HIT_NONE, abi.HIT_GROUND, abi.HIT_TRIANGLE, abi.HIT_SPHERE, abi.HIT_LIGHT, abi.HIT_INVALID) == (0, 1, 2, 3, 4, 0xFFFFFFFF)


def test_null_engine_is_refused_without_a_device():
    lib = _lib.load()
    rays = (abi.Ray * 1)()
    hits = (abi.Hit * 1)()
    null_arg = 15
    assert abi.ERR[null_arg] == "NullArgument"
    assert lib.rb_cast_rays(None, rays, 1, hits, None) == null_arg
    assert lib.rb_cast_rays(None, None, 0, None, None) == null_arg
    assert lib.rb_render_hits(None, hits, None) == null_arg
    assert lib.rb_pick(None, 0, 0, hits, None) == null_arg
    assert lib.rb_last_query_kernel_name(None) == b""


def test_cpp_mirror_compiles(tmp_path):
    src = tmp_path / "q.cpp"
    src.write_text(textwrap.dedent('''
        #include "renderbaby/engine.hpp"
        using namespace renderbaby;
        int use(Engine& e) {
            Engine::Hits a = e.cast_rays({rb_ray{{0, 0, 0}, 0, {0, 0, -1}, 0}}, true);
            Engine::Hits b = e.render_hits();
            rb_surface s{};
            rb_hit h = e.pick(1, 2, &s);
            return (int)(a.hits.size() + b.hits.size() + h.kind);
        }
        int main() { return 0; }
    '''))
    lib_dir = os.path.join(ROOT, "renderbaby_amd")
    subprocess.check_call(["g++", "-std=c++17", "-Wall", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(tmp_path / "q"),
                           "-L", lib_dir, "-l:librenderbaby_hip.so", f"-Wl,-rpath,{lib_dir}"])
