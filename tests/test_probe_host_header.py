"""The C++ mirror (include/renderbaby/engine.hpp) names the probe bake: a three-line translation unit compiles."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_the_mirror_method_compiles(tmp_path):
    src = tmp_path / "probe.cpp"
    src.write_text('#include "renderbaby/engine.hpp"\n'
                   "std::vector<rb_sh9> bake(renderbaby::Engine& e, const std::vector<rb_probe>& p) { return e.bake_probes(p, 64, 7, nullptr); }\n"
                   "void bake_device(renderbaby::Engine& e, const rb_probe* p, rb_sh9* o) { e.bake_probes_device(p, nullptr, 3, o, 64); e.sync(); }\n")
    subprocess.check_call(["g++", "-std=c++17", "-Wall", "-Werror", "-fsyntax-only", "-I", os.path.join(ROOT, "include"), str(src)])
