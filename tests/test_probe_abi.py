"""Irradiance probes made on the device (rb_probe_rays / rb_bake_probes / rb_bake_probes_device), the part
that needs no device: the library exports the entry points; rb_probe, rb_sh9 and RB_PROBE_PIECE_ITEMS are what rb_abi.h states
-- seen from a compiled C program and from the Python mirror --, and rb_probe_rays refuses every bad argument before it touches
a device (device = -1: the call would otherwise use the current one)."""
import ctypes as C
import os
import subprocess
import textwrap

import numpy as np
import pytest

from renderbaby_amd import _lib, abi, probes

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMBOLS = ("rb_probe_rays", "rb_bake_probes", "rb_bake_probes_device")
LAYOUT = {"sizeof(rb_probe)": 16, "offsetof(rb_probe, pos)": 0, "offsetof(rb_probe, _pad)": 12,
          "sizeof(rb_sh9)": 112, "offsetof(rb_sh9, sum)": 0, "offsetof(rb_sh9, sum[1])": 12, "offsetof(rb_sh9, sum[8][2])": 104,
          "offsetof(rb_sh9, weight)": 108, "RB_PROBE_PIECE_ITEMS": 1 << 23, "RB_HEMI_PIECE_ITEMS": 1 << 23}
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
        int (*f0)(int32_t, const rb_probe*, const uint32_t*, size_t, uint32_t, uint32_t, rb_ray*, uint32_t*) = rb_probe_rays;
        int (*f1)(rb_engine*, const rb_probe*, const uint32_t*, size_t, uint32_t, uint32_t, rb_sh9*) = rb_bake_probes;
        int (*f2)(rb_engine*, const rb_probe*, const uint32_t*, size_t, uint32_t, uint32_t, rb_sh9*) = rb_bake_probes_device;
    '''))
    subprocess.check_call(["gcc", "-std=c11", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), "-c", str(proto), "-o", str(tmp_path / "proto.o")])
    got = dict(line.rsplit("=", 1) for line in subprocess.check_output([str(exe)], text=True).splitlines())
    assert {k: int(v) for k, v in got.items()} == LAYOUT


def test_python_mirror_agrees():
    assert abi.PROBE.itemsize == LAYOUT["sizeof(rb_probe)"] == abi.SIZES["probe"][1]
    assert abi.SH9.itemsize == LAYOUT["sizeof(rb_sh9)"] == abi.SIZES["sh9"][1]
    assert abi.PROBE.fields["pos"][1] == 0 and abi.PROBE.fields["_pad"][1] == 12
    assert abi.SH9.fields["sum"][1] == 0 and abi.SH9.fields["weight"][1] == 108 and abi.SH9["sum"].shape == (9, 3)
    assert abi.PROBE_PIECE_ITEMS == LAYOUT["RB_PROBE_PIECE_ITEMS"] == abi.HEMI_PIECE_ITEMS
    assert abi.PROBE_PIECE_ITEMS // 65536 >= 64   # a piece holds a whole block of 64 probes at the largest sample count
    from renderbaby_amd import Engine, bake, engine
    assert callable(Engine.bake_probes) and callable(engine.probe_rays_device) and callable(bake.probes)
    assert callable(probes.rays) and callable(probes.basis) and callable(probes.project) and callable(probes.irradiance)


def _call(n=4, first_sample=0, samples=2, probes_in=True, seeds_in=False, rays=True, seeds=True):
    lib = _lib.load()
    pr, ids = probes.records(np.arange(12, dtype=np.float32).reshape(4, 3)), np.arange(4, dtype=np.uint32)
    m = max(min(n * samples, 1 << 16), 1)
    r, s = np.full(m, 7, dtype=abi.RAY), np.full(m, 7, dtype=np.uint32)
    rc = lib.rb_probe_rays(-1, pr.ctypes.data if probes_in else None, ids.ctypes.data if seeds_in else None, n, first_sample, samples,
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
]


@pytest.mark.parametrize("name,kw", REFUSALS, ids=[r[0] for r in REFUSALS])
def test_refusals_before_a_device_is_touched(name, kw):
    assert _call(**kw) == INVALID_OPTIONS, name
    assert _lib.load().rb_last_error(None)


def test_null_arguments_and_empty_calls():
    assert abi.ERR[NULL_ARGUMENT] == "NullArgument" and abi.ERR[INVALID_OPTIONS] == "InvalidOptions"
    assert _call(probes_in=False) == NULL_ARGUMENT
    assert _call(rays=False) == NULL_ARGUMENT
    # n == 0 is RB_OK, with or without the arrays -- and bad sample counts are still refused
    assert _call(n=0) == 0 and _call(n=0, probes_in=False, rays=False, seeds=False) == 0 and _call(n=0, seeds_in=True) == 0
    assert _call(n=0, samples=0) == INVALID_OPTIONS and _call(n=0, first_sample=M32, samples=1) == INVALID_OPTIONS
    # the engine forms refuse a NULL engine before they look at anything else
    lib = _lib.load()
    pr, out = probes.records(np.zeros((4, 3), np.float32)), np.zeros(4, dtype=abi.SH9)
    for fn in (lib.rb_bake_probes, lib.rb_bake_probes_device):
        assert fn(None, pr.ctypes.data, None, 4, 0, 1, out.ctypes.data) == NULL_ARGUMENT
        assert fn(None, None, None, 0, 0, 0, None) == NULL_ARGUMENT
    ms = C.c_float(5.0)
    assert lib.rb_last_probe_project_ms(None, C.byref(ms)) == NULL_ARGUMENT and ms.value == 5.0
