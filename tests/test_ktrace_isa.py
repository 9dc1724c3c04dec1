"""Guard on the compiled code of k_trace's default instantiations (no GPU: hipcc cross-compiles).  The device assembly is built
with the Makefile's flags and read through tools/isa_blocks.py, the parser the attribution table uses.  What is held:
 * no scalar register is spilled (a spilled one comes back through v_readlane, a slot of the unit that binds the kernel);
   vector spills and scratch stay at what the register budget of each instantiation has always cost (4 registers / 20 B per
   lane outside the segment code with 8 waves per SIMD, none with 6);
 * the innermost triangle loop of the single-node walk touches no scratch memory and hands no -1.0 "miss" value around;
 * the next triangle's record is requested (scalar loads) before the first vector instruction of a trip."""
import os
import re
import shutil
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import isa_blocks  # noqa: E402

# (mangled-name part, vector registers spilled at most, scratch bytes per lane at most)
KERNELS = [("k_traceILb0ELb0ELi8", 4, 20), ("k_traceILb0ELb0ELi6", 0, 0)]


def _makefile_flags():
    text = open(os.path.join(ROOT, "Makefile")).read()
    var = {}
    for name in ("HIPCC", "ARCH", "NUMERICS", "HIPFLAGS"):
        m = re.search(rf"^{name}\s*[:?]?=\s*(.*)$", text, re.M)
        assert m, name
        var[name] = m.group(1).strip()
    flags = var["HIPFLAGS"].replace("$(ARCH)", var["ARCH"]).replace("$(NUMERICS)", var["NUMERICS"])
    assert "$(" not in flags, flags
    return os.environ.get("HIPCC", var["HIPCC"]), flags.split()


@pytest.fixture(scope="module")
def asm(tmp_path_factory):
    hipcc, flags = _makefile_flags()
    if not (os.path.isfile(hipcc) or shutil.which(hipcc)):
        pytest.skip("hipcc is not installed")
    out = tmp_path_factory.mktemp("ktrace_isa")
    s, usage = str(out / "rb_kernels.s"), str(out / "resource_usage.txt")
    with open(usage, "w") as err:
        subprocess.check_call([hipcc, *flags, "-S", "--cuda-device-only", "-o", s, os.path.join(ROOT, "renderbaby_amd/csrc/rb_kernels.hip"),
                               "-Rpass-analysis=kernel-resource-usage"], stderr=err, cwd=ROOT)
    return s, usage


@pytest.mark.parametrize("kernel,vgpr_spill,scratch", KERNELS)
def test_registers_and_spills(asm, kernel, vgpr_spill, scratch):
    r = isa_blocks.resource_usage(asm[1], kernel)
    print(kernel, r)
    assert r["SGPRs Spill"] == 0
    assert r["VGPRs Spill"] <= vgpr_spill
    assert r["ScratchSize [bytes/lane]"] <= scratch


@pytest.mark.parametrize("kernel", [k[0] for k in KERNELS])
def test_triangle_loop(asm, kernel):
    blocks = isa_blocks.parse_blocks(asm[0], kernel)
    header, body = isa_blocks.triangle_loop(blocks)
    assert header.inner_header and len(body) >= 4
    instrs = [i for b in body for i in b.instrs]
    print(kernel, header.name, len(body), "blocks,", sum(len(b.valu) for b in body), "VALU")
    assert not [i.text for i in instrs if i.op.startswith("scratch_")]
    assert not [i.text for i in instrs if i.op.startswith("v_mov_b32") and re.search(r",\s*-1\.0\s*$", i.args)]
    # a trip starts at the loop's header block: the record of the NEXT triangle is on its way before any vector work
    loads = [i.line for i in header.instrs if i.op.startswith("s_load_dwordx")]
    valu = [i.line for b in body for i in b.valu]
    assert loads, "the loop header requests no record"
    assert valu and max(loads) < min(l for l in valu if l >= header.line)
    # ... and it is the whole record: 12 dwords or more
    assert sum(int(re.search(r"dwordx(\d+)", i.op).group(1)) for i in header.instrs if i.op.startswith("s_load_dwordx")) >= 12
    # nothing is fetched anywhere else in the trip (the current record was waited for when the last trip ended)
    assert not [i.text for b in body if b is not header for i in b.instrs if i.op.startswith("s_load_")]
