"""Guard on the compiled code of the flat kernels, k_trace_flat and k_trace_flat_direct (no GPU: hipcc cross-compiles) -- the
kernels of k_trace's plain walk for scenes that never read a triangle's u, v ("Scenes that carry no u, v").
Read through tools/isa_blocks.py from the assembly tests/test_ktrace_isa.py builds.  What is held, for the staged and the direct
form, 8 and 6 waves:
 * a trip of the triangle loop is at most 59 vector instructions (k_trace's 61 less the two moves of u and v) -- the trip as
   tools/ktrace_budget.py prices it, without the division's block that it branches over;
 * the loop touches no scratch memory, hands no -1.0 around, requests the whole record before its first vector instruction and
   fetches nothing else;
 * no scalar register is spilled; vector spills and scratch are at most those of k_trace<false, false, 8> in the same build,
   and the 8-wave kernels' registers and residency no worse than its;
 * the static count of vector instructions is below that kernel's.
The parsers count instructions and registers; no opcode is looked for beyond what tests/test_ktrace_isa.py reads."""
import re

import pytest

from tests.test_ktrace_isa import asm, isa_blocks  # noqa: F401  (the fixture: the device assembly built with the Makefile's flags)
import ktrace_budget  # noqa: E402  (tools/, on the path through tests.test_ktrace_isa)

REFERENCE = "k_traceILb0ELb0ELi8"
FLAT = [f"{name}ILi{waves}E" for name in ("k_trace_flat", "k_trace_flat_direct") for waves in (8, 6)]
TRIP_VALU = 59


@pytest.mark.parametrize("kernel", FLAT)
def test_flat_triangle_loop(asm, kernel):  # noqa: F811
    blocks = isa_blocks.parse_blocks(asm[0], kernel)
    header, body = isa_blocks.triangle_loop(blocks)
    assert header.inner_header and len(body) >= 4
    instrs = [i for b in body for i in b.instrs]
    trip = len(ktrace_budget.rows(blocks)[0][2])
    print(kernel, header.name, len(body), "blocks,", trip, "VALU a trip,", sum(len(b.valu) for b in body), "with the division's block")
    assert trip <= TRIP_VALU
    assert not [i.text for i in instrs if i.op.startswith("scratch_")]
    assert not [i.text for i in instrs if i.op.startswith("v_mov_b32") and re.search(r",\s*-1\.0\s*$", i.args)]
    loads = [i.line for i in header.instrs if i.op.startswith("s_load_dwordx")]
    valu = [i.line for b in body for i in b.valu]
    assert loads, "the loop header requests no record"
    assert valu and max(loads) < min(l for l in valu if l >= header.line)
    assert sum(int(re.search(r"dwordx(\d+)", i.op).group(1)) for i in header.instrs if i.op.startswith("s_load_dwordx")) >= 12
    assert not [i.text for b in body if b is not header for i in b.instrs if i.op.startswith("s_load_")]


@pytest.mark.parametrize("kernel", FLAT)
def test_flat_registers_spills_and_static_count(asm, kernel):  # noqa: F811
    ref, r = isa_blocks.resource_usage(asm[1], REFERENCE), isa_blocks.resource_usage(asm[1], kernel)
    print(kernel, r)
    assert r["SGPRs Spill"] == 0
    assert r["VGPRs Spill"] <= ref["VGPRs Spill"]
    assert r["ScratchSize [bytes/lane]"] <= ref["ScratchSize [bytes/lane]"]
    if "Li8E" in kernel:
        assert r["VGPRs"] <= ref["VGPRs"] and r["Occupancy [waves/SIMD]"] >= ref["Occupancy [waves/SIMD]"]
    total = sum(len(b.valu) for b in isa_blocks.parse_blocks(asm[0], kernel))
    ref_total = sum(len(b.valu) for b in isa_blocks.parse_blocks(asm[0], REFERENCE))
    print(kernel, "static VALU", total, "against", REFERENCE, ref_total)
    assert total < ref_total
