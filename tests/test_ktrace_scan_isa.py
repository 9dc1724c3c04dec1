"""Guard on the compiled code of the two intersection loops of k_trace's default instantiations after their bookkeeping was
cut (no GPU: hipcc cross-compiles; the assembly is the fixture of tests/test_ktrace_isa.py, read through tools/isa_blocks.py
and the loop finders of tools/ktrace_budget.py).  Vector instructions per trip:
 * the sphere scan's pass 1: at most 20.  The parent's trip was 22; this build's is 18 -- the 16 of the reference's
   discriminant without the radius' square, the compare, and the add with carry that shifts the compare's bit in;
 * the triangle loop: at most 73, all 17 blocks of it, the division fallback included.  The parent's was 74; this build's
   is 72, the guard of the reciprocal being two compares where it was two masks and two compares;
 * pass 2 of the sphere scan holds no 32-bit integer multiply (the parent formed its record's address with one).
The point lights' scan, which the same kernels carry after the spheres', is the ascending scan as it was."""
import os
import sys

import pytest

from tests.test_ktrace_isa import asm  # noqa: F401  (the fixture: the device assembly built with the Makefile's flags)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import isa_blocks  # noqa: E402
import ktrace_budget  # noqa: E402

KERNELS = ["k_traceILb0ELb0ELi8", "k_traceILb0ELb0ELi6"]


def _valu(body):
    return [i for b in body for i in b.valu]


@pytest.mark.parametrize("kernel", KERNELS)
def test_sphere_scan_pass_1(asm, kernel):  # noqa: F811
    blocks = isa_blocks.parse_blocks(asm[0], kernel)
    (h1, pass1), _ = ktrace_budget.scan_loops(blocks)[0]
    trip = _valu(pass1)
    print(kernel, "sphere scan pass 1", h1.name, len(trip), "VALU:", " ".join(i.op for i in trip))
    assert len(trip) <= 20
    # the loop's bound and its record's address are the scalar unit's: no vector compare of integers, no vector move
    assert not [i.text for i in trip if i.op.startswith(("v_cmp_eq_u32", "v_cmp_ne_u32", "v_cmp_lt_u32", "v_cmp_gt_u32", "v_mov_b32"))]
    # one record of 16 bytes a trip, from one base pointer
    loads = [i for b in pass1 for i in b.instrs if i.op.startswith("s_load_")]
    assert [i.op for i in loads] == ["s_load_dwordx4"]


@pytest.mark.parametrize("kernel", KERNELS)
def test_triangle_trip(asm, kernel):  # noqa: F811
    blocks = isa_blocks.parse_blocks(asm[0], kernel)
    header, body = isa_blocks.triangle_loop(blocks)
    trip = _valu(body)
    print(kernel, "triangle loop", header.name, len(trip), "VALU,", sum(i.op.startswith("v_cmp") for i in trip), "compares")
    assert len(trip) <= 73


@pytest.mark.parametrize("kernel", KERNELS)
def test_sphere_scan_pass_2_has_no_32_bit_multiply(asm, kernel):  # noqa: F811
    blocks = isa_blocks.parse_blocks(asm[0], kernel)
    _, (h2, pass2) = ktrace_budget.scan_loops(blocks)[0]
    ops = [i.op for i in _valu(pass2)]
    print(kernel, "sphere scan pass 2", h2.name, len(ops), "VALU")
    assert any(o.startswith("v_sqrt_f32") for o in ops)
    assert not [o for o in ops if o.startswith(("v_mul_lo_u32", "v_mul_hi_u32", "v_mul_lo_i32", "v_mul_hi_i32", "v_mad_u64_u32", "v_mad_i64_i32"))]
