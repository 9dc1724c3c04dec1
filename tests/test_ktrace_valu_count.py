"""The static count of vector instructions in k_trace's three non-counting instantiations (no GPU: hipcc cross-compiles).
k_trace is bound by VALU issue, and the code after the intersections runs once per iteration of its persistent loop at
wave cost whatever the number of lanes in each branch, so every vector instruction that stays in the binary there is
paid for.  The bound is the count of the parent of the commit that gave the two scatter branches one normalize between them
(2 135, 2 135 and 3 253, read through tools/isa_blocks.py; profiles/r19_ktrace_blocks_before.txt): no change to the shared shading
code may leave these kernels with more vector instructions than they had then.  It is a ceiling, not a record of the present
count (2 055 when this was written, profiles/r19_ktrace_blocks_after.txt): giving the saved instructions back would still pass.
The triangle loop, which that work left alone, stays at the parent's 74 (98 with the multi-node walks inlined) per trip."""
import pytest

from tests.test_ktrace_isa import asm, isa_blocks  # noqa: F401  (the fixture: the device assembly built with the Makefile's flags)

# (mangled-name part, the parent's static VALU count, the parent's VALU per trip of the triangle loop)
PARENT = [("k_traceILb0ELb0ELi8", 2135, 74), ("k_traceILb0ELb0ELi6", 2135, 74), ("k_traceILb0ELb1ELi6", 3253, 98)]


@pytest.mark.parametrize("kernel,valu,loop_valu", PARENT)
def test_static_valu_not_above_the_parent(asm, kernel, valu, loop_valu):  # noqa: F811
    blocks = isa_blocks.parse_blocks(asm[0], kernel)
    total = sum(len(b.valu) for b in blocks)
    _, body = isa_blocks.triangle_loop(blocks)
    trip = sum(len(b.valu) for b in body)
    print(kernel, "static VALU", total, "parent", valu, "| triangle loop", trip, "parent", loop_valu)
    assert total <= valu
    assert trip <= loop_valu
