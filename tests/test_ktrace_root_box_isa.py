"""The root box in the compiled code of k_trace's two default instantiations (no GPU: hipcc cross-compiles with the Makefile's
flags; the assembly is read through tools/isa_blocks.py and tools/ktrace_budget.py, as tests/test_ktrace_budget.py reads it):
 * segment entry's three reciprocal sites and the slab arithmetic are one run of blocks that control enters at its head only,
   and the way into it from segment entry is scalar: the code in front ends in scalar conditional branches, one of which takes a
   wave whose lanes all have their answer to a block behind the run -- no vector instruction of the run is on that wave's path;
 * the static vector count of that wave's path through segment entry is below the parent's "segment entry and box test" row
   (profiles/r27_ktrace_budget_after.txt: 110), and is the count profiles/r29_ktrace_budget_after.txt records;
 * the two stage_row regions carry the test for the row's primaries, and nothing of it is taken for a normalize site."""
import os
import re
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import isa_blocks  # noqa: E402
import ktrace_budget  # noqa: E402

from tests.test_ktrace_isa import KERNELS, _makefile_flags  # noqa: E402

PARENT_ENTRY_VALU = 110
AFTER = os.path.join(ROOT, "profiles", "r29_ktrace_budget_after.txt")


@pytest.fixture(scope="module")
def asm(tmp_path_factory):
    hipcc, flags = _makefile_flags()
    if not (os.path.isfile(hipcc) or __import__("shutil").which(hipcc)):
        pytest.skip("hipcc is not installed")
    s = str(tmp_path_factory.mktemp("ktrace_root_box") / "rb_kernels.s")
    subprocess.check_call([hipcc, *flags, "-S", "--cuda-device-only", "-o", s, os.path.join(ROOT, "renderbaby_amd/csrc/rb_kernels.hip")], cwd=ROOT)
    return s


def _targets(b):
    return [(i.op, i.args.strip().lstrip(".L")) for i in b.instrs if i.op.startswith(("s_cbranch", "s_branch"))]


def _groups(blocks):
    return {name: (bs, ex) for name, bs, ex, kind, why in ktrace_budget.once_groups(blocks)}


@pytest.mark.parametrize("kernel", [k[0] for k in KERNELS])
def test_the_box_is_behind_one_scalar_way_in(asm, kernel):
    blocks = isa_blocks.parse_blocks(asm, kernel)
    idx = {b.name: k for k, b in enumerate(blocks)}
    g = _groups(blocks)
    box, ex = g["root box: reciprocals and slab test"]
    entry = g["segment entry and box test (from the refill's last memory access on: a new path's moves included)"][0]
    a, z = idx[box[0].name], idx[box[-1].name]
    assert [idx[b.name] for b in box] == list(range(a, z + 1))
    assert sum(ktrace_budget._n(b, "v_rcp_f32") for b in box) == 6 and sum(ktrace_budget._n(b, "v_div_fixup_f32") for b in box) == 3   # three sites, both ways
    assert ktrace_budget._is_slab(box[-1]) and ex == ktrace_budget.ROOT_BOX_SLAB_EXEC
    # control enters the run at its head only
    for k, b in enumerate(blocks):
        if a <= k <= z:
            continue
        for op, target in _targets(b):
            assert target not in idx or not (a < idx[target] <= z), (b.name, op, target)
    # every way to the head is a scalar branch or the fall-through of one, from blocks without a vector instruction behind the
    # rule's compares: the block in front ends in a scalar conditional branch that leaves for a block behind the run
    front = blocks[a - 1]
    leave = [t for op, t in _targets(front) if op.startswith("s_cbranch_") and t in idx and idx[t] > z]
    assert leave, (front.name, _targets(front))
    assert not [i.text for i in front.instrs if i.op.startswith(("s_and_saveexec", "s_or_saveexec", "s_andn2_saveexec"))]
    jumps_in = [b for k, b in enumerate(blocks) if not (a <= k <= z) and any(t == blocks[a].name for _, t in _targets(b))]
    for b in jumps_in:
        assert not b.valu, b.name     # scalar glue
    # the wave that leaves does not come back into the run
    seen, todo = set(), [idx[leave[0]]]
    t = idx[isa_blocks.triangle_loop(blocks)[0].name]
    while todo:
        k = todo.pop()
        if k in seen or k >= t or k < a:
            continue
        seen.add(k)
        assert not (a <= k <= z), blocks[k].name
        ends = _targets(blocks[k])
        todo += [idx[tg] for _, tg in ends if tg in idx]
        if not any(op == "s_branch" for op, _ in ends):
            todo.append(k + 1)
    path_valu = sum(len(b.valu) for b in entry)
    print(kernel, "box blocks", blocks[a].name, "..", blocks[z].name, "; segment entry without them:", path_valu, "vector instructions")
    assert path_valu < PARENT_ENTRY_VALU
    if kernel == KERNELS[0][0]:
        m = re.search(r"^segment entry and box test.*?\s(\d+)\s+(\d+)\s+(\d+)\s+(\d+)\s+\d+\.\d+ measured", open(AFTER).read(), re.M)
        assert m and int(m.group(2)) == path_valu, (m and m.groups(), path_valu)


@pytest.mark.parametrize("kernel", [k[0] for k in KERNELS])
def test_stage_row_carries_the_primaries_test(asm, kernel):
    blocks = isa_blocks.parse_blocks(asm, kernel)
    g = _groups(blocks)
    for rnd in (1, 2):
        bs, _ = g[f"row opening: root box of the row's 64 primaries (reciprocals, slab test), refill round {rnd}"]
        assert sum(ktrace_budget._n(b, "v_div_fixup_f32") for b in bs) == 3 and ktrace_budget._is_slab(bs[-1])
    names = [n for n in g if n.startswith("normalize") and "compiler" not in n]
    assert len([n for n in names if "stage_row" in n]) == 2 and len(names) == 7, names
    assert "unplaced" not in g
