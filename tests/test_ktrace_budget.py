"""tools/ktrace_budget.py on the compiled k_trace (the Makefile's flags, as `make asm` compiles it), without a GPU:
 * the groups of the once-per-iteration path and the loop rows together cover every block inside the persistent loop, each block
   exactly once, and no block lands in the group without an anchor;
 * the loop rows are the ones the tool printed before it was extended: profiles/r27_ktrace_budget_before.txt carries them (its
   first lines are the unextended tool's output on the parent's assembly, line for line), and the change behind that profile left
   the loops alone -- trips and static counts are compared, the compiler's block labels are not;
 * every normalize site the kernel has is found: two in the unrolled refill rounds (stage_row), the sphere's and the light's
   normal, and the three of the scatter."""
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

BEFORE = os.path.join(ROOT, "profiles", "r27_ktrace_budget_before.txt")


@pytest.fixture(scope="module")
def asm(tmp_path_factory):
    hipcc, flags = _makefile_flags()
    if not (os.path.isfile(hipcc) or __import__("shutil").which(hipcc)):
        pytest.skip("hipcc is not installed")
    s = str(tmp_path_factory.mktemp("ktrace_budget") / "rb_kernels.s")
    subprocess.check_call([hipcc, *flags, "-S", "--cuda-device-only", "-o", s, os.path.join(ROOT, "renderbaby_amd/csrc/rb_kernels.hip")], cwd=ROOT)
    return s


@pytest.mark.parametrize("kernel", [k[0] for k in KERNELS])
def test_groups_and_loops_cover_the_loop_once(asm, kernel):
    blocks = isa_blocks.parse_blocks(asm, kernel)
    groups = ktrace_budget.once_groups(blocks)
    seen = {}
    for name, bs, ex, kind, why in groups:
        assert kind in ("measured", "assumed") and why and ex >= 0.0, name
        for b in bs:
            assert id(b) not in seen, (b.name, name, seen[id(b)])
            seen[id(b)] = name
    tri = isa_blocks.triangle_loop(blocks)[1]
    scans = ktrace_budget.scan_loops(blocks)
    in_rows = {id(b) for body in [tri, ktrace_budget.rejection_loop(blocks)[1]] + [l[1] for pair in scans[:2] for l in pair] for b in body}
    assert not in_rows & set(seen)
    inside = {id(b) for b in blocks if b.depth >= 1}
    outer = [b for b in blocks if b.depth == 1 and b.loop == b.name]
    # the drain loops behind the persistent loop are loops of their own, not part of it
    inside = {id(b) for b in blocks if b.depth >= 1 and (b.loop == outer[0].name or b.depth >= 2)}
    assert inside == in_rows | set(seen), [b.name for b in blocks if id(b) in inside ^ (in_rows | set(seen))]
    assert "unplaced" not in [g[0] for g in groups]
    print(kernel, len(groups), "groups,", len(seen), "blocks;", len(in_rows), "in the loop rows")


def _loop_rows(text):
    """(trips, valu, arith, cmp, book, slow) of the table's loop rows, in order"""
    out = []
    for l in text.split("\n"):
        m = re.match(r"^(?:triangle loop|  its division|sphere scan|light scan|rejection loop).*?\s(\d+\.\d\d)\s+(\d+)\s+(\d+)\s+(\d+)\s+(\d+)\s+(\d+)\s+\d+ \|", l)
        if m:
            out.append((float(m.group(1)),) + tuple(int(x) for x in m.groups()[1:]))
    return out


def test_loop_rows_are_the_unextended_tool_s(asm, capsys):
    want = _loop_rows(open(BEFORE).read())
    assert len(want) == 7, want
    old = sys.argv
    sys.argv = ["ktrace_budget.py", asm, KERNELS[0][0]]
    try:
        ktrace_budget.main()
    finally:
        sys.argv = old
    got = capsys.readouterr().out
    assert _loop_rows(got) == want
    assert "# the once-per-iteration path" in got and "vector instructions per iteration; measured" in got


def test_normalize_sites_are_found(asm):
    blocks = isa_blocks.parse_blocks(asm, KERNELS[0][0])
    names = [g[0] for g in ktrace_budget.once_groups(blocks) if g[0].startswith("normalize") and "compiler" not in g[0]]
    print(names)
    assert len([n for n in names if "stage_row" in n]) == 2
    assert any("sphere normal" in n for n in names) and any("light normal" in n for n in names)
    assert any("random_unit_vector" in n for n in names) and any("pt.d" in n for n in names) and any("is_metal" in n for n in names)
