"""Basic blocks of one kernel in the device assembly (`make asm` -> build/rb_kernels.s, build/resource_usage.txt): per block
its VALU instructions split into v_mov / v_cndmask / lane operations / quarter-rate / the rest, its scalar, scalar-memory,
vector-memory, LDS and scratch instructions, and the loop it belongs to (from the compiler's own loop comments).  The
attribution table (this file run as a script) and the guard test (tests/test_ktrace_isa.py) read the ISA through here.

   python tools/isa_blocks.py [build/rb_kernels.s] [kernel substring, default k_traceILb0ELb0ELi8]     the table, per block
"""
import re
import sys
from collections import namedtuple

# issued at a quarter of the plain rate: the 1 228.8 G wave-instructions/s VALU peak assumes none of them
QUARTER_RATE = ("v_rcp_", "v_rsq_", "v_sqrt_", "v_mul_lo_u32", "v_mul_hi_u32", "v_mul_hi_i32", "v_div_scale_f64", "v_exp_", "v_log_",
                "v_sin_", "v_cos_")
LANE_OPS = ("v_readlane_", "v_writelane_", "v_readfirstlane_", "v_permlane", "v_mov_b32_dpp", "v_bpermute")
DPP_WORDS = ("quad_perm:", "row_shl:", "row_shr:", "row_ror:", "row_bcast:", "wave_shl:", "wave_shr:", "row_mirror", "row_half_mirror",
             "row_newbcast:")

Instr = namedtuple("Instr", "line op args text")
_LABEL = re.compile(r"^(\.LBB\d+_\d+):")
_ASM_LABEL = re.compile(r"^(\.L\w+):")
_FALL = re.compile(r"^; (%bb\.\d+):")
_INLOOP = re.compile(r"in Loop: Header=(BB\d+_\d+) Depth=(\d+)")
_HEADER = re.compile(r"This (Inner )?Loop Header: Depth=(\d+)")


class Block:
    def __init__(self, name, line):
        self.name, self.line = name, line
        self.instrs = []
        self.loop = None          # label (without the dot) of the innermost loop's header, None outside every loop
        self.depth = 0
        self.inner_header = False  # header of a loop without child loops

    def _ops(self, pred):
        return [i for i in self.instrs if pred(i)]

    @property
    def valu(self):
        return self._ops(lambda i: i.op.startswith("v_"))

    def counts(self):
        c = dict(valu=0, mov=0, cndmask=0, lane=0, quarter=0, rest=0, salu=0, smem=0, vmem=0, lds=0, scratch=0, wait=0)
        for i in self.instrs:
            op = i.op
            if op.startswith("v_"):
                c["valu"] += 1
                if op.startswith(LANE_OPS) or any(w in i.args for w in DPP_WORDS):
                    c["lane"] += 1
                elif op.startswith("v_mov_b32") or op.startswith("v_mov_b64"):
                    c["mov"] += 1
                elif op.startswith("v_cndmask"):
                    c["cndmask"] += 1
                elif op.startswith(QUARTER_RATE):
                    c["quarter"] += 1
                else:
                    c["rest"] += 1
            elif op.startswith("scratch_"):
                c["scratch"] += 1
            elif op.startswith(("global_", "flat_", "buffer_")):
                c["vmem"] += 1
            elif op.startswith("ds_"):
                c["lds"] += 1
            elif op.startswith(("s_load_", "s_buffer_load_")):
                c["smem"] += 1
            elif op == "s_waitcnt":
                c["wait"] += 1
            elif op.startswith("s_") and op != "s_nop":
                c["salu"] += 1
        return c


def kernel_lines(asm_path, kernel):
    """(first line number, lines) of the one function whose mangled name contains `kernel`, label to .Lfunc_end."""
    lines = open(asm_path).read().split("\n")
    starts = [n for n, l in enumerate(lines) if (m := re.match(r"^(_Z\w+):", l)) and kernel in m.group(1)]
    if len(starts) != 1:
        raise ValueError(f"{len(starts)} functions match {kernel!r} in {asm_path}")
    n0 = starts[0]
    n1 = next(n for n in range(n0, len(lines)) if lines[n].startswith(".Lfunc_end"))
    return n0 + 1, lines[n0:n1]


def parse_blocks(asm_path, kernel):
    """The function's basic blocks in text order: a block starts at a label (.LBBx_y) or at a fall-through mark (; %bb.n)."""
    first, lines = kernel_lines(asm_path, kernel)
    blocks = [Block("entry", first)]
    in_asm = False
    for k, l in enumerate(lines[1:], 1):
        # an inline-asm statement (#ASMSTART .. #ASMEND) can hold branches and labels of its own (accept_trip): a label in it
        # starts a block like any other, which belongs to the loop of the block the statement stands in
        if l.strip().startswith(";;#ASM"):
            in_asm = "#ASMSTART" in l
            continue
        am = _ASM_LABEL.match(l) if in_asm else None
        if am:
            b = Block(am.group(1)[2:], first + k)
            b.loop, b.depth = blocks[-1].loop, blocks[-1].depth
            blocks.append(b)
            continue
        m = _LABEL.match(l) or _FALL.match(l)
        if m:
            b = Block(m.group(1)[2:] if m.group(1).startswith(".L") else m.group(1), first + k)   # .LBB29_5 -> BB29_5, as in the loop comments
            blocks.append(b)
            lm = _INLOOP.search(l)
            if lm:
                b.loop, b.depth = lm.group(1), int(lm.group(2))
            continue
        b = blocks[-1]
        if l.startswith(" ") and ";" in l and not l.strip().startswith(";;"):   # continuation of the block's loop comment
            hm = _HEADER.search(l)
            if hm:
                b.loop, b.depth, b.inner_header = b.name, int(hm.group(2)), bool(hm.group(1))
            continue
        if not l.startswith("\t"):
            continue
        text = l.split(";")[0].strip()
        if not text or text.startswith("."):
            continue
        parts = text.split(None, 1)
        b.instrs.append(Instr(first + k, parts[0], parts[1] if len(parts) > 1 else "", text))
        if in_asm and parts[0].startswith("s_cbranch"):   # what follows a branch of the statement's own is the fall-through block
            nb = Block(b.name + ".fall", first + k + 1)
            nb.loop, nb.depth = b.loop, b.depth
            blocks.append(nb)
    # a header written on the label's own line ("; =>This Inner Loop Header: Depth=1")
    for b in blocks:
        l = lines[b.line - first]
        hm = _HEADER.search(l)
        if hm:
            b.loop, b.depth, b.inner_header = b.name, int(hm.group(2)), bool(hm.group(1))
    return blocks


def loop_blocks(blocks, header):
    """Blocks of the loop whose header block is named `header` (innermost membership, as the compiler prints it)."""
    return [b for b in blocks if b.loop == header]


def triangle_loop(blocks):
    """The single-node walk's triangle loop of k_trace: the first innermost loop in text order (the refill rounds are unrolled
    and the sphere and light loops follow it) that fetches with scalar loads and computes a reciprocal."""
    for h in (b for b in blocks if b.inner_header):
        body = loop_blocks(blocks, h.name)
        ops = [i.op for b in body for i in b.instrs]
        if any(o.startswith("s_load_dwordx") for o in ops) and any(o.startswith("v_rcp_f32") for o in ops):
            return h, body
    raise ValueError("no innermost loop with scalar loads and a reciprocal")


def resource_usage(path, kernel):
    """The -Rpass-analysis=kernel-resource-usage remarks of one function as a dict (ints where they are numbers)."""
    out, on = {}, False
    for l in open(path):
        m = re.search(r"remark:\s+(.*?) \[-Rpass-analysis", l)
        if not m:
            continue
        t = m.group(1)
        if t.startswith("Function Name:"):
            on = kernel in t
        elif on and ": " in t:
            k, v = t.rsplit(": ", 1)
            out[k.strip()] = int(v) if v.isdigit() else v
    if not out:
        raise ValueError(f"no resource remarks for {kernel!r} in {path}")
    return out


def main():
    asm = sys.argv[1] if len(sys.argv) > 1 else "build/rb_kernels.s"
    kernel = sys.argv[2] if len(sys.argv) > 2 else "k_traceILb0ELb0ELi8"
    blocks = parse_blocks(asm, kernel)
    cols = ("valu", "mov", "cndmask", "lane", "quarter", "rest", "salu", "smem", "wait", "vmem", "lds", "scratch")
    print(f"# {kernel}: static instruction counts per basic block (text order); loop = innermost loop header, depth")
    print(f"{'block':12s} {'loop':12s} {'d':>2s} " + " ".join(f"{c:>7s}" for c in cols))
    tot = dict.fromkeys(cols, 0)
    for b in blocks:
        c = b.counts()
        if not b.instrs:
            continue
        for k in cols:
            tot[k] += c[k]
        print(f"{b.name:12s} {(b.loop or '-'):12s} {b.depth:2d} " + " ".join(f"{c[k]:7d}" for k in cols))
    print(f"{'total':12s} {'':12s} {'':2s} " + " ".join(f"{tot[k]:7d}" for k in cols))
    h, body = triangle_loop(blocks)
    t = dict.fromkeys(cols, 0)
    for b in body:
        for k, v in b.counts().items():
            if k in t:
                t[k] += v
    print(f"# triangle loop {h.name}: {len(body)} blocks, one trip through every block: " + ", ".join(f"{k} {t[k]}" for k in cols))


if __name__ == "__main__":
    main()
