"""Where the vector instructions of one iteration of k_trace's persistent loop go, loop by loop: the static blocks of the device
assembly (tools/isa_blocks.py) times the trip structure of the contract workload C2, each loop's instructions split into

   arith    the reference's arithmetic: float add / sub / mul / fma / min / max, conversions, the division's own steps, and --
            in the hash loops -- the integer shifts, xors and adds of pcg
   cmp      comparisons (v_cmp*)
   book     bookkeeping: moves, selects, masks, guards, address arithmetic, lane operations
   slow     the instructions that issue over 8 cycles instead of 2 (isa_blocks.QUARTER_RATE: v_rcp, v_sqrt, v_mul_lo_u32 ...)

and priced at 2 cycles an instruction, 8 for the slow ones.  `salu` is the other stream: the scalar instructions of a trip
(isa_blocks' count: everything s_* but loads, waits and nops), which the four SIMDs of a CU hand to one scalar unit.  Trip counts: the two intersection loops are data-independent (12
triangles, 8 spheres, the phantom point light); the data-dependent ones are the phase counts of profiles/r15_ktrace_phases.txt
(executions per segment x 64, which is executions per iteration of a wavefront that enters with 63.6 lanes).  A trip of the
triangle loop does not run the compiler's division fallback (the blocks with v_div_scale), which the guard of the reciprocal
branches over; they are counted apart.

   python tools/ktrace_budget.py [build/rb_kernels.s] [kernel substring, default k_traceILb0ELb0ELi8]
"""
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import isa_blocks  # noqa: E402

TRIANGLES, SPHERES, LIGHTS = 12, 8, 1
# profiles/r15_ktrace_phases.txt, "this tree": executions per segment x 64
PASS2_TRIPS, LIGHT_PASS2_TRIPS, REJECTION_ROUNDS = 1.62, 0.0, 4.14

_ARITH = ("v_add_f32", "v_sub_f32", "v_subrev_f32", "v_mul_f32", "v_fma_f32", "v_fmac_f32", "v_mac_f32", "v_mad_f32", "v_min_f32", "v_max_f32",
          "v_med3_f32", "v_cvt_", "v_div_scale_f32", "v_div_fmas_f32", "v_div_fixup_f32", "v_ldexp_f32", "v_frexp_", "v_rndne_f32", "v_floor_f32",
          "v_fract_f32", "v_trunc_f32", "v_pk_")
_HASH = ("v_xor_b32", "v_lshrrev_b32", "v_lshlrev_b32", "v_add_u32", "v_mad_u32_u24", "v_mul_u32_u24", "v_add3_u32", "v_xad_u32", "v_lshl_add_u32",
         "v_mad_u64_u32", "v_alignbit_b32", "v_bfe_u32")


def classify(instr, hashes=False):
    """arith / cmp / book / slow for one vector instruction (None for anything else)"""
    op = instr.op
    if not op.startswith("v_"):
        return None
    if op.startswith(isa_blocks.QUARTER_RATE):
        return "slow"
    if op.startswith("v_cmp"):
        return "cmp"
    if op.startswith(_ARITH) or (hashes and op.startswith(_HASH)):
        return "arith"
    return "book"


def split(instrs, hashes=False):
    c = dict(arith=0, cmp=0, book=0, slow=0)
    for i in instrs:
        k = classify(i, hashes)
        if k:
            c[k] += 1
    return c


def inner_loops(blocks):
    """(header, body) of every innermost loop, in text order"""
    return [(h, isa_blocks.loop_blocks(blocks, h.name)) for h in blocks if h.inner_header]


def _ops(body):
    return [i.op for b in body for i in b.instrs]


def scan_loops(blocks):
    """k_trace's two-pass scans that follow the triangle loop, in text order: [(pass 1, pass 2) of the spheres, (pass 1,
    pass 2) of the point lights], each pass as (header, body).  Pass 1 is a one-block innermost loop that fetches its records
    with scalar loads and computes no reciprocal; pass 2 is the next innermost loop, the one with the square root."""
    tri, _ = isa_blocks.triangle_loop(blocks)
    loops = [l for l in inner_loops(blocks) if l[0].line > tri.line]
    out = []
    for k, (h, body) in enumerate(loops[:-1]):
        ops = _ops(body)
        if len(body) == 1 and any(o.startswith("s_load_dwordx4") for o in ops) and not any(o.startswith("v_rcp_f32") for o in ops):
            nh, nbody = loops[k + 1]
            if any(o.startswith("v_sqrt_f32") for o in _ops(nbody)):
                out.append(((h, body), (nh, nbody)))
    if not out:
        raise ValueError("no two-pass scan after the triangle loop")
    return out


def rejection_loop(blocks):
    """random_unit_vector's loop: the one-block innermost loop with 32-bit multiplies (three hashes) and no memory access"""
    for h, body in inner_loops(blocks):
        ops = _ops(body)
        if len(body) == 1 and sum(o.startswith("v_mul_lo_u32") for o in ops) >= 3 and not any(o.startswith(("s_load", "global_", "ds_", "scratch_")) for o in ops):
            return h, body
    raise ValueError("no rejection loop")


def rows(blocks):
    """(name, trips per iteration, instructions of one trip, hash loop?, scalar instructions of one trip) for every loop of the table"""
    tri_h, tri_body = isa_blocks.triangle_loop(blocks)
    fallback = [b for b in tri_body if any(i.op.startswith("v_div_scale") for i in b.instrs)]
    trip = [i for b in tri_body if b not in fallback for i in b.valu]
    scans = scan_loops(blocks)
    salu = lambda body: sum(b.counts()["salu"] for b in body)
    out = [(f"triangle loop {tri_h.name}, a trip", TRIANGLES, trip, False, salu([b for b in tri_body if b not in fallback])),
           (f"  its division fallback ({len(fallback)} blocks, branched over)", 0, [i for b in fallback for i in b.valu], False, salu(fallback))]
    names = ("sphere", "light")
    trips = ((SPHERES, PASS2_TRIPS), (LIGHTS, LIGHT_PASS2_TRIPS))
    for k, ((h1, b1), (h2, b2)) in enumerate(scans[:2]):
        out.append((f"{names[k]} scan pass 1 {h1.name}", trips[k][0], [i for b in b1 for i in b.valu], False, salu(b1)))
        out.append((f"{names[k]} scan pass 2 {h2.name}", trips[k][1], [i for b in b2 for i in b.valu], False, salu(b2)))
    rh, rbody = rejection_loop(blocks)
    out.append((f"rejection loop {rh.name}, a round", REJECTION_ROUNDS, [i for b in rbody for i in b.valu], True, salu(rbody)))
    counted = {id(i) for _, _, ins, _, _ in out for i in ins}
    in_loops = sum(r[4] for r in out)
    rest = [i for b in blocks for i in b.valu if id(i) not in counted]
    out.append(("everything else (static, every block once)", None, rest, True, salu(blocks) - in_loops))
    return out


def main():
    asm = sys.argv[1] if len(sys.argv) > 1 else "build/rb_kernels.s"
    kernel = sys.argv[2] if len(sys.argv) > 2 else "k_traceILb0ELb0ELi8"
    blocks = isa_blocks.parse_blocks(asm, kernel)
    print(f"# {kernel}: vector instructions per iteration of the persistent loop on C2, loop by loop (static count x trips)")
    print(f"{'loop':58s} {'trips':>6s} {'valu':>5s} {'arith':>6s} {'cmp':>5s} {'book':>5s} {'slow':>5s} {'salu':>5s} | {'valu/it':>8s} {'book/it':>8s} {'slow/it':>8s} {'cycles/it':>10s} {'salu/it':>8s}")
    tot = [0.0, 0.0, 0.0, 0.0, 0.0]
    for name, trips, instrs, hashes, salu in rows(blocks):
        c = split(instrs, hashes)
        n = sum(c.values())
        if trips is None:
            print(f"{name:58s} {'-':>6s} {n:5d} {c['arith']:6d} {c['cmp']:5d} {c['book']:5d} {c['slow']:5d} {salu:5d} |")
            continue
        per = [n * trips, c["book"] * trips, c["slow"] * trips, (2 * (n - c["slow"]) + 8 * c["slow"]) * trips, salu * trips]
        tot = [a + b for a, b in zip(tot, per)]
        print(f"{name:58s} {trips:6.2f} {n:5d} {c['arith']:6d} {c['cmp']:5d} {c['book']:5d} {c['slow']:5d} {salu:5d} | {per[0]:8.1f} {per[1]:8.1f} {per[2]:8.1f} {per[3]:10.1f} {per[4]:8.1f}")
    print(f"{'the loops above':58s} {'':6s} {'':5s} {'':6s} {'':5s} {'':5s} {'':5s} {'':5s} | {tot[0]:8.1f} {tot[1]:8.1f} {tot[2]:8.1f} {tot[3]:10.1f} {tot[4]:8.1f}")
    tri_h, tri_body = isa_blocks.triangle_loop(blocks)
    print("# bookkeeping and slow instructions of the intersection loops, by opcode (static, one trip):")
    for name, _, instrs, hashes, _ in rows(blocks)[:4]:
        if name.lstrip().startswith("its division"):
            continue
        ops = {}
        for i in instrs:
            if classify(i, hashes) in ("book", "slow"):
                ops[i.op] = ops.get(i.op, 0) + 1
        print(f"#   {name}: " + ", ".join(f"{o} {n}" for o, n in sorted(ops.items())))


if __name__ == "__main__":
    main()
