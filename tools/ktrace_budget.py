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

Below the loops, the rest: every block on the once-per-iteration path of the persistent loop (depth 1, and the scaffolding of
the scans' block loops), grouped by the source region it comes from, with its static vector / scalar / slow counts and the
executions per iteration; the loops and the groups together are held against what the counters measured, 26.89 vector
wave-instructions per segment at 63.6 active lanes (profiles/r25_c2_pmc.json).  The regions are found from anchors in the
assembly, not from line tables: the loops above; the normalize sites (a block with three v_div_fixup_f32 -- the compiler's
division of three numerators -- and the root and reciprocal blocks around it); LDS and memory instructions (the colour ring's
drain, store and take; the texture lookup).  What an anchor cannot separate stays together and the group's name says so.
Executions are the phase rows of profiles/r15_ktrace_phases.txt where one exists ("measured"); everything else is marked
"assumed" with its reason.

k_trace_sift ("The triangle sift") has two loops where the others have the triangle loop: pass 1, a trip per
group of triangles (C2: six quads), and pass 2, a trip per candidate of the wave's busiest lane (SIFT_TRIPS, counted by
tools/tri_filter_stats.py on a sample of C2's rays).  The table has a row for each.

   python tools/ktrace_budget.py [build/rb_kernels.s] [kernel substring, default k_traceILb0ELb0ELi8] [measured VALU per segment, default 26.89]
"""
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import isa_blocks  # noqa: E402

TRIANGLES, SPHERES, LIGHTS = 12, 8, 1
# profiles/r15_ktrace_phases.txt, "this tree": executions per segment x 64
PASS2_TRIPS, LIGHT_PASS2_TRIPS, REJECTION_ROUNDS = 1.62, 0.0, 4.14
# k_trace_sift: C2's groups, and pass 2's trips per iteration (profiles/r33_tri_filter_stats.txt, waves of mixed segments)
SIFT_GROUPS, SIFT_TRIPS = 6, 3.88

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


def sift_loops(blocks):
    """k_trace_sift's two triangle loops as ((header, body) of pass 1, (header, body) of pass 2), or None for every other kernel.
    Pass 1 is the one-block innermost loop that fetches a 64-byte group record with one scalar load and shifts the group's bits in
    with v_alignbit_b32; pass 2 is the next innermost loop, the one that fetches its records per lane."""
    loops = inner_loops(blocks)
    for k, (h, body) in enumerate(loops[:-1]):
        ops = _ops(body)
        if len(body) == 1 and any(o.startswith("s_load_dwordx16") for o in ops) and any(o.startswith("v_alignbit_b32") for o in ops):
            nh, nbody = loops[k + 1]
            if any(o.startswith("global_load_dwordx4") for o in _ops(nbody)) and any(o.startswith("v_cmpx") for o in _ops(nbody)):
                return (h, body), (nh, nbody)
    return None


def triangle_loops(blocks):
    """the loops over the node's triangle list, in text order: the triangle loop, or the sift's two"""
    sift = sift_loops(blocks)
    return list(sift) if sift else [isa_blocks.triangle_loop(blocks)]


def scan_loops(blocks):
    """k_trace's two-pass scans that follow the triangle loop, in text order: [(pass 1, pass 2) of the spheres, (pass 1,
    pass 2) of the point lights], each pass as (header, body).  Pass 1 is a one-block innermost loop that fetches its records
    with scalar loads and computes no reciprocal; pass 2 is the next innermost loop, the one with the square root."""
    tri = triangle_loops(blocks)[-1][0]
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
    sift = sift_loops(blocks)
    tri_h, tri_body = sift[1] if sift else isa_blocks.triangle_loop(blocks)
    fallback = [b for b in tri_body if any(i.op.startswith("v_div_scale") for i in b.instrs)]
    trip = [i for b in tri_body if b not in fallback for i in b.valu]
    scans = scan_loops(blocks)
    salu = lambda body: sum(b.counts()["salu"] for b in body)
    out = []
    if sift:
        (h1, b1) = sift[0]
        out.append((f"sift pass 1 {h1.name}, a group", SIFT_GROUPS, [i for b in b1 for i in b.valu], False, salu(b1)))
    out += [(f"{'sift pass 2' if sift else 'triangle loop'} {tri_h.name}, a trip", SIFT_TRIPS if sift else TRIANGLES, trip, False,
             salu([b for b in tri_body if b not in fallback])),
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


# ---------------------------------------------------------------------------------------------- the once-per-iteration path
MEASURED_VALU_PER_SEGMENT, ACTIVE_LANES, SEGMENTS_PER_PATH = 26.89, 63.6, 5.155   # profiles/r25_c2_pmc.json; profiles/r15_ktrace_phases.txt
# iterations of C2 that still run the root box's slab path where a wave can branch past it (RB_ROOT_INSIDE): expected under 1 %
# (origins rounded onto a face, points under a resting sphere whose offset origin falls below the floor); not measured yet
ROOT_BOX_SLAB_EXEC = 0.0


def _has(b, *prefixes):
    return any(i.op.startswith(prefixes) for i in b.instrs)


def _n(b, prefix):
    return sum(i.op.startswith(prefix) for i in b.instrs)


def _memory(b):
    return _has(b, "ds_", "global_", "flat_", "buffer_", "scratch_")


def _three_quotients(b):
    """the compiler's division of three numerators by one denominator in one block (a normalize) -- not three reciprocals, whose
    v_div_fixup_f32 all end in the numerator 1.0 (stage_row's 1 / d for the root box of the row's primaries)"""
    fix = [i for i in b.instrs if i.op.startswith("v_div_fixup_f32")]
    return len(fix) == 3 and not all(i.args.replace(" ", "").endswith(",1.0") for i in fix)


def _three_reciprocals(b):
    fix = [i for i in b.instrs if i.op.startswith("v_div_fixup_f32")]
    return len(fix) == 3 and all(i.args.replace(" ", "").endswith(",1.0") for i in fix)


def normalize_sites(blocks):
    """[(first index, last index, index of the slow division)] of every normalize in text order.  A site's own blocks: the
    compiler's division of the three numerators (three v_div_fixup_f32), behind it the fast division (a v_rcp_f32, no
    v_div_scale_f32), in front of it the blocks of the two square roots, the guard of the division and the empty blocks of the
    exec-mask joins.  The dot product and the compares of the first guard sit in the block in front, with other code."""
    out = []
    for k, b in enumerate(blocks):
        if not _three_quotients(b) or _has(b, "v_cvt_f32_u32"):   # (hash_to_color divides three converted integers)
            continue
        first = k
        while first > 0:
            q = blocks[first - 1]
            nv = len(q.valu)
            fast_div = _has(q, "v_rcp_f32") and not _has(q, "v_div_scale_f32") and nv <= 20          # (laid out in front at some sites)
            if nv <= 4 or fast_div or (_has(q, "v_sqrt_f32") and nv <= 25) or (_has(q, "v_min3_u32") and nv <= 12):   # (<= 4: the significand test alone)
                first -= 1
            else:
                break
        last = k
        for j in range(k + 1, min(k + 3, len(blocks))):
            if _has(blocks[j], "v_rcp_f32") and not _has(blocks[j], "v_div_scale_f32") and len(blocks[j].valu) <= 20:
                last = j
                break
        out.append((first, last, k))
    return out


def _is_slab(b):
    """the slab arithmetic of isect_aabb: six subtractions, six multiplies and the min / max chains in one block"""
    return _n(b, "v_sub_f32") + _n(b, "v_subrev_f32") >= 6 and _has(b, "v_min_f32") and _has(b, "v_max_f32") and _has(b, "v_min3_f32", "v_max3_f32")


def root_box_span(blocks, lo, hi):
    """(first, last) index of the root box's blocks among blocks[lo:hi] -- the three rcp_exact sites (each a guard, the compiler's
    division of ONE numerator behind it, v_rcp_f32 and two fma beside it) and the slab arithmetic -- or None.  The division blocks
    hold one v_div_fixup_f32 each, so normalize_sites, which wants three in a block, does not take them for an anchor.  The guard
    of the first site belongs to the span where it has a block of its own (a build that branches past the box); where it shares
    its block with the code in front, it stays there."""
    slab = [k for k in range(lo, hi) if _is_slab(blocks[k])]
    if not slab:
        return None
    z = slab[0]
    if _three_reciprocals(blocks[z]):        # stage_row: 1 / d as three plain divisions, in the slab test's own block
        return (z, z)
    a = z
    while a - 1 >= lo:
        q = blocks[a - 1]
        one_div = _n(q, "v_div_fixup_f32") == 1 and _n(q, "v_div_scale_f32") == 2
        newton = _has(q, "v_rcp_f32") and not _has(q, "v_div_scale_f32") and len(q.valu) <= 4
        guard = _has(q, "v_and_b32") and _has(q, "v_cmp_") and len(q.valu) <= 6 and not _memory(q) and not _has(q, "v_cmp_o_f32", "v_cmp_u_f32")
        if one_div or newton or guard or not q.valu:
            a -= 1
        else:
            break
    while a < z and not blocks[a].valu:      # (scalar-only blocks in front belong to what branches here)
        a += 1
    sites = sum(_n(blocks[k], "v_div_fixup_f32") == 1 for k in range(a, z + 1))
    return (a, z) if sites == 3 else None


def _slow_path(b):
    """a block only lanes outside a guard run: the compiler's division, or its square root (the one that tests the class)"""
    return (_three_quotients(b) and not _has(b, "v_cvt_f32_u32")) or (_has(b, "v_sqrt_f32") and _has(b, "v_cmp_class_f32"))


def once_groups(blocks):
    """[(group name, blocks, executions per iteration, 'measured' | 'assumed', why)] covering every block of the persistent
    loop that no row of rows() counts, each block once; blocks outside the loop (set-up, the final drain) are not listed."""
    idx = {id(b): k for k, b in enumerate(blocks)}
    outer = next(b for b in blocks if b.depth == 1 and b.loop == b.name)
    tris = triangle_loops(blocks)
    tri_h = tris[0][0]
    scans = scan_loops(blocks)
    rh, rbody = rejection_loop(blocks)
    in_rows = {id(b) for body in [l[1] for l in tris] + [rbody] + [l[1] for pair in scans[:2] for l in pair] for b in body}
    tri_last = max(idx[id(b)] for l in tris for b in l[1])   # the sift: its block loop and pass 2's set-up lie between its two loops
    todo = [b for b in blocks if b.depth >= 1 and id(b) not in in_rows and (b.loop == outer.name or b.depth >= 2)]
    sites = normalize_sites(blocks)
    site_of = {}
    for n, (a, z, _) in enumerate(sites):
        for k in range(a, z + 1):
            site_of[k] = n
    h, t = idx[id(outer)], idx[id(tri_h)]
    s1, l2 = idx[id(scans[0][0][0])], idx[id(scans[min(1, len(scans) - 1)][1][0])]
    r = idx[id(rh)]
    pre = [n for n, (a, z, _) in enumerate(sites) if h <= a < t]          # stage_row's, one per unrolled refill round
    mid = [n for n, (a, z, _) in enumerate(sites) if l2 < a < r]          # the sphere's normal, then the light's
    post = [n for n, (a, z, _) in enumerate(sites) if a > r and blocks[a].depth >= 1 and blocks[a].loop == outer.name]
    # stage_row around its site: back to the last block with a memory or LDS access (open_row's drain), on to the ring store
    rows_span = []
    for n in pre:
        a, z, _ = sites[n]
        lo = a
        while lo - 1 > h and not _memory(blocks[lo - 1]):
            lo -= 1
        hi = z
        while hi + 1 < t and not _has(blocks[hi], "ds_"):
            hi += 1
        rows_span.append((lo, hi))
    # the second unrolled round starts as far in front of its stage_row as the first one does behind the loop's header
    round2 = rows_span[1][0] - (rows_span[0][0] - h) if len(rows_span) > 1 else t
    # segment entry: from the last memory access in front of the triangle loop on
    entry = t
    while entry - 1 > h and not _memory(blocks[entry - 1]) and not any(lo <= entry - 1 <= hi for lo, hi in rows_span):
        entry -= 1
    # the root box: in segment entry, and (a build that stages the primaries' answer) in each stage_row behind its normalize
    box_entry = root_box_span(blocks, entry, t)
    box_rows = [root_box_span(blocks, sites[n][1] + 1, hi + 1) for n, (lo, hi) in zip(pre, rows_span)]
    # ... which a wave whose lanes all have their answer branches past, where the rule's NaN test stands in front of it
    box_skipped = box_entry is not None and any(_has(blocks[k], "v_cmp_o_f32", "v_cmp_u_f32") for k in range(entry, box_entry[0]))
    tail_first = sites[post[-1]][1] + 1 if post else r + 1                # behind the last normalize: the path's end
    scatter = (sites[post[1]][1] + 1, sites[post[-1]][0] - 1) if len(post) >= 3 else (0, -1)
    tex = [k for k in range(scatter[0], scatter[1] + 1) if _has(blocks[k], "global_load", "flat_load", "buffer_load")]
    names = {0: "normalize: random_unit_vector", 1: "normalize: is_metal ? d : normal + ruv", 2: "normalize: pt.d = scattered"}
    groups, order = {}, []

    def put(name, b, ex, kind, why):
        if name not in groups:
            groups[name] = [[], ex, kind, why]
            order.append(name)
        groups[name][0].append(b)

    row_ex = 1.0 / SEGMENTS_PER_PATH
    for b in todo:
        k = idx[id(b)]
        if k in site_of and site_of[k] in pre + mid + post:
            n = site_of[k]
            if n in pre:
                which, ex, kind, why = f"normalize: stage_row, refill round {pre.index(n) + 1}", row_ex if pre.index(n) == 0 else 0.0, "assumed", \
                    "a row of 64 paths is opened per 64 paths of 5.155 segments" if pre.index(n) == 0 else "a reservation ends once in queue_batch items"
            elif n in mid:
                which = ("normalize: sphere normal", "normalize: light normal")[min(mid.index(n), 1)]
                ex, kind, why = (1.0, "assumed", "a wave with no sphere winner skips it; 8.4 lanes have candidates") if mid.index(n) == 0 else \
                    (LIGHT_PASS2_TRIPS, "measured", "light pass 2: C2's phantom light is never a candidate")
            else:
                which = names.get(post.index(n) if post.index(n) < 2 else (2 if n == post[-1] else 9), "normalize: scatter branch")
                ex, kind, why = 1.01, "measured", "shading / scatter rows"
            if _slow_path(b):
                put(which + ", compiler's path", b, 0.0, "assumed", "every lane inside the guards; a zero component or an all-ones significand would enter")
            else:
                put(which, b, ex, kind, why)
        elif k < h:
            put("blocks laid out in front of the loop's header (the join behind a finished path)", b, 1.0, "assumed", "the loop's latch")
        elif _three_quotients(b):
            put("resolve and material: hash_to_color", b, 0.0, "assumed", "C2 renders without the colour hash")
        elif h <= k < t:
            in_row = [n for n, (lo, hi) in enumerate(rows_span) if lo <= k <= hi]
            if in_row:
                first = in_row[0] == 0
                staged = box_rows[in_row[0]]
                if staged and staged[0] <= k <= staged[1]:
                    put(f"row opening: root box of the row's 64 primaries (reciprocals, slab test), refill round {in_row[0] + 1}", b, row_ex if first else 0.0,
                        "assumed", "1 / 5.155; the divisions behind the reciprocals' guards are branched over" if first else "second round: not reached")
                else:
                    put(f"row opening: stage_row to the ring store, refill round {in_row[0] + 1}", b, row_ex if first else 0.0, "assumed",
                        "1 / 5.155" if first else "second round: not reached")
            elif box_entry and box_entry[0] <= k <= box_entry[1]:
                if box_skipped:
                    put("root box: reciprocals and slab test", b, ROOT_BOX_SLAB_EXEC, "assumed",
                        "only a wave with a lane that has no answer: C2's secondary rays start inside the box, its primaries' answers are staged")
                else:
                    put("root box: reciprocals and slab test", b, 1.01, "measured", "segment entry row; the divisions are branched over")
            elif k >= entry:
                put("segment entry and box test (from the refill's last memory access on: a new path's moves included)", b, 1.01, "measured", "segment entry row")
            elif k >= round2:
                put("refill round 2, open_row's drain, ColorRing::take", b, 0.0, "assumed", "runs when a reservation ends inside a round: once in queue_batch items")
            else:
                put("refill round 1, open_row's drain, ColorRing::take", b, 1.0, "assumed", "12.3 lanes end a path per iteration: some lane is idle")
        elif len(tris) > 1 and t < k < tri_last:
            put("sift: the list's block loop, pass 1's exit and pass 2's set-up", b, 1.0, "assumed", "one block of 32 slots")
        elif t < k < s1:
            put("segment_pre: ground, triangle winner", b, 1.01, "measured", "segment entry row")
        elif s1 <= k <= l2 + 8 and b.depth >= 2:
            put("scan block loops and pass 2 set-up (depth 2 and 3)", b, 1.0, "assumed", "one block of 32 spheres, one of lights")
        elif k < r and (not mid or k < sites[mid[0]][0]):
            put("resolve and material", b, 1.01, "measured", "shading row")
        elif k < r and mid and k <= sites[mid[-1]][1]:
            put("resolve and material: between the two normal sites", b, 1.0, "assumed", "load_mat of a sphere; the light's is never entered")
        elif k < r:
            put("emission and the first try of random_unit_vector", b, 1.01, "measured", "unit vector: the first try")
        elif post and k < sites[post[0]][0]:
            put("rejection loop exit: dot product of the accepted point", b, 1.01, "measured", "unit vector row")
        elif len(post) >= 2 and k < sites[post[1]][0]:
            put("scatter operand: normal + ruv, select, dot product, guards", b, 1.01, "measured", "shading row")
        elif scatter[0] <= k <= scatter[1]:
            if tex and tex[0] <= k <= tex[-1]:
                put("lambert branch: texture lookup", b, 0.0, "assumed", "C2 has no texture")
            else:
                put("metal branch and lambert branch (arithmetic; the layout does not separate them)", b, 1.0, "assumed", "metal 0.93 and lambert 1.01 measured, the split is not")
        elif k >= tail_first:
            put("path end", b, 1.01, "measured", "path end row")
        else:
            put("unplaced", b, 1.0, "assumed", "no anchor")
    return [(name, *groups[name]) for name in order]


def print_once(blocks, loops_valu, measured=MEASURED_VALU_PER_SEGMENT):
    print("# the once-per-iteration path, by source region (static counts; executions per iteration, measured = a phase row of profiles/r15_ktrace_phases.txt)")
    print(f"{'group':108s} {'blocks':>6s} {'valu':>5s} {'salu':>5s} {'slow':>5s} {'exec/it':>8s} {'':9s} | {'valu/it':>8s}")
    total = 0.0
    for name, bs, ex, kind, why in once_groups(blocks):
        valu = sum(len(b.valu) for b in bs)
        salu = sum(b.counts()["salu"] for b in bs)
        slow = sum(b.counts()["quarter"] for b in bs)
        total += valu * ex
        print(f"{name[:108]:108s} {len(bs):6d} {valu:5d} {salu:5d} {slow:5d} {ex:8.3f} {kind:9s} | {valu * ex:8.1f}   # {bs[0].name}..{bs[-1].name}: {why}")
    want = measured * ACTIVE_LANES
    have = loops_valu + total
    print(f"{'the groups above':108s} {'':6s} {'':5s} {'':5s} {'':5s} {'':8s} {'':9s} | {total:8.1f}")
    print(f"# loops {loops_valu:.1f} + groups {total:.1f} = {have:.1f} vector instructions per iteration; measured {measured} x {ACTIVE_LANES} = {want:.1f}: "
          f"{100.0 * (have - want) / want:+.1f} %")
    if abs(have - want) > 0.05 * want:
        loose = sorted(((sum(len(b.valu) for b in bs) * ex, name) for name, bs, ex, kind, _ in once_groups(blocks) if ex > 0 and "normalize" not in name), reverse=True)[:5]
        print(f"# OUTSIDE 5 %: {have - want:+.1f} instructions are unexplained.  The groups that can hold them are the ones whose blocks are not all run by every")
        print("# iteration and which the anchors cannot split further (ground test, the light's material, the `use_tex` and padding ways, the take of a lane):")
        for v, name in loose:
            print(f"#   {v:7.1f}  {name}")


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
    print("# bookkeeping and slow instructions of the intersection loops, by opcode (static, one trip):")
    for name, _, instrs, hashes, _ in rows(blocks)[:5 if sift_loops(blocks) else 4]:
        if name.lstrip().startswith("its division"):
            continue
        ops = {}
        for i in instrs:
            if classify(i, hashes) in ("book", "slow"):
                ops[i.op] = ops.get(i.op, 0) + 1
        print(f"#   {name}: " + ", ".join(f"{o} {n}" for o, n in sorted(ops.items())))
    print_once(blocks, tot[0], float(sys.argv[3]) if len(sys.argv) > 3 else MEASURED_VALU_PER_SEGMENT)


if __name__ == "__main__":
    main()
