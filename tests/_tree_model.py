"""The invariants of the library's own triangle tree and of its sphere tree (section 4.3), checked on
a read-back in plain numpy: float64 on the f32 inputs, iterative traversal, no call into the library.  Each check returns None
or a short reason that names the first violation.

What the walks trust and nothing else reads back: every valid slot in exactly one leaf, every child box over everything below
it, FA not under the largest F_k below, +inf where no finite bound is claimed, mesh bounds over the mesh, a depth that covers
the walk's stack; for the spheres a permutation, the spheres' own bytes, leaves that tile, boxes that contain c -+ r, the split
the ray order assumes and the stack entries of the levels."""
import numpy as np

LEAF = 0x80000000
NONE = 0xFFFFFFFF
FA_LIMIT = 1.5e5            # beyond it FA is +inf: the walk always enters (FastWalk::entry)
GRAZE_COS = float(np.float32(0.03))   # c0, kFastGrazeCos as the builders read it
SUBNORMAL = 2.0 ** -149     # the f32 grid's finest step: no f32 rounding can be finer
SPH_LEAF = 16


def ulp32(x):
    """spacing of f32 at |x| (the smallest subnormal at 0)"""
    return float(np.spacing(np.float32(abs(float(x)))))


# ---------------------------------------------------------------- shared traversal ---
def _walk(root, n_nodes, children, is_leaf):
    """Pre-order list of the reachable nodes, or (None, reason).  children(i) -> the references node i holds."""
    if is_leaf(root):
        return [], None
    order, seen, stack = [], np.zeros(n_nodes, bool), [int(root)]
    if root >= n_nodes:
        return None, f"root {root} is not a node (of {n_nodes})"
    seen[root] = True
    while stack:
        i = stack.pop()
        order.append(i)
        for r in children(i):
            if is_leaf(r):
                continue
            if r >= n_nodes:
                return None, f"node {i} references node {r} of {n_nodes}"
            if seen[r]:
                return None, f"node {r} referenced twice"
            seen[r] = True
            stack.append(int(r))
    return order, None


def _tiling(leaves, n, what):
    """leaves: [(first, count, where)]: they must cover [0, n) once"""
    at = 0
    for first, count, where in sorted(leaves):
        if first != at:
            return f"{what}: leaf range [{first}, {first + count}) of {where} {'overlaps its neighbour' if first < at else 'leaves a gap'} at {at}"
        at = first + count
    if at != n:
        return f"{what}: the leaves cover [0, {at}) of [0, {n})"
    return None


# -------------------------------------------------------------------- the own tree ---
def tri_bounds(tris, indices, slots, slot_meta):
    """per position of `slots`: (vmin[n,3], vmax[n,3], F[n], Q[n]) in float64 -- the tight box of the f32 vertices; F_k of DESIGN.md
    section 4.1 (A) from the f32 edges: L^2 / 1e-6 for a small triangle, (L^2 / N) / (0.95 c0) for a large one, +inf at N = 0; and
    Q_k, F_k with the builders' documented outward factors, the value they round to f32: (1 + 1e-5)(1 + 1e-6) small, (1 + 1e-5) large."""
    t = tris[indices[slots]]
    v = np.stack([t["v0"], t["v1"], t["v2"]], axis=1).astype(np.float32)
    e1, e2 = (v[:, 1] - v[:, 0]).astype(np.float64), (v[:, 2] - v[:, 0]).astype(np.float64)   # subtracted in f32, as k_prep_tris does
    ll = np.maximum((e1 * e1).sum(1), (e2 * e2).sum(1))
    nn = np.sqrt((np.cross(e1, e2) ** 2).sum(1))
    large = (slot_meta[2 * slots.astype(np.int64) + 1] & 0x80000000) != 0
    with np.errstate(divide="ignore", invalid="ignore"):
        f_large = np.where(nn > 0.0, ll / nn / (0.95 * GRAZE_COS), np.inf)
    f = np.where(large, f_large, ll / 1e-6)
    q = np.where(large, f_large * (1.0 + 1e-5), ll * 1e6 * (1.0 + 1e-5) * (1.0 + 1e-6))
    v64 = v.astype(np.float64)
    return v64.min(1), v64.max(1), f, q


def fa_verdict(fa, exact, rounded=None):
    """FA against the exact largest F_k below (and `rounded`, the largest Q_k below): None or the reason.  The builders round Q to
    f32, never below it, and store +inf when that exceeds 1.5e5: FA >= exact hard, FA no more than half an f32 ulp under Q (a
    conversion to nearest loses no more; this is what tells an FA that was lowered by one ulp), FA <= exact (1 + 2e-5) (plus the
    f32 grid's finest step, which no rounding can undercut), +inf exactly when the rounded value is beyond 1.5e5 -- either answer
    where the exact value lies within that slack of 1.5e5."""
    fa, exact = float(fa), float(exact)
    if np.isnan(fa):
        return "FA is NaN"
    hi = exact * (1.0 + 2e-5) + SUBNORMAL
    if exact > FA_LIMIT:
        return None if fa == np.inf else f"FA {fa!r} finite where +inf is due (largest F_k below {exact!r})"
    if fa == np.inf:
        return None if hi > FA_LIMIT else f"FA +inf where a finite bound is due (largest F_k below {exact!r})"
    if fa < exact:
        return f"FA {fa!r} below the largest F_k below it {exact!r}"
    if rounded is not None and rounded <= FA_LIMIT and fa < float(rounded) * (1.0 - 1e-13) - 0.5 * ulp32(fa) * (1.0 + 1e-9):
        return f"FA {fa!r} below the f32 of the builders' outward-rounded bound {float(rounded)!r}"
    if fa > hi:
        return f"FA {fa!r} above (1 + 2e-5) times the largest F_k below it {exact!r}"
    if fa > FA_LIMIT:
        return f"FA {fa!r} finite above 1.5e5"
    return None


def check_own_tree(nodes, slots, slot_meta, root, depth, bmin, bmax, tris, indices, tri_count, report=None):
    """None, or the first violated invariant of the library's own triangle tree.  `report`, a dict, receives need (internal
    nodes on the longest root-to-leaf path = the stack entries a walk can hold) and excess = depth - need."""
    slots = np.asarray(slots, dtype=np.uint32)
    n, index_len = len(slots), len(indices)
    # ---- slots: a permutation of exactly the valid slots
    if len(slot_meta) != 2 * index_len:
        return f"slot_meta has {len(slot_meta)} words for {index_len} index slots"
    if n and int(slots.max()) >= index_len:
        return f"slots holds {int(slots.max())}, beyond the {index_len} index slots"
    valid = np.flatnonzero((np.asarray(indices) < tri_count) & (slot_meta[0::2] != NONE))
    s_sorted = np.sort(slots)
    dup = np.flatnonzero(s_sorted[1:] == s_sorted[:-1])
    if len(dup):
        return f"slots holds slot {int(s_sorted[dup[0]])} twice"
    if len(s_sorted) != len(valid) or not np.array_equal(s_sorted, valid):
        missing, extra = np.setdiff1d(valid, s_sorted), np.setdiff1d(s_sorted, valid)
        return f"slots is not the valid slots: {len(missing)} missing (first {missing[:1]}), {len(extra)} not valid (first {extra[:1]})"
    # ---- reachability and leaves
    is_leaf = lambda r: bool(int(r) & LEAF)
    order, why = _walk(int(root), len(nodes), lambda i: (nodes["left"][i], nodes["right"][i]), is_leaf)
    if order is None:
        return why
    left, right = nodes["left"], nodes["right"]
    refs = [(int(root), "the root")] if is_leaf(root) else [(int(r), f"node {i}") for i in order for r in (left[i], right[i]) if is_leaf(r)]
    leaves = []
    for r, where in refs:
        count, first = ((r >> 28) & 7) + 1, r & 0x0FFFFFFF
        if count > 2:
            return f"leaf {r:#x} of {where} holds {count} triangles"
        leaves.append((first, count, where))
    why = _tiling(leaves, n, "own tree")
    if why:
        return why
    # ---- per subtree, bottom-up: box, largest F_k, internal nodes on the longest path
    vmin, vmax, f, q = tri_bounds(tris, np.asarray(indices), slots, slot_meta)

    def leaf_stat(r):
        first, count = r & 0x0FFFFFFF, ((r >> 28) & 7) + 1
        sl = slice(first, first + count)
        return vmin[sl].min(0), vmax[sl].max(0), float(f[sl].max()), 0, float(q[sl].max())

    stat = {}
    fields = (("lmin", "lmax", "left_fa", "left"), ("rmin", "rmax", "right_fa", "right"))
    for i in reversed(order):
        got = []
        for f_min, f_max, f_fa, f_ref in fields:
            r = int(nodes[f_ref][i])
            mn, mx, fk, need, qk = leaf_stat(r) if is_leaf(r) else stat.pop(r)
            side = f"node {i} {f_ref}"
            if not (np.array_equal(nodes[f_min][i].astype(np.float64), mn) and np.array_equal(nodes[f_max][i].astype(np.float64), mx)):
                return f"{side}: box {nodes[f_min][i]} .. {nodes[f_max][i]} is not the triangles' {mn.astype(np.float32)} .. {mx.astype(np.float32)}"
            why = fa_verdict(nodes[f_fa][i], fk, qk)
            if why:
                return f"{side}: {why}"
            got.append((mn, mx, fk, need, qk))
        (amn, amx, af, an, aq), (bmn, bmx, bf, bn, bq) = got
        stat[i] = (np.minimum(amn, bmn), np.maximum(amx, bmx), max(af, bf), 1 + max(an, bn), max(aq, bq))
    mn, mx, _, need, _ = leaf_stat(int(root)) if is_leaf(root) else stat[int(root)]
    # ---- mesh bounds, depth
    if not (np.array_equal(np.asarray(bmin, np.float64), mn) and np.array_equal(np.asarray(bmax, np.float64), mx)):
        return f"mesh bounds {np.asarray(bmin)} .. {np.asarray(bmax)} are not the mesh's {mn.astype(np.float32)} .. {mx.astype(np.float32)}"
    if report is not None:
        report.update(need=need, excess=int(depth) - need)
    if depth < need:
        return f"depth {depth} does not cover the {need} internal nodes of the longest path"
    return None


# ----------------------------------------------------------------- the sphere tree ---
def set_box(lo, hi):
    """SphereNode4::set_box in its own f32 arithmetic (no fused operations): centre and half extent of [lo, hi]"""
    lo, hi, half = np.float32(lo), np.float32(hi), np.float32(0.5)
    m = half * lo + half * hi
    d = max(m - lo, hi - m)
    return m, (d * np.float32(1.0000004) + np.float32(1e-37) if d >= 0 else np.float32(0.0))


def longest_axis(lo, hi):
    """the builders' rule on the f32 extents of the centres' bounds: x if strictly longest, else y if longer than z, else z"""
    e = np.asarray(hi, np.float32) - np.asarray(lo, np.float32)
    return 0 if (e[0] > e[1] and e[0] > e[2]) else (1 if e[1] > e[2] else 2)


def check_sphere_tree(nodes, leaf, ids, root, depth, spheres, axis_rule=True):
    """None, or the first violated invariant of the sphere tree over `spheres` (abi.SPHERE[])."""
    n = len(spheres)
    ids = np.asarray(ids)
    if len(ids) != n or len(leaf) != n:
        return f"{len(ids)} ids and {len(leaf)} leaf records for {n} spheres"
    if not np.array_equal(np.sort(ids), np.arange(n, dtype=ids.dtype)):
        return "ids is not a permutation of the spheres"
    rec = np.concatenate([spheres["center"], spheres["radius"][:, None]], axis=1).astype(np.float32)
    bad = np.flatnonzero((np.ascontiguousarray(leaf, np.float32).view(np.uint32) != np.ascontiguousarray(rec[ids]).view(np.uint32)).any(1))
    if len(bad):
        return f"leaf record {int(bad[0])} is not the bytes of sphere {int(ids[bad[0]])}"
    # ---- structure
    ref = nodes["ref"]
    is_leaf = lambda r: int(r) != NONE and bool(int(r) & LEAF)
    kids = lambda i: [r for r in ref[i] if int(r) != NONE]
    order, why = _walk(int(root), len(nodes), kids, is_leaf)
    if order is None:
        return why
    refs = [(int(root), "the root")] if is_leaf(root) else [(int(r), f"node {i}") for i in order for r in ref[i] if is_leaf(r)]
    leaves = []
    for r, where in refs:
        count, first = ((r >> 27) & 0xF) + 1, r & 0x07FFFFFF
        if not 1 <= count <= SPH_LEAF:
            return f"leaf {r:#x} of {where} holds {count} spheres"
        leaves.append((first, count, where))
    why = _tiling(leaves, n, "sphere tree")
    if why:
        return why
    # ---- per subtree, bottom-up: c -+ r as f32 computes them, the centres' bounds, node levels below
    c, rad = rec[ids][:, :3], rec[ids][:, 3:4]
    lo32, hi32 = (c - rad).astype(np.float64), (c + rad).astype(np.float64)   # f32 arithmetic, then exact in f64
    c64 = c.astype(np.float64)

    def leaf_stat(r):
        first, count = r & 0x07FFFFFF, ((r >> 27) & 0xF) + 1
        sl = slice(first, first + count)
        return lo32[sl].min(0), hi32[sl].max(0), c64[sl].min(0), c64[sl].max(0), 0

    def merge(a, b):
        return np.minimum(a[0], b[0]), np.maximum(a[1], b[1]), np.minimum(a[2], b[2]), np.maximum(a[3], b[3]), max(a[4], b[4])

    stat = {}
    box = [(nodes["cx"], nodes["hx"]), (nodes["cy"], nodes["hy"]), (nodes["cz"], nodes["hz"])]
    for i in reversed(order):
        ch = [None] * 4
        for k in range(4):
            r = int(ref[i][k])
            if r == NONE:
                continue
            st = leaf_stat(r) if is_leaf(r) else stat.pop(r)
            ch[k] = st
            for a in range(3):
                cc, hh = float(box[a][0][i][k]), float(box[a][1][i][k])
                lo, hi = float(st[0][a]), float(st[1][a])
                if not (cc - hh <= lo and cc + hh >= hi):
                    return f"node {i} child {k} axis {a}: box {cc!r} -+ {hh!r} does not contain [{lo!r}, {hi!r}] of the spheres below"
                if not hh <= (hi - lo) / 2 * (1 + 1e-6) + 2 * ulp32(max(abs(lo), abs(hi))) + 1e-37:
                    return f"node {i} child {k} axis {a}: half extent {hh!r} is loose for [{lo!r}, {hi!r}]"
                # both builders hand the exact min / max to set_box: its very words, which also tells a bound moved by one ulp
                m, h = set_box(lo, hi)
                if not (cc == float(m) and hh == float(h)):
                    return f"node {i} child {k} axis {a}: box {cc!r} -+ {hh!r} is not set_box's {float(m)!r} -+ {float(h)!r} for [{lo!r}, {hi!r}]"
        if ch[0] is None or ch[2] is None:
            return f"node {i}: a half of the split has no child 0 / 2"
        halves = [merge(ch[0], ch[1]) if ch[1] is not None else ch[0], merge(ch[2], ch[3]) if ch[3] is not None else ch[2]]
        whole = merge(halves[0], halves[1])
        axes = int(nodes["axes"][i])
        splits = [("the node", axes & 3, whole, halves[0], halves[1])]
        for h in range(2):
            if ch[2 * h + 1] is not None:
                splits.append((f"half {h}", (axes >> (2 + 2 * h)) & 3, halves[h], ch[2 * h], ch[2 * h + 1]))
        for what, a, both, low, high in splits:
            if a > 2:
                return f"node {i}: axes {axes:#x} names axis 3 for {what}"
            if axis_rule and a != longest_axis(both[2], both[3]):
                return f"node {i}: axes {axes:#x} names axis {a} for {what}, the longest axis of its centres is {longest_axis(both[2], both[3])}"
            if not low[3][a] <= high[2][a]:
                return f"node {i}: split order of {what} along axis {a}: {low[3][a]!r} below, {high[2][a]!r} above"
        stat[i] = whole[:4] + (1 + whole[4],)
    levels = 0 if is_leaf(root) else stat[int(root)][4]
    if depth != 3 * levels or depth > 32:
        return f"depth {depth} is not 3 x {levels} levels of nodes (or beyond the 32 stack entries)"
    return None
