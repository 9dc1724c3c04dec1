"""numpy model of the triangle sift of the single-node kernels ("The triangle sift"): the group records and
the origin region as renderbaby_amd/csrc/rb_tri_filter.hpp makes them (double arithmetic, every stored value rounded to the
safe side), and pass 1 as sift_triangles (rb_device_intersect.hpp) evaluates it, one float32 operation per kernel instruction
(a fused multiply-add is modelled in float64 and rounded once; the approximate reciprocal as the correctly rounded 1 / x, which
v_rcp_f32 is within one ulp of -- the records carry that slack).  The model is not the kernel bit for bit; it is the same rule.

Everything is vectorised over `n` independent cases: a group is a dict of float32 arrays [n] (c, h, nrm as [3][n]), so that a
stress test can give every ray a group and a region of its own, and a scene's table is the same dicts with n = 1 per group."""
import numpy as np

F32 = np.float32
U = 2.0 ** -24
C0 = 0.03                      # kFastGrazeCos
FMAX = F32(1.5e5)              # kChunkFMax
KS, KP, KT, KD = (F32(24.0) * F32(5.9604645e-8) * F32(1.01), F32(12.0) * F32(5.9604645e-8) * F32(1.01),
                  F32(11.0) * F32(5.9604645e-8) * F32(1.01), F32(16.0) * F32(5.9604645e-8) * F32(1.01))
SLAB_ULPS = 8.0                # kSiftSlabUlps
EDGE_MAX, SP_MAX = 1e9, 1e12   # kSiftEdgeMax, kSiftSpMax
GROUP_MAX, ALPHA_MAX, BOX_GROW, MIN_LIVE, MAX_SLOTS = 4, 1e-3, 1.05, 4, 128
INF = F32(np.inf)


def f32_not_below(v, floor):
    """v >= floor >= 0 (float64 arrays) as float32 that is not below `floor`"""
    v, floor = np.asarray(v, np.float64), np.asarray(floor, np.float64)
    with np.errstate(over="ignore"):
        f = v.astype(F32)
    up = np.nextafter(f, INF)
    return np.where(f.astype(np.float64) < floor, up, f).astype(F32)


def _fma(a, b, c):
    with np.errstate(invalid="ignore", over="ignore"):
        return (np.asarray(a, np.float64) * np.asarray(b, np.float64) + np.asarray(c, np.float64)).astype(F32)


# ------------------------------------------------------------------------------------- records ---
def make_group(v0, e1, e2):
    """One group per case from its m member triangles: v0, e1, e2 float32 [m][3][n] (the prepared records' f32 edges).
    -> dict(c [3][n], h [3][n], nrm [3][n], fk, cap, s [n], closed bool [n]); where `closed` is False the members may not form a
    group that rejects (rb_tri_filter.hpp close_group) and the record is the always-pass one."""
    v0, e1, e2 = (np.asarray(a, F32) for a in (v0, e1, e2))
    m, _, n = v0.shape
    d0, d1, d2 = v0.astype(np.float64), e1.astype(np.float64), e2.astype(np.float64)
    finite = np.isfinite(d0).all((0, 1)) & np.isfinite(d1).all((0, 1)) & np.isfinite(d2).all((0, 1))
    with np.errstate(all="ignore"):
        l1, l2 = (d1 * d1).sum(1), (d2 * d2).sum(1)                       # [m][n]
        nx = np.stack([d1[:, 1] * d2[:, 2] - d1[:, 2] * d2[:, 1], d1[:, 2] * d2[:, 0] - d1[:, 0] * d2[:, 2],
                       d1[:, 0] * d2[:, 1] - d1[:, 1] * d2[:, 0]], 1)     # [m][3][n]
        nn = np.sqrt((nx * nx).sum(1))
        ll = np.maximum(l1, l2)
        has_normal = (nn > 0.0) & np.isfinite(nn)
        unit = nx / np.where(has_normal, nn, 1.0)[:, None]
        graze = ll / nn / (0.95 * float(F32(C0)))
        bf = np.where(ll * 1e6 * (1.0 + 1e-5) <= 0.0, 0.0, f32_not_below(graze * (1.0 + 1e-5), graze * (1.0 + 1e-6)).astype(np.float64))
        g = np.sqrt(l1) * np.sqrt(l2) * (1.0 + 1e-12)
        cap = g * 1e6 * (1.0 + 1e-5)
        fa = np.where(ll > 0.0, bf * (g / np.where(ll > 0.0, ll, 1.0)) * (1.0 + 1e-9), bf)
        cap_l, fa_l = ll * 1e6 * (1.0 + 1e-5), bf
        ok = finite & (has_normal & np.isfinite(fa_l) & np.isfinite(fa) & (fa_l > 0.0)).all(0)
        # boxes
        p1, p2 = d0 + d1, d0 + d2
        tlo, thi = np.minimum(d0, np.minimum(p1, p2)), np.maximum(d0, np.maximum(p1, p2))     # [m][3][n]
        lo, hi = tlo.min(0), thi.max(0)
        largest = (thi - tlo).sum(1).max(0)
        if m > 1:
            ok &= (hi - lo).sum(0) <= BOX_GROW * largest
        # cone: the normalised sum of the sign-aligned normals
        sg = np.where((unit * unit[0:1]).sum(1) < 0.0, -1.0, 1.0)        # [m][n]
        axis = (unit * sg[:, None]).sum(0)
        ln = np.sqrt((axis * axis).sum(0))
        ok &= ln > 1e-9
        axis = axis / np.where(ln > 1e-9, ln, 1.0)
        cmin = np.minimum(1.0, np.abs((unit * axis[None]).sum(1)).min(0))
        alpha = np.arccos(cmin) + 1e-9
        ok &= alpha <= ALPHA_MAX
        ok &= cap_l.max(0) <= EDGE_MAX * EDGE_MAX * 1e6 * (1.0 + 1e-5)
        beyond = ~(cap_l.max(0) * (1.0 + 1e-6) <= 1.5e5)
        capv = np.where(beyond, np.inf, cap.max(0) * (1.0 + 1e-6))
        fav = np.where(beyond, fa_l.max(0), fa.max(0))
        fk = fav * float(F32(C0)) * 1.00001 * (1.0 + 2e-6)
        ok &= fk <= 1.5e5
        mid = 0.5 * (lo + hi)
        c = mid.astype(F32)
        half = np.maximum(hi - c.astype(np.float64), c.astype(np.float64) - lo)
        h = f32_not_below(half * (1.0 + 1e-6) + 1e-12 * np.abs(mid) + 1e-37, half)
        ok &= np.isfinite(c).all(0) & np.isfinite(h).all(0)
        cos_a = np.cos(alpha) * (1.0 - 1e-6) - 1e-7
        sin_a = np.sin(alpha) * (1.0 + 1e-5) + 2e-6
        grp = dict(c=np.where(ok, c, F32(0)), h=np.where(ok, h, F32(0)), nrm=np.where(ok, (axis * cos_a).astype(F32), F32(0)),
                   fk=np.where(ok, f32_not_below(fk, fk), INF), cap=np.where(ok, np.where(np.isfinite(capv), f32_not_below(capv, capv), INF), INF),
                   s=np.where(ok, f32_not_below(sin_a, sin_a), F32(0)), closed=ok)
    return grp


def make_region(grp, extra_lo, extra_hi):
    """The origin region and the folded constants of cases whose table is the one closed group `grp` each (float64 [3][n] boxes
    `extra`: the camera, the spheres -- here whatever the case's ray starts from) -> dict(lo, hi [3][n], kp, ks, kt, kd [n])"""
    c, h = grp["c"], grp["h"]
    tlo = np.nextafter((c - h).astype(F32), -INF).astype(np.float64)
    thi = np.nextafter((c + h).astype(F32), INF).astype(np.float64)
    lhalf = 0.5 * (2.0 * h.astype(np.float64)).sum(0)
    return region_of(tlo, thi, lhalf, extra_lo, extra_hi)


def region_of(tlo, thi, lhalf, extra_lo, extra_hi):
    lo, hi = np.minimum(tlo, extra_lo), np.maximum(thi, extra_hi)
    m = np.maximum(np.abs(lo), np.abs(hi)).max(0)
    pad = 1e-3 * np.maximum(m, (hi - lo).max(0)) + 1e-30
    rlo = np.nextafter((lo - pad).astype(F32), -INF)
    rhi = np.nextafter((hi + pad).astype(F32), INF)
    ext = rhi.astype(np.float64) - rlo.astype(np.float64)
    m = np.maximum(m, np.maximum(np.abs(rlo), np.abs(rhi)).max(0).astype(np.float64))
    sp = 1.001 * (np.sqrt((ext * ext).sum(0)) + lhalf)
    k = lambda v: f32_not_below(v * (1.0 + 1e-6), v * (1.0 + 1e-6))
    kp, ks = sp * float(KP) * (1.0 + 1e-6), (sp * float(KS) + SLAB_ULPS * U * (m + sp)) * (1.0 + 1e-6)
    # the reciprocal up to which no product of the slab values overflows: |c|, |o| <= M, h <= Sp, mm <= kp FMax + ks
    reach = 2.0 * m + sp + (kp * 1.5e5 + ks)
    with np.errstate(over="ignore"):
        rmax = (1e38 / reach).astype(F32)
        rmax = np.where(rmax.astype(np.float64) * reach > 1e38, np.nextafter(rmax, F32(0)), rmax).astype(F32)
    return dict(on=(sp <= SP_MAX) & np.isfinite(rmax) & (rmax > 0), lo=rlo, hi=rhi, kp=k(sp * float(KP)), ks=k(sp * float(KS) + SLAB_ULPS * U * (m + sp)),
                kt=k(sp * float(KT)), kd=k(sp * float(KD)), rmax=rmax)


# -------------------------------------------------------------------------------------- pass 1 ---
def pass1(grp, reg, o, d, detail=False):
    """sift_triangles' pass 1: o, d float32 [3][n] -> keep bool [n] (True: the group's slots are candidates)"""
    o, d = [np.asarray(x, F32) for x in o], [np.asarray(x, F32) for x in d]
    with np.errstate(all="ignore"):
        inv = [F32(1.0) / d[i] for i in range(3)]
        oi = [o[i] * inv[i] for i in range(3)]
        inside = np.ones(o[0].shape, bool)
        for i in range(3):
            inside &= (o[i] > reg["lo"][i]) & (o[i] < reg["hi"][i]) & (np.abs(inv[i]) <= reg["rmax"])   # (a NaN fails every compare)
        nrm, c, h = grp["nrm"], grp["c"], grp["h"]
        y = _fma(d[2], nrm[2], _fma(d[1], nrm[1], d[0] * nrm[0]))
        lb = np.abs(y) - grp["s"]
        fl = grp["fk"] * (F32(1.0) / lb)
        f = np.where((lb > F32(1e-6)) & (fl < grp["cap"]), fl, grp["cap"]).astype(F32)
        mm = _fma(reg["kp"], f, reg["ks"])
        thr = F32(0.001) - _fma(reg["kt"], f, reg["kd"])
        tn, tf = None, None
        for i in range(3):
            tc = _fma(c[i], inv[i], -oi[i])
            hm = h[i] + mm
            a, b = _fma(-hm, np.abs(inv[i]), tc), _fma(hm, np.abs(inv[i]), tc)
            tn = a if tn is None else np.fmax(tn, a)       # v_max3_f32 / v_min3_f32 drop a NaN operand
            tf = b if tf is None else np.fmin(tf, b)
        keep = (~(tf < tn) & ~(tf < thr)) | ~(f <= FMAX) | ~inside | ~reg["on"]   # (a launch whose region is off does not sift at all)
    if detail:
        return keep, dict(tn=tn, tf=tf, thr=thr, f=f, inside=inside)
    return keep


# ------------------------------------------------------------------------------ a node's table ---
def build_table(v0, e1, e2, valid):
    """The groups of a node's list (rb_tri_filter.hpp build_sift_table): v0, e1, e2 float32 [n][3] in slot order, valid [n].
    -> (groups: list of (first, count, record of n = 1), live, closed)"""
    v0, e1, e2 = (np.asarray(a, F32) for a in (v0, e1, e2))
    n = len(v0)
    assert n <= MAX_SLOTS
    rec = lambda a, b: make_group(v0[a:b].reshape(b - a, 3, 1), e1[a:b].reshape(b - a, 3, 1), e2[a:b].reshape(b - a, 3, 1))
    single = [rec(i, i + 1) if valid[i] else None for i in range(n)]
    is_closed = [g is not None and bool(g["closed"][0]) for g in single]
    groups, a = [], 0
    while a < n:
        block_end = min(n, (a // 32 + 1) * 32)
        b = a + 1
        if is_closed[a]:
            g = single[a]
            while b < block_end and b - a < GROUP_MAX and is_closed[b]:
                wider = rec(a, b + 1)
                if not wider["closed"][0]:
                    break
                g, b = wider, b + 1
        else:
            g = make_group(np.full((1, 3, 1), np.nan, F32), np.zeros((1, 3, 1), F32), np.zeros((1, 3, 1), F32))   # always pass
            while b < block_end and b - a < GROUP_MAX and not is_closed[b]:
                b += 1
        groups.append((a, b - a, g))
        a = b
    return groups, int(np.count_nonzero(valid)), sum(1 for g in groups if g[2]["closed"][0])


def table_region(groups, extra_lo, extra_hi):
    """the region of a launch over `groups` (sift_region): extra boxes as float64 [3] lo / hi (union of the camera and the spheres)"""
    closed = [g for _, _, g in groups if g["closed"][0]]
    tlo = np.min([np.nextafter((g["c"] - g["h"]).astype(F32), -INF) for g in closed], 0).astype(np.float64)
    thi = np.max([np.nextafter((g["c"] + g["h"]).astype(F32), INF) for g in closed], 0).astype(np.float64)
    lhalf = max(0.5 * float((2.0 * g["h"].astype(np.float64)).sum()) for g in closed)
    return region_of(tlo, thi, lhalf, np.asarray(extra_lo, np.float64).reshape(3, 1), np.asarray(extra_hi, np.float64).reshape(3, 1))


def candidate_mask(groups, reg, o, d):
    """bool [slots][rays]: each ray's candidate slots, as sift_triangles leaves them after pass 1"""
    o, d = np.asarray(o, F32), np.asarray(d, F32)
    n = sum(c for _, c, _ in groups)
    out = np.zeros((n, o.shape[1]), bool)
    for first, count, g in groups:
        out[first:first + count] = pass1(g, reg, o, d)[None]
    return out
