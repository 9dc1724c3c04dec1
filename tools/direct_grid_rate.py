"""Direct light with the emitters picked per grid cell: what the tables cost to make, what the pick from
a table per cell costs beside the pick from one table, and how much noise it removes.  Nothing is judged; the yardstick is the
pick by power (section 23) in the same process.

    python tools/direct_grid_rate.py [--runs 5] [--samples 16] [--width 1920 --height 1080] [--child-timeout 300]
                                     [--out profiles/r36_direct_grid_rate.txt]

Timings, kernel ms as median (max - min) of `runs` calls after a warm-up call:

    build    rb_emitter_grid_cdf_device with the scene's kept emitter table (rb_last_query_ms: the powers, the bounds, one
             block per cell) for spheres_scene(n = 10^6) with two lights added (about 10^4 emitters) at 8^3 and 16^3 cells, and
             for C2's two emitters at 16^3
    direct   rb_direct_light_cdf_device with the scene's kept table (by power, the yardstick) against rb_direct_light_grid_device
             with tables built beforehand, on the same surfels and samples: all three stages (rb_last_query_ms) and the
             generator's share (rb_last_camera_rays_ms), on C2's first hits and on the ground hits of that sphere scene

Noise, by direct_light_rate.py's method with occlusion included: one surfel per sample so that the per-sample values come back;
per point the variance of the mean of the three channels under the uniform pick, the pick by power and the pick per cell, on
ground points of spheres_scene(n = 100 000) -- at 8 x 1 x 8 cells, about 16 of its emitters to a cell, and at 32 x 1 x 32, about
one -- and on 8 floor points of the feature scene at 4 x 2 x 4.  One process per line group.
"""
import argparse, os, statistics, sys
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from _rate import Report, child_argv, child_exit, med_text, run_children, scene_of
from direct_pick_rate import OWN, engine_of, ground


def first_hits(name, e, s):
    from renderbaby_amd import aov
    _, pts, nrm = aov.ambient_occlusion_surfels(s.uniforms, e.render_hits())
    if name == "c4":
        keep = ground(pts, nrm)
        pts, nrm = pts[keep], nrm[keep]
    return pts, nrm


def build(name, width, height, runs):
    import torch
    from renderbaby_amd import bake
    s = scene_of(name, OWN).with_params(width=width, height=height, spp=1)
    e, _ = engine_of(s)
    tab = e.scene_emitters()
    lines = []
    for counts in ((8, 8, 8), (16, 16, 16)) if name == "c4" else ((16, 16, 16),):
        g = bake.pick_grid(tab, counts)
        rows = counts[0] * counts[1] * counts[2]
        out = torch.empty(rows * len(tab), dtype=torch.int32, device=torch.device("cuda", 0))
        ms = []
        for run in range(runs + 1):
            e.emitter_grid(g, out=out)
            if run:
                ms.append(e.last_query_ms())
        m = statistics.median(ms)
        lines.append(f"build    {name:7} {len(tab):6d} emitters x {counts[0]} x {counts[1]} x {counts[2]} cells = {rows * len(tab):9d} entries, "
                     f"{e.last_query_kernel_name()}: {med_text(ms)} ms  ({rows * len(tab) * 4 / m / 1e6:.1f} GB/s of rows written, "
                     f"{rows * len(tab) * 2 / m / 1e6:.1f} G weights/s)")
    e.close()
    return lines


def stages(name, width, height, samples, runs):
    import numpy as np
    import torch
    from renderbaby_amd import bake
    s = scene_of(name, OWN).with_params(width=width, height=height, spp=1)
    e, _ = engine_of(s)
    pts, nrm = first_hits(name, e, s)
    n = len(pts)
    dev = torch.device("cuda", 0)
    tp, tn = torch.from_numpy(np.ascontiguousarray(pts)).to(dev), torch.from_numpy(np.ascontiguousarray(nrm)).to(dev)
    tab = e.scene_emitters()
    counts = (16, 2, 16) if name == "c4" else (8, 8, 8)
    g = bake.pick_grid(tab, counts, points=pts)
    rows = counts[0] * counts[1] * counts[2]
    tables = e.emitter_grid(g, out=torch.empty(rows * len(tab), dtype=torch.int32, device=dev))   # built beforehand, kept by the caller
    out = torch.empty((n, 4), dtype=torch.float32, device=dev)
    ms = {k: [] for k in ("pow", "pow_gen", "grid", "grid_gen")}
    for run in range(runs + 1):
        e.direct_light(tp, tn, samples, out=out, pick="power")
        p, pg, kernel = e.last_query_ms(), e.last_camera_rays_ms(), e.last_query_kernel_name()
        e.direct_light(tp, tn, samples, out=out, pick=("grid", g, tables))
        q, qg = e.last_query_ms(), e.last_camera_rays_ms()
        if run:
            for k, v in zip(ms, (p, pg, q, qg)):
                ms[k].append(v)
    e.close()
    share = lambda gen, a: 100 * statistics.median(gen) / statistics.median(a)
    return [f"direct   {name:7} {n:8d} surfels x {samples:3d}, {len(tab)} emitters, {counts[0]} x {counts[1]} x {counts[2]} cells, {kernel}:",
            f"         by power all {med_text(ms['pow'])} ms  generator {med_text(ms['pow_gen'])}  ({share(ms['pow_gen'], ms['pow']):.1f} % of the call)",
            f"         per cell all {med_text(ms['grid'])} ms  generator {med_text(ms['grid_gen'])}  ({share(ms['grid_gen'], ms['grid']):.1f} % of the call); "
            f"generator x {statistics.median(ms['grid_gen']) / statistics.median(ms['pow_gen']):.2f}, call x {statistics.median(ms['grid']) / statistics.median(ms['pow']):.3f}"]


def noise(name, points, samples):
    import numpy as np
    from renderbaby_amd import aov, bake, direct
    s = scene_of(name, OWN)
    if name == "feature":
        pts = np.array([(x, -1.0, z) for x in (-1.5, 0.5) for z in (-3.0, -2.0, -1.0, 0.0)], np.float32)
        nrm = np.tile(np.float32([0, 1, 0]), (len(pts), 1))
        grids = ((4, 2, 4),)
        e, _ = engine_of(s)
    else:
        s = s.with_params(width=96, height=54, spp=1)
        grids = ((8, 1, 8), (32, 1, 32))   # about 16 emitters to a cell, and about one
        e, _ = engine_of(s)
        _, p0, n0 = aov.ambient_occlusion_surfels(s.uniforms, e.render_hits())
        idx = np.nonzero(ground(p0, n0))[0]
        idx = idx[(np.arange(min(points, len(idx))) * len(idx)) // min(points, len(idx))]
        pts, nrm = p0[idx], n0[idx]
    tab = e.scene_emitters()
    power = direct.emitter_weights(tab)
    p, nn = np.repeat(pts, samples, axis=0), np.repeat(nrm, samples, axis=0)
    per = lambda pick: e.direct_light(p, nn, 1, pick=pick)["sum"].astype(np.float64).mean(1).reshape(len(pts), samples)
    uni, pw = per("uniform"), per("power")
    vu, vp = uni.var(1, ddof=1), pw.var(1, ddof=1)
    lines = [f"noise    {name:7} {len(pts):3d} points x {samples} samples, {len(power)} emitters of power {power.min():.3g} .. {power.max():.3g}: "
             f"means uniform {uni.mean():.5f}, by power {pw.mean():.5f}"]
    for counts in grids:
        g = bake.pick_grid(tab, counts, points=pts)
        gr = per(("grid", g, e.emitter_grid(g)))
        vg = gr.var(1, ddof=1)
        ok = (vu > 0) & (vp > 0) & (vg > 0)
        se = np.hypot(pw.std(ddof=1), gr.std(ddof=1)) / np.sqrt(gr.size)
        lines += [f"         {counts[0]} x {counts[1]} x {counts[2]} cells: mean {gr.mean():.5f} ({abs(pw.mean() - gr.mean()) / se:.2f} combined standard errors from the pick by power's), "
                  f"{int(ok.sum())} points with light",
                  "           per-point variance uniform / per cell: " + " ".join(f"{r:.2f}" for r in vu[ok] / vg[ok]) + f"; pooled {vu.mean() / vg.mean():.2f}",
                  "           per-point variance by power / per cell: " + " ".join(f"{r:.2f}" for r in vp[ok] / vg[ok]) + f"; pooled {vp.mean() / vg.mean():.2f}"]
    e.close()
    return lines


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--samples", type=int, default=16)
    ap.add_argument("--width", type=int, default=1920)
    ap.add_argument("--height", type=int, default=1080)
    ap.add_argument("--child-timeout", type=int, default=300, help="seconds one child process may take")
    ap.add_argument("--out", default=None)
    ap.add_argument("--child", default=None, help=argparse.SUPPRESS)
    a = ap.parse_args()
    if a.child:
        kind, name = a.child.split(":")
        lines = (build(name, a.width, a.height, a.runs) if kind == "build" else stages(name, a.width, a.height, a.samples, a.runs) if kind == "stages"
                 else noise(name, 6, 65536) if name == "c4like" else noise(name, 8, 4096))
        print("\n".join(lines), flush=True)
        child_exit()
    from renderbaby_amd._lib import source_fingerprint   # (this process never opens the device: the children do)
    with Report(a.out) as r:
        r.say(f"# library sources {source_fingerprint()}; kernel ms as median (max - min) of {a.runs} calls after a warm-up call; one process per line group")
        r.say("# build: rb_emitter_grid_cdf_device with the scene's kept emitter table; direct: rb_direct_light_cdf_device with the scene's kept table (by")
        r.say("# power, the yardstick) and rb_direct_light_grid_device with tables built beforehand, on the same surfels and samples")
        r.say("# noise: one surfel per sample, occlusion included; variance of the per-sample mean of the three channels under each pick, per point")
        ok, _ = run_children(r, lambda name, first: child_argv(__file__, name, a, ("runs", "samples", "width", "height")),
                             ("build:c4", "build:c2", "stages:c2", "stages:c4", "noise:c4like", "noise:feature"), a.child_timeout)
    return 0 if ok else 1


if __name__ == "__main__":
    sys.exit(main())
