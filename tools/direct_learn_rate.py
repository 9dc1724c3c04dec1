"""Per-cell emitter tables that learn visibility: what the count costs a call, what the learned build
costs beside section 24's, and how much noise the learned tables remove.  Nothing is judged; section 24.5's method, scenes and
yardstick (the pick by power in the same process).

    python tools/direct_learn_rate.py [--runs 5] [--samples 16] [--width 1920 --height 1080] [--child-timeout 300]
                                      [--out profiles/r37_direct_learn_rate.txt]

Timings, kernel ms as median (max - min) of `runs` calls after a warm-up call:

    build    rb_emitter_grid_cdf_device (k_grid_rows) against rb_emitter_grid_learned_device (k_grid_rows_seen) with a tally of
             one training call, the scene's kept emitter table, spheres_scene(n = 10^6) with two lights added at 8^3 and 16^3 cells
    direct   rb_direct_light_grid_device against rb_direct_light_grid_tally_device with and without sums, tables built beforehand,
             the same surfels and samples (rb_last_query_ms: the generator, the walk, the count, the fold).  The count's kernel
             time is the tallied call less the plain one, k_direct_fold's the tallied call less the training-only one.  Both
             forms of the count: the one that is launched, which adds once per wave and distinct record (k_grid_tally), and
             one add per item (k_grid_tally_plain, RB_GRID_TALLY=plain), in alternating order.
             `records hit`: how many of the tally's records the call added to, and the largest share of one record -- what the
             atomics' addresses look like.

Noise, by direct_grid_rate.py's method with occlusion included, the same points: per point the variance under the pick by power
over that under section 24's tables and under the learned tables after 1 and 2 rounds of `--learn-samples` training samples per
training surfel -- every ground hit of the frame, or a 24 x 24 lattice on the feature scene's floor --, samples that lie
behind the rendered ones.  One process per line group.
"""
import argparse, os, statistics, sys
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from _rate import Report, alternating, child_argv, child_exit, env, med_text, run_children, scene_of
from direct_grid_rate import first_hits
from direct_pick_rate import OWN, engine_of, ground


def build(name, width, height, samples, runs):
    import numpy as np
    import torch
    from renderbaby_amd import bake
    s = scene_of(name, OWN).with_params(width=width, height=height, spp=1)
    e, _ = engine_of(s)
    pts, nrm = first_hits(name, e, s)
    dev = torch.device("cuda", 0)
    tp, tn = torch.from_numpy(np.ascontiguousarray(pts)).to(dev), torch.from_numpy(np.ascontiguousarray(nrm)).to(dev)
    tab = e.scene_emitters()
    lines = []
    for counts in ((8, 8, 8), (16, 16, 16)):
        g = bake.pick_grid(tab, counts, points=pts)
        rows = counts[0] * counts[1] * counts[2]
        out = torch.empty(rows * len(tab), dtype=torch.int32, device=dev)
        kept = torch.zeros((rows * len(tab), 2), dtype=torch.int32, device=dev)
        e.emitter_grid(g, out=out)
        e.direct_light(tp, tn, samples, first_sample=1 << 20, pick=("grid", g, out), tally=kept, out=False)
        ms = {"k_grid_rows": [], "k_grid_rows_seen": []}
        for run in range(runs + 1):
            for which in ms:
                e.emitter_grid(g, out=out, **(dict(tally=kept, prior=1.0) if which.endswith("seen") else {}))
                assert e.last_query_kernel_name() == which
                if run:
                    ms[which].append(e.last_query_ms())
        a, b = (statistics.median(v) for v in ms.values())
        lines.append(f"build    {name:7} {len(tab):6d} emitters x {counts[0]} x {counts[1]} x {counts[2]} cells = {rows * len(tab):9d} entries: "
                     f"k_grid_rows {med_text(ms['k_grid_rows'])} ms, k_grid_rows_seen {med_text(ms['k_grid_rows_seen'])} ms, x {b / a:.2f} "
                     f"({rows * len(tab) * 2 * 8 / b / 1e6:.1f} GB/s of tally read over both sweeps)")
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
    tables = e.emitter_grid(g, out=torch.empty(rows * len(tab), dtype=torch.int32, device=dev))
    out = torch.empty((n, 4), dtype=torch.float32, device=dev)
    arms = {"no count": ("combined", {}), "combined": ("combined", dict(tally=True)), "per item": ("plain", dict(tally=True)),
            "combined, no sums": ("combined", dict(tally=True, out=False))}
    kept = torch.zeros((rows * len(tab), 2), dtype=torch.int32, device=dev)
    tallies = {}

    def measure(arm):
        form, kw = arms[arm]
        kw = dict(kw)
        if kw.pop("tally", False):
            kept.zero_()
            kw["tally"] = kept
        kw.setdefault("out", out)
        with env("RB_GRID_TALLY", form):
            e.direct_light(tp, tn, samples, pick=("grid", g, tables), **kw)
        if "tally" in kw:
            tallies[arm] = kept.cpu().numpy().copy()
        return e.last_query_ms()
    ms = alternating(arms, runs, measure)
    kernel = e.last_query_kernel_name()
    e.close()
    assert (tallies["combined"] == tallies["per item"]).all() and (tallies["combined"] == tallies["combined, no sums"]).all()
    head = f"direct   {name:7} {n:8d} surfels x {samples:3d}, {len(tab)} emitters, {counts[0]} x {counts[1]} x {counts[2]} cells, {kernel}"
    tried = tallies["combined"][:, 0].view(np.uint32).astype(np.int64)
    p, c, i, tr = (statistics.median(ms[k]) for k in arms)
    return [f"{head}:",
            f"         rb_direct_light_grid_device {med_text(ms['no count'])} ms",
            f"         _tally_device, one add per wave and record {med_text(ms['combined'])} ms; without sums {med_text(ms['combined, no sums'])} ms; "
            f"one add per item {med_text(ms['per item'])} ms",
            f"         k_grid_tally {c - p:7.3f} ms ({100 * (c - p) / p:.1f} % of the call without a count), call x {c / p:.3f}; "
            f"k_grid_tally_plain {i - p:7.3f} ms, call x {i / p:.3f}; k_direct_fold {c - tr:7.3f} ms",
            f"         records hit {int((tried > 0).sum())} of {len(tried)}, {int(tried.sum())} shadow rays, the busiest record {100 * tried.max() / max(tried.sum(), 1):.1f} % of them; "
            "both forms leave the same tally"]


def noise(name, points, samples, learn_samples):
    import numpy as np
    from renderbaby_amd import aov, bake, direct, hemisphere
    s = scene_of(name, OWN)
    if name == "feature":
        pts = np.array([(x, -1.0, z) for x in (-1.5, 0.5) for z in (-3.0, -2.0, -1.0, 0.0)], np.float32)
        nrm = np.tile(np.float32([0, 1, 0]), (len(pts), 1))
        grids = ((4, 2, 4),)
        e, _ = engine_of(s)
        t_pts = np.array([(x, -1.0, z) for x in np.linspace(-2.0, 1.0, 24) for z in np.linspace(-3.5, 0.5, 24)], np.float32)   # the floor about them
        t_nrm = np.tile(np.float32([0, 1, 0]), (len(t_pts), 1))
    else:
        s = s.with_params(width=96, height=54, spp=1)
        grids = ((8, 1, 8), (32, 1, 32))
        e, _ = engine_of(s)
        _, p0, n0 = aov.ambient_occlusion_surfels(s.uniforms, e.render_hits())
        idx = np.nonzero(ground(p0, n0))[0]
        idx = idx[(np.arange(min(points, len(idx))) * len(idx)) // min(points, len(idx))]
        pts, nrm = p0[idx], n0[idx]
        t_pts, t_nrm = p0[ground(p0, n0)], n0[ground(p0, n0)]   # every ground hit of the frame
    tab = e.scene_emitters()
    p, nn = np.repeat(pts, samples, axis=0), np.repeat(nrm, samples, axis=0)
    per = lambda pick: e.direct_light(p, nn, 1, pick=pick)["sum"].astype(np.float64).mean(1).reshape(len(pts), samples)
    pw = per("power")
    vp = pw.var(1, ddof=1)
    lines = [f"noise    {name:7} {len(pts):3d} points x {samples} samples, {len(tab)} emitters; training: {len(t_pts)} surfels x {learn_samples} samples a round, "
             f"from sample {1 << 20} on, prior 1; mean by power {pw.mean():.5f}"]
    surf = hemisphere.surfels(t_pts, t_nrm)
    for counts in grids:
        g = bake.pick_grid(tab, counts, points=np.concatenate([pts, t_pts]))
        cols = {"section 24": e.emitter_grid(g)}
        for rounds in (1, 2):
            cols[f"learned, {rounds} round{'s' * (rounds > 1)}"], kept = bake.learn_grid(e, g, surf, rounds, learn_samples, prior=1.0)
        lines.append(f"         {counts[0]} x {counts[1]} x {counts[2]} cells; after 2 rounds {int(kept['tried'].sum())} rays tried, {int(kept['seen'].sum())} seen")
        for label, tables in cols.items():
            gr = per(("grid", g, tables))
            vg = gr.var(1, ddof=1)
            ok = (vp > 0) & (vg > 0)
            se = np.hypot(pw.std(ddof=1), gr.std(ddof=1)) / np.sqrt(gr.size)
            lines.append(f"           {label:17}: mean {gr.mean():.5f} ({abs(pw.mean() - gr.mean()) / se:.2f} combined standard errors from the pick by power's); "
                         "per-point variance by power / this: " + " ".join(f"{r:.2f}" for r in vp[ok] / vg[ok]) + f"; pooled {vp.mean() / vg.mean():.2f}")
    e.close()
    return lines


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--samples", type=int, default=16)
    ap.add_argument("--learn-samples", type=int, default=64)
    ap.add_argument("--width", type=int, default=1920)
    ap.add_argument("--height", type=int, default=1080)
    ap.add_argument("--child-timeout", type=int, default=300, help="seconds one child process may take")
    ap.add_argument("--out", default=None)
    ap.add_argument("--child", default=None, help=argparse.SUPPRESS)
    a = ap.parse_args()
    if a.child:
        kind, name = a.child.split(":")
        lines = (build(name, a.width, a.height, a.samples, a.runs) if kind == "build"
                 else stages(name, a.width, a.height, a.samples, a.runs) if kind == "stages"
                 else noise(name, 6, 65536, a.learn_samples) if name == "c4like" else noise(name, 8, 4096, a.learn_samples))
        print("\n".join(lines), flush=True)
        child_exit()
    from renderbaby_amd._lib import source_fingerprint   # (this process never opens the device: the children do)
    names = ("build:c4", "stages:c2", "stages:c4", "noise:c4like", "noise:feature")
    with Report(a.out) as r:
        r.say(f"# library sources {source_fingerprint()}; kernel ms as median (max - min) of {a.runs} calls after a warm-up call; one process per line group")
        r.say("# build: the scene's kept emitter table, a tally of one training call; direct: tables built beforehand, the same surfels and samples")
        r.say("# noise: one surfel per sample, occlusion included; variance of the per-sample mean of the three channels under each pick, per point")
        ok, _ = run_children(r, lambda name, first: child_argv(__file__, name, a, ("runs", "samples", "learn_samples", "width", "height")),
                             names, a.child_timeout)
    return 0 if ok else 1


if __name__ == "__main__":
    sys.exit(main())
