"""Hemisphere rays made on the device next to the same rays given by the caller, and the two bakers end to end (DESIGN.md
section 16.7):

    python tools/hemisphere_rate.py [--configs c2,c3,lamp,c4] [--runs 5] [--samples 16] [--surfels 1048576]
                                    [--width 1920 --height 1080] [--child-timeout 300] [--out profiles/r16_hemisphere_rate.txt]

One process per configuration.  In it the scene at --width x --height, `surfels` surfels spread evenly over the first hits of
its pixel centres (Engine.render_hits; the normal turned towards the camera), and two ways to the same paths:

    hemisphere  rb_trace_hemisphere_device, `samples` samples per surfel: k_hemi_rays into the record scratch, the k_cam kernel,
                k_rad_sum
    rays        rb_trace_rays_device with samples = 1 on the n x `samples` records of those surfels, made beforehand by
                rb_hemisphere_rays and uploaded: the same rays; that entry point hashes an id into its seed, so the paths
                continue with other random numbers -- the same first segments, statistically the same work after them

Kernel ms from rb_last_query_ms -- for the hemisphere form that is generator, trace and sum together --, and the generator's
share from rb_last_camera_rays_ms; one warm-up pair, then `runs` alternating pairs, median and spread (max - min).  The
requirement: the hemisphere form's median is at most the ray form's median plus the larger of the two spreads plus the
generator's median.  The exit status says whether it held for every configuration.

Then, in the same process, wall time end to end (a host clock around calls that end in a synchronise; median and spread of
`wall_runs` calls after one warm-up call each, alternating): bake.irradiance against bake.irradiance_device on `wall_surfels`
of those points, and aov.ambient_occlusion against aov.ambient_occlusion_device on the whole frame's first hits.
"""
import argparse, os, sys, time
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from _rate import Report, alternating, child_argv, child_exit, child_header, med, med_text, run_children, scene_of

HEADER = (f"{'scene':6} {'surfels':>9} {'spp':>4}  {'hemi kernel':13} {'ms':>18}  {'generator ms':>18}  {'ray kernel':12} {'ms':>18}  "
          f"{'hemi/rays':>9}  held")


def wall(fns, runs):
    """seconds of each of `fns`, alternating, after one warm-up call each: [(median, spread), ...]"""
    def seconds(fn):
        t0 = time.perf_counter()
        fn()
        return time.perf_counter() - t0
    return [med(x) for x in alternating(fns, runs, seconds).values()]


def one(name, width, height, samples, runs, n, wall_surfels, wall_runs):
    """the lines of one configuration, and whether the requirement held"""
    import numpy as np
    import torch
    from renderbaby_amd import Engine, RenderConfig, aov, bake, engine

    def progress(what):   # (stderr: the parent passes it through)
        print(f"[{name}] {what}", file=sys.stderr, flush=True)
    s = scene_of(name).with_params(width=width, height=height, spp=1)
    rc = RenderConfig.from_scene(s)
    e = Engine.new(rc, device=0)
    e.update(rc)
    progress("scene uploaded")
    hits = e.render_hits()
    _, pts, nrm = aov.ambient_occlusion_surfels(s.uniforms, hits)
    if len(pts) == 0:
        raise SystemExit(f"{name}: no pixel centre hits anything")
    pick = (np.arange(n, dtype=np.int64) * len(pts)) // n   # evenly over the hits; fewer hits than surfels: some twice
    pts, nrm = np.ascontiguousarray(pts[pick]), np.ascontiguousarray(nrm[pick])
    dev = torch.device("cuda", 0)
    records = torch.empty((n * samples, 8), dtype=torch.float32, device=dev)
    step = max(1, (1 << 22) // samples)   # the generator's own piece at a time through host memory
    for i0 in range(0, n, step):
        sl = slice(i0, min(i0 + step, n))
        rays, _ = engine.hemisphere_rays_device(pts[sl], nrm[sl], samples, seeds=np.arange(sl.start, sl.stop, dtype=np.uint32), device=0)
        records[sl.start * samples:sl.stop * samples] = torch.from_numpy(rays.view(np.float32).reshape(-1, 8)).to(dev)
    tp, tn = torch.from_numpy(pts).to(dev), torch.from_numpy(nrm).to(dev)
    out_h = torch.empty((n, 4), dtype=torch.float32, device=dev)
    out_r = torch.empty((n * samples, 4), dtype=torch.float32, device=dev)
    progress("records made")

    def measure(which):   # (kernel ms, the generator's share, the kernel's name)
        if which == "hemi":
            e.trace_hemisphere(tp, tn, samples, out=out_h)
        else:
            e.trace_ray_records(records, samples=1, out=out_r)
        return e.last_query_ms(), e.last_camera_rays_ms(), e.last_query_kernel_name()
    got = alternating(("hemi", "rays"), runs, measure)
    hemi, gen, rays = [v[0] for v in got["hemi"]], [v[1] for v in got["hemi"]], [v[0] for v in got["rays"]]
    (mh, sh), mg, (mr, sr) = med(hemi), med(gen)[0], med(rays)
    ok = mh <= mr + max(sh, sr) + mg
    lines = [f"{name:6} {n:9d} {samples:4d}  {got['hemi'][-1][2]:13} {med_text(hemi)}  {med_text(gen)}  {got['rays'][-1][2]:12} {med_text(rays)}  "
             f"{mh / mr:9.3f}  {ok}"]
    del records, out_r
    progress("kernels timed")
    # end to end: the parent's host path against the device path, on the same points and on the same first hits
    wp, wn = pts[:wall_surfels], nrm[:wall_surfels]
    (bh, bhs), (bd, bds) = wall([lambda: bake.irradiance(e, wp, wn, samples), lambda: bake.irradiance_device(e, wp, wn, samples)], wall_runs)
    progress("bakers timed")
    (ah, ahs), (ad, ads) = wall([lambda: aov.ambient_occlusion(e, hits, n_dirs=samples, radius=1.0),
                                 lambda: aov.ambient_occlusion_device(e, hits, samples=samples, radius=1.0)], wall_runs)
    lines.append(f"#wall {name:6} bake.irradiance, {len(wp)} points x {samples}: host {bh:8.3f} ({bhs:6.3f}) s  device {bd:8.3f} ({bds:6.3f}) s  host / device {bh / bd:7.1f}")
    lines.append(f"#wall {name:6} AO image {width} x {height} x {samples}: host {ah:8.3f} ({ahs:6.3f}) s  device {ad:8.3f} ({ads:6.3f}) s  host / device {ah / ad:7.1f}")
    e.close()
    return lines, ok


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--configs", default="c2,c3,lamp,c4")
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--samples", type=int, default=16)
    ap.add_argument("--surfels", type=int, default=1 << 20)
    ap.add_argument("--width", type=int, default=1920)
    ap.add_argument("--height", type=int, default=1080)
    ap.add_argument("--wall-surfels", type=int, default=1 << 20)
    ap.add_argument("--wall-runs", type=int, default=3)
    ap.add_argument("--child-timeout", type=int, default=300, help="seconds one configuration's process may take")
    ap.add_argument("--out", default=None)
    ap.add_argument("--child", default=None, help=argparse.SUPPRESS)
    ap.add_argument("--header", action="store_true", help=argparse.SUPPRESS)
    a = ap.parse_args()
    if a.child:   # one configuration in this process: its lines, the verdict as the exit status
        if a.header:
            child_header()
        lines, ok = one(a.child, a.width, a.height, a.samples, a.runs, a.surfels, min(a.wall_surfels, a.surfels), a.wall_runs)
        print("\n".join(lines), flush=True)
        child_exit(ok)
    from renderbaby_amd._lib import source_fingerprint   # (this process never opens the device: the children do)
    with Report(a.out) as r:
        r.say(f"# library sources {source_fingerprint()}; {a.runs} alternating runs after one warm-up pair; kernel ms as median (max - min)")
        r.say("# hemi = rb_trace_hemisphere_device (generator + trace + sum, rb_last_query_ms; generator alone: rb_last_camera_rays_ms);")
        r.say("# rays = rb_trace_rays_device, samples = 1, on the surfels' n x spp records made by rb_hemisphere_rays; one process per scene")
        r.say(f"# #wall lines: end-to-end seconds of the host path and of the device path, median (max - min) of {a.wall_runs} alternating calls after a warm-up call")
        r.say(HEADER)
        options = ("runs", "samples", "surfels", "width", "height", "wall_surfels", "wall_runs")
        held, _ = run_children(r, lambda name, first: child_argv(__file__, name, a, options, first), a.configs.split(","), a.child_timeout)
        r.say(f"# hemisphere median <= ray median + max(spreads) + generator median for every scene: {held}")
    return 0 if held else 1


if __name__ == "__main__":
    sys.exit(main())
