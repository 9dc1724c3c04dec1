"""Radiance along given rays next to the render of the same paths:

    python tools/radiance_rate.py [--configs c3,lamp,c5,c4,c2] [--runs 5] [--samples 16] [--scene-timeout 300] [--out FILE]

One process per scene (this one starts them in turn).  In each, at the scene's BASELINE frame size with one sample per pass:
a warm-up pair, then `runs` alternating pairs of

    render   rb_dispatch(e, 0, samples): the render kernels and k_accumulate; ms = rb_last_dispatch_ms (HIP events around all
             launches of the group)
    query    rb_trace_rays_device on the frame's pixel-centre rays in device memory, `samples` samples each; ms =
             rb_last_query_ms (HIP events around all launches: the k_rad kernels and k_rad_sum)

The two trace the same number of paths, width x height x samples, through the same per-path code; the paths themselves differ
(the render jitters its primary rays inside the pixel and seeds by pixel index in shader order, the query starts every sample
at the pixel centre and seeds by ray index), so the work is the same statistically, not path by path.  Reported: median and
spread (max - min) of each.  The requirement, for the scenes whose per-path code is the render's own (c3, lamp, c5, c4): the
query's median is not above the render's by more than the larger of the two spreads plus the time of reading the 32-byte rays,
n x 32 B at the HBM rate a device copy of the ray buffer achieves in the same process (a ray's later samples find it in cache).  c2 is recorded, not judged
(k_rad starts every path on its own lane; the render's k_trace stages its row starts, profiles/r10_c2_bench_ab.txt).
Whole-call times of the host form, and on c3 of bake.irradiance on 2^20 points x 16, are recorded beside these.
The exit status says whether the requirement held on every judged scene.
"""
import argparse, os, sys, time
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from _rate import Report, alternating, child_exit, med, med_text, run_children, scene_of
JUDGED = ("c3", "lamp", "c5", "c4")


def one(name, runs, samples, whole):
    """the measurements of one scene, as lines on stdout; whether the requirement held, or the scene is not judged"""
    import numpy as np
    import torch
    from renderbaby_amd import Engine, RenderConfig, abi, aov, bake
    dev = torch.device("cuda", 0)
    s = scene_of(name).with_params(spp=samples)
    rc = RenderConfig.from_scene(s)
    e = Engine.new(rc, device=0)
    e.update(rc)
    dirs = aov.pixel_centre_dirs(s.uniforms).reshape(-1, 3)
    n = len(dirs)
    rays = torch.zeros((n, 8), dtype=torch.float32, device=dev)
    rays[:, 0:3] = torch.tensor(s.uniforms["camera"]["pos"][0], dtype=torch.float32, device=dev)
    rays[:, 4:7] = torch.from_numpy(dirs).to(dev)
    out = torch.empty((n, 4), dtype=torch.float32, device=dev)

    def measure(which):
        if which == "render":
            e.dispatch(0, samples)
            e.sync()
            return e.last_dispatch_ms()
        e.trace_ray_records(rays, samples=samples, out=out)
        return e.last_query_ms()
    ms = alternating(("render", "query"), runs, measure)
    # the HBM rate a copy of the ray buffer achieves (read + write), for the allowance
    copy = torch.empty_like(rays)
    best = None
    for _ in range(4):
        t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        t0.record()
        copy.copy_(rays)
        t1.record()
        t1.synchronize()
        best = t0.elapsed_time(t1) if best is None else min(best, t0.elapsed_time(t1))
    rate = 2.0 * n * 32 / (best * 1e-3)
    allowance = n * 32 / rate * 1e3
    (mr, sr), (mq, sq) = med(ms["render"]), med(ms["query"])
    ok = mq <= mr + max(sr, sq) + allowance
    judged = name in JUDGED
    lit = float((out[:, :3] != 0).any(1).float().mean())
    print(f"{name:5} {s.width}x{s.height}x{samples} {n * samples:11d}  {e.last_kernel_name():14} {med_text(ms['render'])}  {e.last_query_kernel_name():12} "
          f"{med_text(ms['query'])}  {mq / mr:6.3f}  {allowance:7.3f} ms at {rate / 1e12:.2f} TB/s  {'held' if ok else 'MISSED'}{'' if judged else ' (recorded, not judged)'}"
          f"  lit {lit:.3f}", flush=True)
    if whole:
        host = rays.cpu().numpy().view(abi.RAY).reshape(-1)
        e.trace_ray_records(host[:1024], samples=samples)
        t0 = time.perf_counter()
        e.trace_ray_records(host, samples=samples)
        t_host = (time.perf_counter() - t0) * 1e3
        t0 = time.perf_counter()
        e.trace_ray_records(rays, samples=samples, out=out)
        t_dev = (time.perf_counter() - t0) * 1e3
        print(f"#   {name} whole calls, {n} rays x {samples}: rb_trace_rays (host) {t_host:.1f} ms (kernels {e.last_query_ms():.1f}); rb_trace_rays_device + rb_sync {t_dev:.1f} ms", flush=True)
        if name == "c3":
            rng = np.random.default_rng(1)
            m = 1 << 20
            pts = np.stack([rng.uniform(-6, 6, m), np.full(m, 4.5), rng.uniform(-12, 0, m)], axis=1).astype(np.float32)
            nrm = np.tile(np.array([0, 1, 0], np.float32), (m, 1))
            t0 = time.perf_counter()
            irr = bake.irradiance(e, pts, nrm, 16)
            print(f"#   c3 bake.irradiance, 2^20 points x 16 rays (rays built in numpy, host form): {(time.perf_counter() - t0) * 1e3:.0f} ms end to end, "
                  f"kernels {e.last_query_ms():.1f} ms, mean {float(irr.mean()):.4f}", flush=True)
    e.close()
    return ok or not judged


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--configs", default="c3,lamp,c5,c4,c2")
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--samples", type=int, default=16)
    ap.add_argument("--out", default=None)
    ap.add_argument("--no-whole-calls", action="store_true")
    ap.add_argument("--scene-timeout", "--child-timeout", type=int, default=300, help="seconds one scene's process may take")
    ap.add_argument("--one", default=None, help=argparse.SUPPRESS)
    a = ap.parse_args()
    if a.one:   # one scene in this process: its lines, the verdict as the exit status
        child_exit(one(a.one, a.runs, a.samples, not a.no_whole_calls))
    from renderbaby_amd._lib import source_fingerprint   # (this process never opens the device: the children do)
    with Report(a.out) as r:
        r.say(f"# library sources {source_fingerprint()}; one process per scene; {a.runs} alternating runs after one warm-up pair; kernel ms as median (max - min)")
        r.say("# render = rb_dispatch(e, 0, samples), rb_last_dispatch_ms (all launches, k_accumulate included); query = rb_trace_rays_device on the")
        r.say("# pixel-centre rays, rb_last_query_ms (all launches, k_rad_sum included).  The same number of paths through the same per-path code;")
        r.say("# the paths differ (jitter and seeds), so the work is the same statistically.  Requirement on c3, lamp, c5, c4: query <= render +")
        r.say("# max(spreads) + the time of reading n x 32 B of rays at the HBM rate of a device copy of the ray buffer (column `rays`).")
        r.say(f"{'scene':5} {'frame':16} {'paths':>11}  {'render kernel':14} {'ms':>18}  {'query kernel':12} {'ms':>18}  {'q/r':>6}  rays")

        def argv_of(name, first):
            return ([sys.executable, os.path.abspath(__file__), "--one", name, "--runs", str(a.runs), "--samples", str(a.samples)]
                    + (["--no-whole-calls"] if a.no_whole_calls else []))
        # a time limit of its own per scene: building the scene, a dozen launches of a second at the most, the whole calls
        held, _ = run_children(r, argv_of, a.configs.split(","), a.scene_timeout, merge_stderr=True)
        r.say(f"# the requirement held on every judged scene: {held}")
    return 0 if held else 1


if __name__ == "__main__":
    sys.exit(main())
