"""Camera rays made on the device next to the same rays given by the caller:

    python tools/camera_rate.py [--configs c2,c3,lamp,c4] [--runs 5] [--samples 16] [--width 1920 --height 1080]
                                [--child-timeout 300] [--out profiles/r13_camera_rate.txt]

One process per configuration.  In it, at --width x --height, a thin-lens PERSPECTIVE camera where the scene's own camera
stands, and two ways to the same paths:

    camera  rb_trace_camera_device, `samples` samples per pixel: k_cam_rays into the record scratch, the k_cam kernel, k_rad_sum
    rays    rb_trace_rays_device with samples = 1 on the n x `samples` records of that camera, made beforehand by
            rb_camera_rays and uploaded: the same rays; that entry point hashes an id into its seed, so the paths continue
            with other random numbers than the camera form's -- the same first segments, statistically the same work after them

    rays*   the ray form again on the same records put into the camera form's item order, [64 pixels][sample][64]: recorded, not
            judged.  In pixel-major order a wave's 64 rays are 4 pixels x 16 samples, in item order 64 pixels x 1 sample: what
            is left between camera and rays* is the camera form's own cost, what lies between rays and rays* is ray coherence

Kernel ms from rb_last_query_ms -- for the camera form that is generator, trace and sum together --, and the generator's share
from rb_last_camera_rays_ms; one warm-up pair, then `runs` alternating pairs, median and spread (max - min).  The requirement:
the camera form's median is at most the ray form's median plus the larger of the two spreads plus the generator's median.  The
exit status says whether it held for every configuration.
"""
import argparse, os, sys
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from _rate import Report, alternating, child_argv, child_exit, child_header, med, med_text, run_children, scene_of

HEADER = (f"{'scene':6} {'pixels':>9} {'spp':>4}  {'camera kernel':13} {'ms':>18}  {'generator ms':>18}  {'ray kernel':12} {'ms':>18}  {'rays* ms':>18}  "
          f"{'camera/rays':>11}  held")


def one(name, width, height, samples, runs):
    """the line of one configuration, and whether the requirement held"""
    import numpy as np
    import torch
    from renderbaby_amd import Engine, RenderConfig, camera, engine
    s = scene_of(name).with_params(spp=1)
    rc = RenderConfig.from_scene(s)
    e = Engine.new(rc, device=0)
    e.update(rc)
    c = s.uniforms["camera"][0]
    cam = camera.make("perspective", width, height, c["pos"], dir=c["dir"], fov_deg=50.0, aperture=0.1, focus_distance=5.0)
    n = width * height
    dev = torch.device("cuda", 0)
    records = torch.empty((n * samples, 8), dtype=torch.float32, device=dev)
    rows = max(1, (1 << 22) // (width * samples))   # the generator's own piece at a time through host memory
    for r0 in range(0, height, rows):
        first, m = r0 * width, min(rows, height - r0) * width
        rays, _ = engine.camera_rays_device(cam, samples, region=(first, m), device=0)
        records[first * samples:(first + m) * samples] = torch.from_numpy(rays.view(np.float32).reshape(-1, 8)).to(dev)
    # rays*: [block of 64 pixels][sample][64] (the last block, if it is not whole, stays pixel-major)
    whole = (n // 64) * 64
    reordered = records.clone()
    reordered[:whole * samples] = records[:whole * samples].view(n // 64, 64, samples, 8).permute(0, 2, 1, 3).reshape(-1, 8)
    out_c = torch.empty((n, 4), dtype=torch.float32, device=dev)
    out_r = torch.empty((n * samples, 4), dtype=torch.float32, device=dev)

    def measure(which):   # (kernel ms, the generator's share, the kernel's name)
        if which == "camera":
            e.trace_camera(cam, samples, out=out_c)
        else:
            e.trace_ray_records(records if which == "rays" else reordered, samples=1, out=out_r)
        return e.last_query_ms(), e.last_camera_rays_ms(), e.last_query_kernel_name()
    got = alternating(("camera", "rays", "rays*"), runs, measure)
    (cam_ms, gen, cam_k), (ray_ms, _, ray_k), (item_ms, _, _) = (tuple(zip(*got[which])) for which in ("camera", "rays", "rays*"))
    (mc, sc), mg, (mr, sr) = med(cam_ms), med(gen)[0], med(ray_ms)
    ok = mc <= mr + max(sc, sr) + mg
    e.close()
    return (f"{name:6} {n:9d} {samples:4d}  {cam_k[-1]:13} {med_text(cam_ms)}  {med_text(gen)}  {ray_k[-1]:12} {med_text(ray_ms)}  "
            f"{med_text(item_ms)}  {mc / mr:11.3f}  {ok}"), ok


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--configs", default="c2,c3,lamp,c4")
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--samples", type=int, default=16)
    ap.add_argument("--width", type=int, default=1920)
    ap.add_argument("--height", type=int, default=1080)
    ap.add_argument("--child-timeout", type=int, default=300, help="seconds one configuration's process may take")
    ap.add_argument("--out", default=None)
    ap.add_argument("--child", default=None, help=argparse.SUPPRESS)
    ap.add_argument("--header", action="store_true", help=argparse.SUPPRESS)
    a = ap.parse_args()
    if a.child:   # one configuration in this process: its line, the verdict as the exit status
        if a.header:
            child_header()
        line, ok = one(a.child, a.width, a.height, a.samples, a.runs)
        print(line, flush=True)
        child_exit(ok)
    from renderbaby_amd._lib import source_fingerprint   # (this process never opens the device: the children do)
    with Report(a.out) as r:
        r.say(f"# library sources {source_fingerprint()}; {a.runs} alternating runs after one warm-up pair; kernel ms as median (max - min)")
        r.say("# camera = rb_trace_camera_device (generator + trace + sum, rb_last_query_ms; generator alone: rb_last_camera_rays_ms);")
        r.say("# rays = rb_trace_rays_device, samples = 1, on the camera's n x spp records made by rb_camera_rays; one process per scene")
        r.say("# rays* = the same records in the camera form's item order, [64 pixels][sample][64]: recorded, not judged")
        r.say(HEADER)
        held, _ = run_children(r, lambda name, first: child_argv(__file__, name, a, ("runs", "samples", "width", "height"), first),
                               a.configs.split(","), a.child_timeout)
        r.say(f"# camera median <= ray median + max(spreads) + generator median for every scene: {held}")
    return 0 if held else 1


if __name__ == "__main__":
    sys.exit(main())
