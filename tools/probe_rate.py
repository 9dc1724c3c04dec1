"""Irradiance probes made on the device: the rate of a bake and where its kernel time goes, for both shapes of the projection
(DESIGN.md section 18.4):

    python tools/probe_rate.py [--configs c2,c3] [--runs 5] [--probes 4096] [--samples 1024] [--width 480 --height 270]
                               [--child-timeout 300] [--out profiles/r21_probe_rate.txt]

One process per configuration.  In it the scene at --width x --height (the frame only places the probes), `probes` probes spread
evenly over the first hits of its pixel centres (Engine.render_hits) and pushed 0.05 along the normal into free space, and
rb_bake_probes_device on them with `samples` samples each, once per shape of k_sh_project (RB_PROBE_SHAPE):

    plain  one wavefront per block of 64 probes folds all nine coefficients
    split  three wavefronts per block of 64 probes, three coefficients each: three times the waves, the rows read three times

Kernel ms of the whole call from rb_last_query_ms, the generator's share from rb_last_camera_rays_ms, the projection's from
rb_last_probe_project_ms; the trace (queue word, k_cam kernel and the k_rad_sum pass launch_radiance makes beside it) is the
rest.  One warm-up pair, then `runs` alternating pairs, median and spread (max - min).  Nothing is required of the numbers: the
faster shape becomes kProbeShapeDefault by hand.

Then, in a process of its own on the feature scene, printed and not judged: the relative difference between
probes.irradiance(sh, n) / pi and bake.irradiance_device at the same points for the six axis normals -- the truncation at band 2
plus the noise of two estimators.
"""
import argparse, os, sys
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from _rate import Report, alternating, child_argv, child_exit, child_header, env, med, med_text, run_children, scene_of

HEADER = (f"{'scene':6} {'shape':6} {'probes':>7} {'spp':>5}  {'kernel':12} {'total ms':>18}  {'generator ms':>18}  {'trace ms':>18}  "
          f"{'projection ms':>18}  {'probes/s':>10} {'items/s':>10}")
AXES = [(1, 0, 0), (-1, 0, 0), (0, 1, 0), (0, -1, 0), (0, 0, 1), (0, 0, -1)]


def placed(e, s, n):
    """n points of free space: evenly over the first hits, 0.05 along the normal towards the camera; with them the hit normals"""
    import numpy as np
    from renderbaby_amd import aov
    _, pts, nrm = aov.ambient_occlusion_surfels(s.uniforms, e.render_hits())
    if len(pts) == 0:
        raise SystemExit(f"{s.name}: no pixel centre hits anything")
    pick = (np.arange(n, dtype=np.int64) * len(pts)) // n
    return np.ascontiguousarray((pts[pick] + np.float32(0.05) * nrm[pick]).astype(np.float32)), np.ascontiguousarray(nrm[pick])


def one(name, width, height, samples, runs, n):
    import torch
    from renderbaby_amd import Engine, RenderConfig
    s = scene_of(name).with_params(width=width, height=height, spp=1)
    rc = RenderConfig.from_scene(s)
    e = Engine.new(rc, device=0)
    e.update(rc)
    pos, _ = placed(e, s, n)
    tp = torch.from_numpy(pos).to(torch.device("cuda", 0))
    out = torch.empty((n, 28), dtype=torch.float32, device=tp.device)

    def measure(sh):   # (total, generator and projection ms, the kernel's name)
        with env("RB_PROBE_SHAPE", sh):
            e.bake_probes(tp, samples, out=out)
        return e.last_query_ms(), e.last_camera_rays_ms(), e.last_probe_project_ms(), e.last_query_kernel_name()
    got = alternating(("plain", "split"), runs, measure)
    kernel = got["plain" if runs % 2 else "split"][-1][3]   # (of the last call)
    lines = []
    for sh, m in got.items():
        total, gen, proj = ([v[i] for v in m] for i in range(3))
        trace = [a - g - p for a, g, p in zip(total, gen, proj)]
        ma = med(total)[0]
        lines.append(f"{name:6} {sh:6} {n:7d} {samples:5d}  {kernel:12} {med_text(total)}  {med_text(gen)}  {med_text(trace)}  "
                     f"{med_text(proj)}  {n / ma * 1e3:10.3e} {n * samples / ma * 1e3:10.3e}")
    e.close()
    return lines


def truncation(samples, n):
    """probes.irradiance / pi beside bake.irradiance_device on the feature scene, at n points, for the six axis normals"""
    import numpy as np
    from renderbaby_amd import Engine, RenderConfig, bake, probes
    s = scene_of("feature")
    rc = RenderConfig.from_scene(s)
    e = Engine.new(rc, device=0)
    e.update(rc)
    pos, _ = placed(e, s, n)
    sh = e.bake_probes(pos, samples)
    from_sh = probes.irradiance(sh, np.float32(AXES)) / np.pi                      # (n, 6, 3)
    lines = []
    for j, axis in enumerate(AXES):
        # offset 0: the hemisphere's rays start at the probe's own position
        direct = bake.irradiance_device(e, pos, np.tile(np.float32(axis), (n, 1)), samples, offset=0.0).astype(np.float64)
        scale = np.maximum(np.abs(direct).mean(1), 1e-6)
        rel = np.abs(from_sh[:, j] - direct).mean(1) / scale
        lines.append(f"#sh9 feature normal {axis!s:12} {n} probes x {samples}: |E_sh9 / pi - hemisphere mean| / hemisphere mean, median {np.median(rel):.3f}  "
                     f"90th percentile {np.quantile(rel, 0.9):.3f}  largest {rel.max():.3f}")
    e.close()
    return lines


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--configs", default="c2,c3")
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--probes", type=int, default=4096)
    ap.add_argument("--samples", type=int, default=1024)
    ap.add_argument("--width", type=int, default=480)
    ap.add_argument("--height", type=int, default=270)
    ap.add_argument("--child-timeout", type=int, default=300, help="seconds one configuration's process may take")
    ap.add_argument("--out", default=None)
    ap.add_argument("--child", default=None, help=argparse.SUPPRESS)
    ap.add_argument("--header", action="store_true", help=argparse.SUPPRESS)
    a = ap.parse_args()
    if a.child:   # one configuration in this process
        if a.header:
            child_header()
        lines = truncation(a.samples, 256) if a.child == "truncation" else one(a.child, a.width, a.height, a.samples, a.runs, a.probes)
        print("\n".join(lines), flush=True)
        child_exit()
    from renderbaby_amd._lib import source_fingerprint   # (this process never opens the device: the children do)
    with Report(a.out) as r:
        r.say(f"# library sources {source_fingerprint()}; {a.runs} alternating runs after one warm-up pair; kernel ms as median (max - min)")
        r.say("# rb_bake_probes_device: total = rb_last_query_ms, generator = rb_last_camera_rays_ms, projection = rb_last_probe_project_ms,")
        r.say("# trace = the rest (queue word, k_cam kernel, k_rad_sum); shape = RB_PROBE_SHAPE; one process per scene")
        r.say(HEADER)
        options = ("runs", "samples", "probes", "width", "height")
        ok, _ = run_children(r, lambda name, first: child_argv(__file__, name, a, options, first), a.configs.split(",") + ["truncation"], a.child_timeout)
    return 0 if ok else 1


if __name__ == "__main__":
    sys.exit(main())
