"""Irradiance probes made on the device: the rate of a bake and where its kernel time goes, for both shapes of the projection
(DESIGN.md section 18.4):

    python tools/probe_rate.py [--configs c2,c3] [--runs 5] [--probes 4096] [--samples 1024] [--width 480 --height 270]
                               [--out profiles/r21_probe_rate.txt]

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
import argparse, os, statistics, subprocess, sys
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

HEADER = (f"{'scene':6} {'shape':6} {'probes':>7} {'spp':>5}  {'kernel':12} {'total ms':>18}  {'generator ms':>18}  {'trace ms':>18}  "
          f"{'projection ms':>18}  {'probes/s':>10} {'items/s':>10}")
AXES = [(1, 0, 0), (-1, 0, 0), (0, 1, 0), (0, -1, 0), (0, 0, 1), (0, 0, -1)]


def scene_of(name):
    from renderbaby_amd import scenes
    return {"c2": scenes.cornell_c2, "c3": scenes.mesh_c3, "feature": scenes.feature_scene}[name]()


def med(xs):
    return statistics.median(xs), max(xs) - min(xs)


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
    shapes = ("plain", "split")
    ms = {sh: {"all": [], "gen": [], "proj": []} for sh in shapes}
    kernel = ""
    for run in range(runs + 1):
        for sh in (shapes if run % 2 == 0 else shapes[::-1]):
            os.environ["RB_PROBE_SHAPE"] = sh
            e.bake_probes(tp, samples, out=out)
            kernel = e.last_query_kernel_name()
            if run:
                ms[sh]["all"].append(e.last_query_ms())
                ms[sh]["gen"].append(e.last_camera_rays_ms())
                ms[sh]["proj"].append(e.last_probe_project_ms())
    lines = []
    for sh in shapes:
        m = ms[sh]
        trace = [a - g - p for a, g, p in zip(m["all"], m["gen"], m["proj"])]
        (ma, sa), (mg, sg), (mt, st), (mp, sp) = med(m["all"]), med(m["gen"]), med(trace), med(m["proj"])
        lines.append(f"{name:6} {sh:6} {n:7d} {samples:5d}  {kernel:12} {ma:9.3f} ({sa:6.3f})  {mg:9.3f} ({sg:6.3f})  {mt:9.3f} ({st:6.3f})  "
                     f"{mp:9.3f} ({sp:6.3f})  {n / ma * 1e3:10.3e} {n * samples / ma * 1e3:10.3e}")
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
    ap.add_argument("--out", default=None)
    ap.add_argument("--child", default=None, help=argparse.SUPPRESS)
    ap.add_argument("--header", action="store_true", help=argparse.SUPPRESS)
    a = ap.parse_args()
    if a.child:   # one configuration in this process
        if a.header:
            from renderbaby_amd import engine
            print(f"# {engine.device_name(0)}", flush=True)
        lines = truncation(a.samples, 256) if a.child == "truncation" else one(a.child, a.width, a.height, a.samples, a.runs, a.probes)
        print("\n".join(lines), flush=True)
        return 0
    from renderbaby_amd._lib import source_fingerprint   # (this process never opens the device: the children do)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    out_file = open(a.out, "w") if a.out else None

    def say(s=""):
        print(s, flush=True)
        if out_file:   # line by line: a run that is cut short keeps what it measured
            out_file.write(s + "\n")
            out_file.flush()
    say(f"# library sources {source_fingerprint()}; {a.runs} alternating runs after one warm-up pair; kernel ms as median (max - min)")
    say("# rb_bake_probes_device: total = rb_last_query_ms, generator = rb_last_camera_rays_ms, projection = rb_last_probe_project_ms,")
    say("# trace = the rest (queue word, k_cam kernel, k_rad_sum); shape = RB_PROBE_SHAPE; one process per scene")
    say(HEADER)
    ok = True
    for i, name in enumerate(a.configs.split(",") + ["truncation"]):
        p = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", name, "--runs", str(a.runs), "--samples", str(a.samples),
                            "--probes", str(a.probes), "--width", str(a.width), "--height", str(a.height)] + (["--header"] if i == 0 else []),
                           stdout=subprocess.PIPE, text=True)
        for line in p.stdout.splitlines():
            say(line)
        if p.returncode != 0:
            say(f"{name:6} failed: exit status {p.returncode}")
            ok = False
            break   # whatever ended that process may have left the device in a bad state: nothing more is started on it
    if out_file:
        out_file.close()
    return 0 if ok else 1


if __name__ == "__main__":
    sys.exit(main())
