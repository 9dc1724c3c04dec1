"""Light points from a baked probe grid: the rate of rb_light_points_device for both shapes of k_probe_light (DESIGN.md
section 19.4):

    python tools/probe_light_rate.py [--configs c2,c3] [--runs 5] [--grids 16,64] [--width 1920 --height 1080]
                                     [--out profiles/r23_probe_light_rate.txt]

One process.  Per scene: the first hits of the pixel centres of a --width x --height frame (Engine.render_hits) as surfels on the
device -- neighbouring points share their eight probes: the coherent case -- and the same surfels shuffled: the incoherent case;
a grid of G x G x G probes over the box of the hit points for every G of --grids, its coefficients synthetic (random sums through
rb_probe_coefficients_device: what they hold does not move the time).  rb_light_points_device on them once per shape
(RB_LIGHT_SHAPE):

    pairs  the corners in groups of two, five waves per SIMD
    wide   all eight corners' 56 loads in flight per lane, two waves per SIMD

One warm-up pair, then `runs` alternating pairs; kernel ms from rb_last_query_ms as median (max - min); points/s, and the
effective rate of the corner records read, 8 x 112 B per point, in GB/s (what the caches serve of it never reaches memory).
Nothing is required of the numbers: the faster shape becomes kLightShapeDefault by hand.
"""
import argparse, os, sys
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from _rate import Report, alternating, env, med, med_text, scene_of

HEADER = f"{'scene':6} {'grid':>6} {'points':10} {'shape':5} {'kernel':18} {'n':>8} {'ms':>18} {'points/s':>10} {'GB/s':>8}"
SHAPES = ("pairs", "wide")


def one(name, width, height, grids, runs, say):
    import numpy as np
    import torch
    from renderbaby_amd import Engine, RenderConfig, abi, aov, probes
    s = scene_of(name).with_params(width=width, height=height, spp=1)
    rc = RenderConfig.from_scene(s)
    e = Engine.new(rc, device=0)
    e.update(rc)
    _, pts, nrm = aov.ambient_occlusion_surfels(s.uniforms, e.render_hits())
    m = len(pts)
    if m == 0:
        raise SystemExit(f"{s.name}: no pixel centre hits anything")
    surf = np.zeros(m, dtype=abi.SURFEL)
    surf["pos"], surf["normal"] = pts, nrm
    dev = torch.device("cuda", 0)
    rng = np.random.default_rng(23)
    orders = {"coherent": torch.from_numpy(surf.view(np.float32).reshape(-1, 8)).to(dev),
              "shuffled": torch.from_numpy(surf[rng.permutation(m)].view(np.float32).reshape(-1, 8)).to(dev)}
    out = torch.empty((m, 4), dtype=torch.float32, device=dev)
    lo, hi = pts.min(0).astype(np.float64), pts.max(0).astype(np.float64)
    hi = np.maximum(hi, lo + 1e-3)
    for g in grids:
        grid = probes.grid_params(lo, hi, (g, g, g))
        sums = np.zeros(g ** 3, dtype=abi.SH9)
        sums["sum"] = rng.normal(size=(g ** 3, 9, 3)).astype(np.float32)
        sums["sum"][:, 0] += np.float32(8.0)
        sums["weight"] = 64.0
        co = torch.from_numpy(sums.view(np.float32).reshape(-1, 28)).to(dev)
        e.probe_coefficients(co, out=co)
        for order, t in orders.items():

            def measure(sh):   # (kernel ms, the kernel's name)
                with env("RB_LIGHT_SHAPE", sh):
                    e.light_points(grid, co, t, out=out)
                return e.last_query_ms(), e.last_query_kernel_name()
            for sh, got in alternating(SHAPES, runs, measure).items():
                ms = [v[0] for v in got]
                v = med(ms)[0]
                say(f"{name:6} {g:4d}^3 {order:10} {sh:5} {got[-1][1]:18} {m:8d} {med_text(ms)} {m / v * 1e3:10.3e} {m * 8 * 112 / v / 1e6:8.1f}")
    e.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--configs", default="c2,c3")
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--grids", default="16,64")
    ap.add_argument("--width", type=int, default=1920)
    ap.add_argument("--height", type=int, default=1080)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    from renderbaby_amd import engine
    from renderbaby_amd._lib import source_fingerprint
    report = Report(a.out)
    say = report.say
    say(f"# {engine.device_name(0)}")
    say(f"# library sources {source_fingerprint()}; {a.runs} alternating runs after one warm-up pair; kernel ms (rb_last_query_ms) as median (max - min)")
    say("# rb_light_points_device on the first hits of the frame's pixel centres (coherent) and on the same surfels shuffled; shape = RB_LIGHT_SHAPE;")
    say("# GB/s = 8 x 112 B of corner records per point over the kernel time; one process")
    say(HEADER)
    for name in a.configs.split(","):
        one(name, a.width, a.height, [int(g) for g in a.grids.split(",")], a.runs, say)
    report.close()
    return 0


if __name__ == "__main__":
    sys.exit(main())
