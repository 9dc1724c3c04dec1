"""Probe visibility: where a depth bake's kernel time goes for both folds of k_depth_project, and what the visibility weights
cost the blend (the protocols of sections 18.4 and 19.4):

    python tools/probe_visibility_rate.py [--configs c2,c3] [--runs 5] [--probes 4096] [--samples 1024] [--grids 16,64]
                                          [--width 1920 --height 1080] [--out profiles/r24_probe_visibility_rate.txt]

One process.  Per scene:

  bake   `probes` probes spread evenly over the first hits of the frame's pixel centres (Engine.render_hits), pushed 0.05 along
         the normal into free space; rb_bake_probe_depth_device on them with `samples` samples each, once per fold of
         k_depth_project (RB_DEPTH_SHAPE):
             lds       a row's 64 terms parked in LDS, every lane reads entry j at one address
             readlane  lane j's four words read across into scalar registers
         Kernel ms of the whole call from rb_last_query_ms, the generator's share from rb_last_camera_rays_ms, the projection's
         from rb_last_probe_depth_project_ms; the query (k_query*) is the rest.
  blend  the first hits as surfels on the device (coherent) and shuffled, a grid of G x G x G probes over their box for every
         G of --grids with synthetic coefficients and moments (what they hold does not move the time);
         rb_light_points_device (k_probe_light) against rb_light_points_visible_device (k_probe_light_vis) on the same points.
         GB/s = the corner data a point reads, 8 x 112 B (x (112 + 16) B with the texels), over the kernel time: an effective
         rate, the caches serve most of it.  A 64^3 grid's maps are 268 MB: beyond the caches, every texel is a line from memory.

One warm-up pair, then `runs` alternating pairs; median (max - min).  Nothing is required of the numbers: the faster fold becomes
kDepthShapeDefault by hand.
"""
import argparse, os, sys
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from _rate import Report, alternating, env, med, med_text, scene_of

BAKE_HEADER = (f"{'scene':6} {'fold':8} {'probes':>7} {'spp':>5}  {'kernel':14} {'total ms':>18}  {'generator ms':>18}  {'query ms':>18}  "
               f"{'projection ms':>18}  {'items/s':>10} {'proj GB/s':>9}")
BLEND_HEADER = f"{'scene':6} {'grid':>6} {'points':10} {'kernel':18} {'n':>8} {'ms':>18} {'points/s':>10} {'GB/s':>8}"
FOLDS = ("lds", "readlane")


def one(name, a, say):
    import numpy as np
    import torch
    from renderbaby_amd import Engine, RenderConfig, abi, aov, probes
    s = scene_of(name).with_params(width=a.width, height=a.height, spp=1)
    rc = RenderConfig.from_scene(s)
    e = Engine.new(rc, device=0)
    e.update(rc)
    _, pts, nrm = aov.ambient_occlusion_surfels(s.uniforms, e.render_hits())
    m = len(pts)
    if m == 0:
        raise SystemExit(f"{s.name}: no pixel centre hits anything")
    dev = torch.device("cuda", 0)
    rng = np.random.default_rng(23)
    lo, hi = pts.min(0).astype(np.float64), pts.max(0).astype(np.float64)
    hi = np.maximum(hi, lo + 1e-3)

    # ---- the bake
    pick = np.linspace(0, m - 1, a.probes).astype(np.int64)
    pos = torch.from_numpy(np.ascontiguousarray((pts[pick] + np.float32(0.05) * nrm[pick]).astype(np.float32))).to(dev)
    maps = torch.empty((a.probes, 256), dtype=torch.float32, device=dev)
    reach = float(1.5 * np.linalg.norm((hi - lo) / 16.0))
    words = {}

    def bake(f):   # (total, generator and projection ms, the kernel's name); the warm-up call's words are kept
        with env("RB_DEPTH_SHAPE", f):
            e.bake_probe_depth(pos, a.samples, reach, out=maps)
        if f not in words:
            words[f] = maps.view(torch.int32).clone()
        return e.last_query_ms(), e.last_camera_rays_ms(), e.last_probe_depth_project_ms(), e.last_query_kernel_name()
    baked = alternating(FOLDS, a.runs, bake)
    if not torch.equal(words["lds"], words["readlane"]):
        raise SystemExit("the two folds disagree")
    say(BAKE_HEADER)
    items = a.probes * a.samples
    for f, got in baked.items():
        tot, gen, proj = ([v[i] for v in got] for i in range(3))
        query = [x - y - z for x, y, z in zip(tot, gen, proj)]
        cells = "  ".join(med_text(x) for x in (tot, gen, query, proj))
        say(f"{name:6} {f:8} {a.probes:7d} {a.samples:5d}  {got[-1][3]:14} {cells}  {items / med(tot)[0] * 1e3:10.3e} {items * 48 / med(proj)[0] / 1e6:9.1f}")

    # ---- the blend
    surf = np.zeros(m, dtype=abi.SURFEL)
    surf["pos"], surf["normal"] = pts, nrm
    orders = {"coherent": torch.from_numpy(surf.view(np.float32).reshape(-1, 8)).to(dev),
              "shuffled": torch.from_numpy(surf[rng.permutation(m)].view(np.float32).reshape(-1, 8)).to(dev)}
    out = torch.empty((m, 4), dtype=torch.float32, device=dev)
    say(BLEND_HEADER)
    for g in a.grids:
        grid = probes.grid_params(lo, hi, (g, g, g))
        sums = np.zeros(g ** 3, dtype=abi.SH9)
        sums["sum"] = rng.normal(size=(g ** 3, 9, 3)).astype(np.float32)
        sums["sum"][:, 0] += np.float32(8.0)
        sums["weight"] = 64.0
        co = torch.from_numpy(sums.view(np.float32).reshape(-1, 28)).to(dev)
        e.probe_coefficients(co, out=co)
        cell = float(np.linalg.norm(grid["step"]))
        mom = torch.empty((g ** 3, 64, 4), dtype=torch.float32, device=dev)
        mom[:, :, 0] = torch.rand((g ** 3, 64), device=dev) * cell + 0.5 * cell
        mom[:, :, 1] = mom[:, :, 0] ** 2 + torch.rand((g ** 3, 64), device=dev) * (0.1 * cell * cell)
        mom[:, :, 2] = 1.0
        mom[:, :, 3] = 0.0
        mom = mom.reshape(-1, 256)
        calls = {"plain": (lambda pts_t: e.light_points(grid, co, pts_t, out=out), 8 * 112),
                 "visible": (lambda pts_t: e.light_points_visible(grid, co, mom, pts_t, normal_bias=0.01 * cell, out=out), 8 * 128)}
        for order, pts_t in orders.items():
            def blend(k):   # (kernel ms, the kernel's name)
                calls[k][0](pts_t)
                return e.last_query_ms(), e.last_query_kernel_name()
            for k, got in alternating(calls, a.runs, blend).items():
                ms = [x[0] for x in got]
                v = med(ms)[0]
                say(f"{name:6} {g:4d}^3 {order:10} {got[-1][1]:18} {m:8d} {med_text(ms)} {m / v * 1e3:10.3e} {m * calls[k][1] / v / 1e6:8.1f}")
        del mom, co
    e.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--configs", default="c2,c3")
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--probes", type=int, default=4096)
    ap.add_argument("--samples", type=int, default=1024)
    ap.add_argument("--grids", default="16,64")
    ap.add_argument("--width", type=int, default=1920)
    ap.add_argument("--height", type=int, default=1080)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    a.grids = [int(g) for g in a.grids.split(",")]
    from renderbaby_amd import engine
    from renderbaby_amd._lib import source_fingerprint
    report = Report(a.out)
    say = report.say
    say(f"# {engine.device_name(0)}")
    say(f"# library sources {source_fingerprint()}; {a.runs} alternating runs after one warm-up pair; kernel ms as median (max - min); one process")
    say("# bake: rb_bake_probe_depth_device, fold = RB_DEPTH_SHAPE; proj GB/s = the 48 B of record and hit quads read per item over the projection's time")
    say("# blend: rb_light_points_device against rb_light_points_visible_device on the same points; GB/s = 8 corners x (112 B, or 112 + 16 B) per point")
    for name in a.configs.split(","):
        one(name, a, say)
    report.close()
    return 0


if __name__ == "__main__":
    sys.exit(main())
