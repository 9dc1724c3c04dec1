"""The lightmap bake next to the hemisphere form it is built on, and what the numpy model costs a caller:

    python tools/lightmap_rate.py [--configs lamp,cubes] [--atlases 1024,4096] [--runs 5] [--samples 16] [--tile 64]
                                  [--model-atlas 1024] [--child-timeout 300] [--out profiles/r18_lightmap_rate.txt]

One process per scene.  `lamp`: the reference's lamp fixture with the uvs it carries (charts overlap: the owner rule decides).
`cubes`: the cube example tiled --tile x --tile times, every cube's two textured faces in a cell of their own of the atlas
(12 x tile^2 triangles).  For every atlas two ways to the same sums:

    bake        rb_bake_lightmap_device: surfels, rb_trace_hemisphere's pieces over them, resolve with two fill passes
    hemisphere  rb_trace_hemisphere_device on the same surfels, made beforehand by rb_lightmap_surfels_device

Kernel ms from rb_last_query_ms, the bake's first and last stage from rb_last_lightmap_ms; one warm-up pair, then `runs`
alternating pairs, median and spread (max - min).  The requirement: the bake's median is at most the hemisphere form's median plus
the larger of the two spreads plus the medians of surfels_ms and resolve_ms.  The exit status says whether it held everywhere.
Reported beside, without a pass mark: the bytes the surfel stage writes per second (36 B per texel: surfel and owner), and the
host seconds of the numpy model (lightmap.surfels) for the --model-atlas atlas: what a caller pays without the feature.
"""
import argparse, os, sys, time
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from _rate import Report, alternating, child_argv, child_exit, child_header, med, med_text, run_children

HEADER = (f"{'scene':6} {'tris':>7} {'atlas':>6} {'owned':>6} {'spp':>4}  {'bake ms':>18}  {'surfels ms':>16}  {'resolve ms':>16}  "
          f"{'hemisphere ms':>18}  {'bake/hemi':>9}  {'surfel TB/s':>11}  held")


def tiled_cubes(k):
    """the cube example k x k times on a grid in x and z, cube (i, j)'s uvs scaled into cell (i, j) of the unit square"""
    import numpy as np
    from renderbaby_amd import bvh, scene_io, scenes
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    s = scene_io.load_scene(os.path.join(root, "examples", "cube_scene", "scene.json"), total_samples=1)
    t0, uv0 = s.bvh_triangles, s.uvs.reshape(-1, 2)
    n = len(t0)
    tris = np.tile(t0, k * k)
    uvs = np.tile(uv0, (k * k, 1)).astype(np.float32)
    for c in range(k * k):
        i, j = c % k, c // k
        sl = slice(c * n, (c + 1) * n)
        for v in ("v0", "v1", "v2"):
            tris[v][sl] += np.float32([1.5 * (i - k / 2), 0.0, -1.5 * j])
            tris[v + "_index"][sl] += c * len(uv0)
        uvs[c * len(uv0):(c + 1) * len(uv0)] = (uv0 * 0.9 + 0.05 + np.float32([i, j])) / k
    nodes, indices = bvh.build(tris)
    u = s.uniforms.copy()
    u["bvh_node_count"], u["bvh_triangle_count"] = len(nodes), len(tris)
    return scenes.Scene(u, s.spheres, s.lights, s.meshes, nodes, indices, tris, uvs.reshape(-1).copy(), s.textures, "cubes")


def one(name, atlases, samples, runs, tile, model_atlas):
    import numpy as np
    import torch
    from renderbaby_amd import Engine, RenderConfig, abi, lightmap, refscenes

    def progress(what):
        print(f"[{name}] {what}", file=sys.stderr, flush=True)
    s = (refscenes.ref_lamp() if name == "lamp" else tiled_cubes(tile)).with_params(width=64, height=64, spp=1)
    rc = RenderConfig.from_scene(s)
    e = Engine.new(rc, device=0)
    e.update(rc)
    progress("scene uploaded")
    dev = torch.device("cuda", 0)
    lines, held = [], True
    for side in atlases:
        n = side * side
        surf = torch.empty((n, 8), dtype=torch.float32, device=dev)
        own = torch.empty((n,), dtype=torch.int32, device=dev)
        e.lightmap_surfels(side, side, out=(surf, own))
        owned = int((own != -1).sum().item())
        pts, nrm = surf[:, 0:3].contiguous(), surf[:, 4:7].contiguous()
        out_b = torch.empty((n, 4), dtype=torch.float32, device=dev)
        out_h = torch.empty((n, 4), dtype=torch.float32, device=dev)

        def measure(which):   # (kernel ms, surfels ms, resolve ms)
            if which == "bake":
                e.bake_lightmap(side, side, samples, dilate=2, out=out_b)
            else:
                e.trace_hemisphere(pts, nrm, samples, out=out_h)
            return (e.last_query_ms(),) + tuple(e.last_lightmap_ms())
        got = alternating(("bake", "hemi"), runs, measure)
        bake, surfels, resolve = ([v[i] for v in got["bake"]] for i in range(3))
        hemi = [v[0] for v in got["hemi"]]
        (mb, sb), (msf, ssf), (mrs, srs), (mh, sh) = med(bake), med(surfels), med(resolve), med(hemi)
        ok = mb <= mh + max(sb, sh) + msf + mrs
        held = held and ok
        rate = n * 36 / (msf * 1e-3) / 1e12
        lines.append(f"{name:6} {len(s.bvh_triangles):7d} {side:6d} {100.0 * owned / n:5.1f}% {samples:4d}  {med_text(bake)}  {msf:7.3f} ({ssf:6.3f})  "
                     f"{mrs:7.3f} ({srs:6.3f})  {med_text(hemi)}  {mb / mh:9.3f}  {rate:11.3f}  {ok}")
        progress(f"atlas {side} timed")
        del surf, own, pts, nrm, out_b, out_h
    t0 = time.perf_counter()
    lightmap.surfels(s.bvh_triangles, s.uvs, model_atlas, model_atlas)
    lines.append(f"#model {name:6} lightmap.surfels (numpy, host) for {model_atlas} x {model_atlas}: {time.perf_counter() - t0:8.2f} s")
    e.close()
    return lines, held


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--configs", default="lamp,cubes")
    ap.add_argument("--atlases", default="1024,4096")
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--samples", type=int, default=16)
    ap.add_argument("--tile", type=int, default=64)
    ap.add_argument("--model-atlas", type=int, default=1024)
    ap.add_argument("--child-timeout", type=int, default=300, help="seconds one scene's process may take")
    ap.add_argument("--out", default=None)
    ap.add_argument("--child", default=None, help=argparse.SUPPRESS)
    ap.add_argument("--header", action="store_true", help=argparse.SUPPRESS)
    a = ap.parse_args()
    if a.child:   # one scene in this process: its lines, the verdict as the exit status
        if a.header:
            child_header()
        lines, ok = one(a.child, [int(x) for x in a.atlases.split(",")], a.samples, a.runs, a.tile, a.model_atlas)
        print("\n".join(lines), flush=True)
        child_exit(ok)
    from renderbaby_amd._lib import source_fingerprint   # (this process never opens the device: the children do)
    with Report(a.out) as r:
        r.say(f"# library sources {source_fingerprint()}; {a.runs} alternating runs after one warm-up pair; kernel ms as median (max - min)")
        r.say("# bake = rb_bake_lightmap_device (surfels + trace + resolve with dilate 2, rb_last_query_ms; first and last stage: rb_last_lightmap_ms);")
        r.say("# hemisphere = rb_trace_hemisphere_device on the surfels rb_lightmap_surfels_device made beforehand; one process per scene")
        r.say(HEADER)
        options = ("atlases", "runs", "samples", "tile", "model_atlas")
        held, _ = run_children(r, lambda name, first: child_argv(__file__, name, a, options, first), a.configs.split(","), a.child_timeout)
        r.say(f"# bake median <= hemisphere median + max(spreads) + surfels median + resolve median for every scene and atlas: {held}")
    return 0 if held else 1


if __name__ == "__main__":
    sys.exit(main())
