"""Render a RenderBaby scene file (.json or .rscn) to a PNG through the HIP backend:

    python tools/render_scene.py scene.rscn out.png [--spp N] [--max-depth D] [--fast-bvh] [--device-bvh]
                                 [--width W --height H] [--included-root DIR] [--every N]
                                 [--aov depth,normal,albedo,emission,id,ao] [--ao-radius R]
                                 [--denoise [--denoise-iterations N]]
                                 [--camera equirect|ortho|thin-lens [--ortho-width W] [--aperture A --focus-distance F] [--jitter]]
                                 [--probe x,y,z [--probe-normal x,y,z]] [--device-rays]
                                 [--lightmap W H [--lightmap-mesh i] [--lightmap-flip] [--direct [--pick power | --pick grid NX NY NZ |
                                                                                          --pick learned NX NY NZ [--learn ROUNDS SAMPLES]]]]
                                 [--probe-grid NX NY NZ] [--lit-by-probes NX NY NZ [--probe-visibility]]

scene file -> scene_io.load_scene (the importer's and the Scene->RenderConfig adapter's rules) ->
RenderConfig -> librenderbaby_hip.so -> Frame -> PNG.  With --every N the progressive iterator is used
and a frame is written every N samples (out_0001.png, ...).  --aov writes the first-hit buffers of the pixel centres
(Engine.render_hits -> renderbaby_amd.aov) next to the frame as out.<name>.png; `ao` is ambient occlusion over those hits
(aov.ambient_occlusion: 16 directions per hit, one any-hit query).  --denoise writes the frame through the edge-avoiding
a-trous filter (Engine.denoise) as out.denoised.png -- with --every, every delivered frame next to the raw
one (out_0001.denoised.png, ...).  --camera renders the scene a second time through a camera the scene file cannot express, at
the scene camera's position and direction (bake.camera_rays -> bake.render_rays: Engine.trace_rays on one ray per pixel, spp
samples each), as out.<camera>.png; with --jitter every sample's ray is made on the device instead -- sub-pixel jitter and, for the
thin lens, a lens point per sample, focused on a plane at the focus distance (camera.make -> bake.render_camera:
Engine.trace_camera).  --probe prints the mean radiance over the cosine-weighted hemisphere at a point
(bake.irradiance, spp rays; normal +y unless --probe-normal says otherwise).  --device-rays makes the hemisphere rays of
--aov ao and --probe on the device (aov.ambient_occlusion_device, bake.irradiance_device): other
directions than the host generators', the same estimate.  --lightmap W H bakes the scene's lightmap over its uvs on the device
(bake.lightmap -> Engine.bake_lightmap, spp samples per texel) and writes it as out.lightmap.png in the
texture's own encoding (bake.lightmap_texture), for one mesh with --lightmap-mesh; with --aov ao also the ambient-occlusion map
of the same texels (aov.ambient_occlusion_map) as out.lightmap.ao.png, and with --direct the map of the direct light alone --
spp shadow rays per texel to points on the scene's emitters (bake.lightmap_direct -> Engine.direct_light)
-- as out.lightmap.direct.png; --pick power picks each ray's emitter in proportion to its emission times its area (section 23);
--pick grid NX NY NZ picks it from a table per cell of a grid over the bounding box of the emitters and the mesh, weighted by
power over squared distance to the cell (bake.pick_grid -> Engine.direct_light(pick=("grid", grid)); section 24);
--pick learned NX NY NZ trains such tables first on which emitters the texels of each cell see -- --learn ROUNDS SAMPLES training
samples per texel, default 2 16, which lie behind the rendered ones and are not rendered (bake.learn_grid; section 25).
--probe-grid NX NY NZ bakes a grid of irradiance probes
over the bounding box of the scene's triangles and spheres (probes.grid -> bake.probes: Engine.bake_probes, spp uniform-sphere
rays per probe, traced and projected onto SH9 on the device) and writes out.probes.npz with `positions`
(n, 3) and `coefficients` (n, 9, 3), which probes.irradiance evaluates for any normal.  --lit-by-probes NX NY NZ bakes the same
grid (bake.probe_grid, spp rays per probe) and lights the first hits of the pixel centres from it in one launch
(aov.probe_lit -> Engine.light_points): out.probe_lit.png through aov.color_map shows what the grid holds --
emission + albedo x the blended irradiance over pi, no shadows --, so a bake can be judged before anything consumes it.
--probe-visibility bakes the probes' depth maps beside them and blends with the visibility weights (bake.probe_grid(visibility=
True) -> Engine.bake_probe_depth, Engine.probe_moments; Engine.light_points_visible): probes inside geometry
drop out and light no longer leaks through walls.
"""
import argparse, os, sys, time
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from renderbaby_amd import Engine, Frame, RenderConfig, aov, bake, camera, denoise, probes, scene_io  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("scene"); ap.add_argument("png")
ap.add_argument("--spp", type=int, default=None); ap.add_argument("--max-depth", type=int, default=5)
ap.add_argument("--width", type=int, default=0); ap.add_argument("--height", type=int, default=0)
ap.add_argument("--fast-bvh", action="store_true"); ap.add_argument("--device-bvh", action="store_true")
ap.add_argument("--build-tree", action="store_true", help="send triangles only: the engine builds the mesh's tree on the device")
ap.add_argument("--included-root", default=None); ap.add_argument("--every", type=int, default=0)
ap.add_argument("--aov", default="", help="comma-separated first-hit buffers to write as out.<name>.png: " + ", ".join(aov.NAMES) + ", ao")
ap.add_argument("--ao-radius", type=float, default=1.0, help="how far an occluder may be for --aov ao")
ap.add_argument("--denoise", action="store_true", help="also write every frame filtered, as <name>.denoised.png")
ap.add_argument("--denoise-iterations", type=int, default=None, help="a-trous iterations, 0..8 (default: the library's)")
ap.add_argument("--camera", choices=["equirect", "ortho", "thin-lens"], default=None, help="also write out.<camera>.png through bake.render_rays")
ap.add_argument("--ortho-width", type=float, default=10.0); ap.add_argument("--aperture", type=float, default=0.1)
ap.add_argument("--focus-distance", type=float, default=5.0)
ap.add_argument("--jitter", action="store_true", help="--camera with a ray per sample, made on the device: anti-aliased, and a thin lens that blurs")
ap.add_argument("--probe", default=None, help="x,y,z: print the mean radiance arriving at this point (bake.irradiance)")
ap.add_argument("--probe-normal", default="0,1,0")
ap.add_argument("--device-rays", action="store_true", help="--aov ao and --probe with their hemisphere rays made on the device (DESIGN.md section 16)")
ap.add_argument("--lightmap", type=int, nargs=2, metavar=("W", "H"), default=None, help="also bake the lightmap over the scene's uvs, as out.lightmap.png")
ap.add_argument("--lightmap-mesh", type=int, default=None, help="--lightmap for the triangles of this mesh index only")
ap.add_argument("--lightmap-flip", action="store_true", help="--lightmap with the triangles' normals negated")
ap.add_argument("--direct", action="store_true", help="with --lightmap: also the map of the direct light alone, by shadow rays to the scene's emitters, as out.lightmap.direct.png")
ap.add_argument("--pick", nargs="+", default=["uniform"], metavar="HOW",
                help="--direct: how a shadow ray picks its emitter: uniform, power (DESIGN.md section 23), grid NX NY NZ (section 24) or learned NX NY NZ (section 25)")
ap.add_argument("--learn", type=int, nargs=2, metavar=("ROUNDS", "SAMPLES"), default=[2, 16],
                help="--pick learned: training rounds and samples per texel and round (DESIGN.md section 25)")
ap.add_argument("--probe-grid", type=int, nargs=3, metavar=("NX", "NY", "NZ"), default=None,
                help="also bake a grid of irradiance probes over the scene's bounding box, as out.probes.npz")
ap.add_argument("--lit-by-probes", type=int, nargs=3, metavar=("NX", "NY", "NZ"), default=None,
                help="also light the first hits from a grid of probes baked over the scene's bounding box, as out.probe_lit.png")
ap.add_argument("--probe-visibility", action="store_true", help="--lit-by-probes with the probes' depth maps and the leak-free blend (DESIGN.md section 20)")
a = ap.parse_args()
if a.pick not in (["uniform"], ["power"]) and not (len(a.pick) == 4 and a.pick[0] in ("grid", "learned") and all(c.isdigit() and int(c) > 0 for c in a.pick[1:])):
    ap.error("--pick: uniform, power, grid NX NY NZ or learned NX NY NZ")
if a.learn[0] < 0 or a.learn[1] < 1:
    ap.error("--learn: ROUNDS >= 0 and SAMPLES >= 1")
aovs = [n for n in a.aov.split(",") if n]
for n in aovs:
    if n not in aov.NAMES + ("ao",):
        ap.error(f"unknown AOV {n!r}: one of {', '.join(aov.NAMES)}, ao")

t0 = time.time()
s = scene_io.load_scene(a.scene, total_samples=a.spp, max_depth=a.max_depth, included_root=a.included_root)
if a.width and a.height:
    s = s.with_params(width=a.width, height=a.height)
print(f"loaded {a.scene}: {len(s.bvh_triangles)} triangles, {len(s.spheres)} spheres, {len(s.lights)} lights, "
      f"{len(s.textures)} textures, {s.width}x{s.height}, {s.total_samples} spp ({time.time() - t0:.2f} s)")
rc = RenderConfig.from_scene(s, with_tree=not a.build_tree)
eng = Engine.new(rc, fast_bvh=a.fast_bvh, device_bvh=a.device_bvh, build_tree="device" if a.build_tree else None)
dn_params = denoise.params(**({} if a.denoise_iterations is None else dict(iterations=a.denoise_iterations)))
dn_ms = []


def export_denoised(path):
    """the committed frame through the filter, next to `path`"""
    img = eng.denoise(dn_params)
    dn_ms.append(eng.last_denoise_ms()[0])
    b, x = os.path.splitext(path)
    scene_io.export_png(f"{b}.denoised{x}", Frame(img.shape[1], img.shape[0], img))


t0 = time.time()
if a.every > 0:
    base, ext = os.path.splitext(a.png)
    for i, frame in enumerate(eng.frame_iterator(rc, passes_per_frame=a.every)):
        scene_io.export_png(f"{base}_{i + 1:04d}{ext}", frame)
        if a.denoise:
            export_denoised(f"{base}_{i + 1:04d}{ext}")
    scene_io.export_png(a.png, frame)
else:
    frame = eng.render(rc)
    scene_io.export_png(a.png, frame)
if a.denoise:
    export_denoised(a.png)
dt = time.time() - t0
st = eng.stats()
print(f"rendered with {eng.last_kernel_name()} in {dt:.3f} s: {st['segments'] / dt / 1e6:.0f} M ray-segments/s -> {a.png}")
if a.denoise:
    print(f"denoised {len(dn_ms)} frame(s), {int(dn_params['iterations'])} iterations: {sum(dn_ms) / len(dn_ms):.3f} ms of kernels per frame")
if aovs:
    hits, surf = eng.render_hits(surfaces=True)
    base, ext = os.path.splitext(a.png)
    for n in aovs:
        ao = aov.ambient_occlusion_device if a.device_rays else aov.ambient_occlusion
        img = aov.ao_u8(ao(eng, hits, radius=a.ao_radius)) if n == "ao" else aov.image(n, hits, surf)
        scene_io.export_png(f"{base}.{n}{ext}", Frame(img.shape[1], img.shape[0], img))
    print(f"first-hit buffers with {eng.last_query_kernel_name()} in {eng.last_query_ms():.3f} ms: {', '.join(aovs)}")
if a.camera:
    kind = a.camera.replace("-", "_")
    cam = s.uniforms["camera"][0]
    spp = min(max(s.total_samples, 1), 65536)
    if a.jitter:
        cam_ex = camera.make("perspective" if kind == "thin_lens" else kind, s.width, s.height, cam["pos"], dir=cam["dir"],
                             ortho_width=a.ortho_width, aperture=a.aperture, focus_distance=a.focus_distance)
        img = bake.render_camera(eng, cam_ex, spp)
    else:
        O, D = bake.camera_rays(kind, s.width, s.height, cam["pos"], dir=cam["dir"], ortho_width=a.ortho_width, aperture=a.aperture,
                                focus_distance=a.focus_distance)
        img = bake.render_rays(eng, O, D, spp)
    base, ext = os.path.splitext(a.png)
    scene_io.export_png(f"{base}.{kind}{ext}", Frame(img.shape[1], img.shape[0], img))
    print(f"{a.camera} camera with {eng.last_query_kernel_name()} in {eng.last_query_ms():.3f} ms -> {base}.{kind}{ext}")
if a.probe:
    point, normal = [[float(v) for v in t.split(",")] for t in (a.probe, a.probe_normal)]
    rays = max(s.total_samples, 1)
    if a.device_rays:
        rays = min(rays, 65536)   # rb_trace_hemisphere's limit for one call
        rgb = bake.irradiance_device(eng, [point], [normal], rays)[0]
    else:
        rgb = bake.irradiance(eng, [point], [normal], rays)[0]
    print(f"probe at {tuple(point)}, normal {tuple(normal)}, {rays} rays: mean radiance {rgb[0]:.6g} {rgb[1]:.6g} {rgb[2]:.6g}")
if a.lightmap:
    import numpy as np
    w, h = a.lightmap
    spp = min(max(s.total_samples, 1), 65536)
    base, ext = os.path.splitext(a.png)
    rgba = bake.lightmap(eng, w, h, spp, mesh=a.lightmap_mesh, flip=a.lightmap_flip)
    surfels_ms, resolve_ms = eng.last_lightmap_ms()
    scene_io.export_png(f"{base}.lightmap{ext}", Frame(w, h, bake.lightmap_texture(rgba).view(np.uint8)))
    print(f"lightmap {w} x {h}, {spp} samples per texel, {int((rgba[..., 3] == 1).sum())} baked and {int((rgba[..., 3] == 2).sum())} filled texels, "
          f"with {eng.last_query_kernel_name()} in {eng.last_query_ms():.3f} ms (surfels {surfels_ms:.3f}, resolve {resolve_ms:.3f}) -> {base}.lightmap{ext}")
    if a.direct:
        pick = a.pick[0]
        if pick in ("grid", "learned"):
            tri = s.bvh_triangles
            cells = bake.pick_grid(eng.scene_emitters(), [int(c) for c in a.pick[1:]],
                                   points=np.concatenate([tri[k].reshape(-1, 3) for k in ("v0", "v1", "v2")]))
            pick = ("grid", cells) if pick == "grid" else ("learned", cells, a.learn[0], a.learn[1])
        picked = " ".join(a.pick) + (f" after {a.learn[0]} rounds of {a.learn[1]} training samples" if a.pick[0] == "learned" else "")
        direct_map = bake.lightmap_direct(eng, w, h, spp, mesh=a.lightmap_mesh, flip=a.lightmap_flip, pick=pick)
        scene_io.export_png(f"{base}.lightmap.direct{ext}", Frame(w, h, bake.lightmap_texture(direct_map).view(np.uint8)))
        print(f"direct-light map of {len(eng.scene_emitters())} emitters, {spp} shadow rays per texel picked by {picked}, with {eng.last_query_kernel_name()} "
              f"-> {base}.lightmap.direct{ext}")
    if "ao" in aovs:
        ao = aov.ambient_occlusion_map(eng, w, h, 16, a.ao_radius, mesh=a.lightmap_mesh, flip=a.lightmap_flip)
        img = aov.ao_u8(np.where(np.isnan(ao), np.float32(0), ao))
        scene_io.export_png(f"{base}.lightmap.ao{ext}", Frame(w, h, img))
        print(f"ambient-occlusion map with {eng.last_query_kernel_name()} in {eng.last_query_ms():.3f} ms -> {base}.lightmap.ao{ext}")


def scene_box(option):
    """the bounding box of the scene's triangles and spheres, for the options that span a grid of probes over it"""
    import numpy as np
    tri = s.bvh_triangles
    lo = [tri[k].reshape(-1, 3) for k in ("v0", "v1", "v2")] + [s.spheres["center"] - s.spheres["radius"][:, None]]
    hi = lo[:3] + [s.spheres["center"] + s.spheres["radius"][:, None]]
    if not len(tri) and not len(s.spheres):
        ap.error(f"{option}: the scene has neither triangles nor spheres to span a box")
    return np.concatenate(lo).min(0), np.concatenate(hi).max(0)


if a.probe_grid:
    import numpy as np
    lo, hi = scene_box("--probe-grid")
    pos = probes.grid(lo, hi, a.probe_grid)
    spp = min(max(s.total_samples, 1), 65536)
    coeff = bake.probes(eng, pos, spp)
    base, _ = os.path.splitext(a.png)
    np.savez(f"{base}.probes.npz", positions=pos, coefficients=coeff)
    print(f"{len(pos)} probes over {tuple(float(v) for v in lo)} .. {tuple(float(v) for v in hi)}, {spp} rays each, with {eng.last_query_kernel_name()} in {eng.last_query_ms():.3f} ms "
          f"(generator {eng.last_camera_rays_ms():.3f}, projection {eng.last_probe_project_ms():.3f}) -> {base}.probes.npz")
if a.lit_by_probes:
    lo, hi = scene_box("--lit-by-probes")
    spp = min(max(s.total_samples, 1), 65536)
    grid, coeffs, *maps = bake.probe_grid(eng, lo, hi, a.lit_by_probes, spp, visibility=a.probe_visibility)
    hits, surf = eng.render_hits(surfaces=True)
    import numpy as np
    rgb = aov.color_map(aov.probe_lit(eng, grid, coeffs, hits, surf, moments=maps[0] if maps else None))
    img = np.concatenate([rgb, np.full(rgb.shape[:2] + (1,), 255, np.uint8)], axis=-1)
    base, ext = os.path.splitext(a.png)
    scene_io.export_png(f"{base}.probe_lit{ext}", Frame(img.shape[1], img.shape[0], img))
    print(f"{len(coeffs)} probes over {tuple(float(v) for v in lo)} .. {tuple(float(v) for v in hi)}, {spp} rays each ({int((coeffs['weight'] > 0).sum())} valid); "
          f"the first hits of {s.width}x{s.height} pixels lit with {eng.last_query_kernel_name()} in {eng.last_query_ms():.3f} ms -> {base}.probe_lit{ext}")
eng.close()
