"""Any-hit occlusion next to the closest-hit query on the same rays:

    python tools/occlusion_rate.py [--configs c3,lamp,c5,c4] [--runs 5] [--ao-hits 4194304] [--out profiles/r08_occlusion_rate.txt]

Per configuration at its BASELINE frame size, two ray sets in device memory: (a) the pixel-centre rays, (b) the rays of
aov.ambient_occlusion -- 16 cosine-weighted directions per first hit, built on the device from the records of (a) with torch (at
most --ao-hits first hits, evenly spaced over the frame).  On each, `runs` alternating pairs of rb_cast_rays_device (hits only:
the yardstick, the closest-hit kernel) and rb_occluded_device (tmax NULL, RB_MASK_ALL) in one process on the same buffers;
kernel ms from rb_last_query_ms after one warm-up pair, median and spread (max - min).  The requirement: the any-hit median is
not above the closest-hit median by more than the larger of the two spreads; the exit status says whether it held everywhere.
Then whole-call times, recorded and not judged: rb_occluded / rb_cast_rays from host memory, the device forms, and one
ambient_occlusion at 1920 x 1080 x 16 on C3 end to end.
"""
import argparse, os, sys, time
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from _rate import Report, alternating, med, med_text, scene_of


def ao_rays_device(uniforms, dirs, hits, n_dirs, seed, max_hits):
    """aov.ambient_occlusion_rays on the device: (n, 8) ray records from the (n, 12) hit records of the pixel-centre rays"""
    import torch
    from renderbaby_amd import abi
    kind = hits[:, 1].view(torch.int32)
    idx = torch.nonzero((kind != abi.HIT_NONE) & (kind != -1)).reshape(-1)
    if len(idx) > max_hits:
        idx = idx[torch.linspace(0, len(idx) - 1, max_hits, device=idx.device).long()]
    d, t, n = dirs[idx], hits[idx, 0:1], hits[idx, 8:11]
    n = torch.where((n * d).sum(-1, keepdim=True) > 0, -n, n)
    cam = torch.tensor(uniforms["camera"]["pos"][0], dtype=torch.float32, device=d.device)
    org = cam + t * d + n * (1e-3 * torch.clamp(t, min=1.0))
    g = torch.Generator(device=d.device).manual_seed(seed)
    r1 = torch.rand((len(idx), n_dirs), generator=g, device=d.device)
    r2 = torch.rand((len(idx), n_dirs), generator=g, device=d.device)
    phi, r = 6.283185307179586 * r1, torch.sqrt(r2)
    a = torch.where(n[:, 0:1].abs() > 0.5, torch.tensor([0.0, 1.0, 0.0], device=d.device), torch.tensor([1.0, 0.0, 0.0], device=d.device))
    tx = torch.nn.functional.normalize(torch.linalg.cross(a, n), dim=-1)
    ty = torch.linalg.cross(n, tx)
    dd = (r * torch.cos(phi))[..., None] * tx[:, None, :] + (r * torch.sin(phi))[..., None] * ty[:, None, :] \
        + torch.sqrt(torch.clamp(1.0 - r2, min=0.0))[..., None] * n[:, None, :]
    rays = torch.zeros((len(idx) * n_dirs, 8), dtype=torch.float32, device=d.device)
    rays[:, 0:3] = org.repeat_interleave(n_dirs, dim=0)
    rays[:, 4:7] = dd.reshape(-1, 3)
    return rays


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--configs", default="c3,lamp,c5,c4")
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--ao-hits", type=int, default=1 << 22)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import numpy as np
    import torch
    from renderbaby_amd import Engine, RenderConfig, abi, aov, engine
    from renderbaby_amd._lib import source_fingerprint
    held = True
    report = Report(a.out)
    say = report.say
    say(f"# {engine.device_name(0)}; library sources {source_fingerprint()}; {a.runs} alternating runs after one warm-up pair; kernel ms as median (max - min)")
    say(f"# closest = rb_cast_rays_device, hits only; any = rb_occluded_device, tmax NULL, RB_MASK_ALL; same process, same buffers")
    say(f"{'scene':6} {'rays':10} {'n':>10} {'occluded':>9}  {'closest kernel':15} {'ms':>18}  {'any kernel':13} {'ms':>18}  {'any/closest':>11}  held")
    dev = torch.device("cuda", 0)
    for name in a.configs.split(","):
        s = scene_of(name).with_params(spp=1)
        rc = RenderConfig.from_scene(s)
        e = Engine.new(rc, device=0)
        e.update(rc)
        dirs = torch.from_numpy(aov.pixel_centre_dirs(s.uniforms).reshape(-1, 3)).to(dev)
        pix = torch.zeros((len(dirs), 8), dtype=torch.float32, device=dev)
        pix[:, 0:3] = torch.tensor(s.uniforms["camera"]["pos"][0], dtype=torch.float32, device=dev)
        pix[:, 4:7] = dirs
        first = e.cast_ray_records(pix)
        sets = [("pixels", pix), ("ao x16", ao_rays_device(s.uniforms, dirs, first, 16, 0, a.ao_hits))]
        del first
        for label, rays in sets:
            n = len(rays)
            hits = torch.empty((n, 12), dtype=torch.float32, device=dev)
            out = torch.empty(n, dtype=torch.uint8, device=dev)

            def measure(which):   # (kernel ms, the kernel's name)
                if which == "closest":
                    e.cast_ray_records(rays, hits_out=hits)
                else:
                    e.occluded_records(rays, out=out)
                return e.last_query_ms(), e.last_query_kernel_name()
            got = alternating(("closest", "any"), a.runs, measure)
            ms = {which: [v[0] for v in got[which]] for which in got}
            names = {which: got[which][-1][1] for which in got}
            (mc, sc), (ma, sa) = med(ms["closest"]), med(ms["any"])
            ok = ma <= mc + max(sc, sa)
            held = held and ok
            occ = float((out == abi.OCCL_OCCLUDED).float().mean())
            say(f"{name:6} {label:10} {n:10d} {occ:9.3f}  {names['closest']:15} {med_text(ms['closest'])}  {names['any']:13} {med_text(ms['any'])}  {ma / mc:11.3f}  {ok}")
            del hits, out
        # whole calls on the pixel rays: host memory in and out against the device forms
        host = pix.cpu().numpy().view(abi.RAY).reshape(-1)
        t = {}
        for label, fn in (("rb_cast_rays (host)", lambda: e.cast_ray_records(host)), ("rb_occluded (host)", lambda: e.occluded_records(host)),
                          ("rb_cast_rays_device + rb_sync", lambda: e.cast_ray_records(pix)), ("rb_occluded_device + rb_sync", lambda: e.occluded_records(pix))):
            fn()
            w = []
            for _ in range(3):
                t0 = time.perf_counter()
                fn()
                w.append((time.perf_counter() - t0) * 1e3)
            t[label] = med(w)
        say(f"#   {name} whole calls, {len(host)} pixel rays, ms: " + "; ".join(f"{k} {v[0]:.2f} ({v[1]:.2f})" for k, v in t.items()))
        if name == "c3":
            hits = e.render_hits()
            aov.ambient_occlusion(e, hits, 16, 1.0)
            t0 = time.perf_counter()
            ao = aov.ambient_occlusion(e, hits, 16, 1.0)
            say(f"#   c3 aov.ambient_occlusion {hits.shape[1]} x {hits.shape[0]} x 16 (rays built in numpy, host form): {(time.perf_counter() - t0) * 1e3:.0f} ms end to end, "
                f"kernel {e.last_query_ms():.2f} ms, mean AO {float(ao.mean()):.3f}")
        e.close()
        del pix, dirs, sets
        torch.cuda.empty_cache()
    say(f"# any-hit median <= closest-hit median + max(spreads) on every scene and ray set: {held}")
    report.close()
    return 0 if held else 1


if __name__ == "__main__":
    sys.exit(main())
