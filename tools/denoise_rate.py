"""Times and quality of the edge-avoiding a-trous denoiser on one MI355X:

    python tools/denoise_rate.py [--configs c2,c3] [--sizes 1920x1080,512x512] [--repeats 9] [--spp 4] [--no-quality]

Per configuration and frame size, after one warm-up and as median (max - min) over the repeats, from HIP events on the engine's
stream (rb_last_denoise_ms):
  * kernel ms of a whole denoise (prepare + iterations + finish) with the default parameters, and per iteration: the time of a
    run of k iterations minus that of k - 1 (the earlier iterations do the same work in both, so the difference is iteration
    k - 1, step 2^(k-1)); iterations = 0 is prepare + finish alone;
  * the bytes the taps must move -- per filtered pixel and iteration 16 B for the colour | class of every tap inside the frame,
    32 B more (normal | t, position) for every tap of the pixel's class, 48 B for the pixel itself and 16 B written, counted
    from the engine's guide buffer with numpy -- and the rate achieved against them;
  * the plain iteration kernel against the LDS-staged one for steps 1 and 2 (RB_DENOISE_VARIANT), alternating;
  * the guide-buffer build (pixel-centre query + pack), and one 1-spp pass of the same scene and frame in the same session.
Then the quality figures of section 13: 256 x 256, depth 4, mean squared error of x / (x + 1) against the same engine's
1024-spp render, raw 4 spp against denoised 4 spp.
"""
import argparse, os, statistics, sys
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from _rate import env, med, scene_of


def tap_bytes(cls, iterations):
    """bytes per iteration the taps must move, from the classes of the guide buffer"""
    import numpy as np
    h, w = cls.shape
    live = cls != 0
    out = []
    for i in range(iterations):
        s = 1 << i
        inside = same = 0
        for dy in range(-2, 3):
            for dx in range(-2, 3):
                oy, ox = dy * s, dx * s
                if abs(oy) >= h or abs(ox) >= w:
                    continue
                a = (slice(max(0, -oy), min(h, h - oy)), slice(max(0, -ox), min(w, w - ox)))
                b = (slice(max(0, oy), min(h, h + oy)), slice(max(0, ox), min(w, w + ox)))
                inside += int(live[a].sum())
                same += int((live[a] & (cls[a] == cls[b])).sum())
        out.append(16 * inside + 32 * same + int(live.sum()) * 48 + h * w * 16)
    return out


def tone_mse(lin, ref):
    import numpy as np
    a, b = lin[..., :3].astype(np.float64), ref[..., :3].astype(np.float64)
    return float((((a / (a + 1)) - (b / (b + 1))) ** 2).mean())


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--configs", default="c2,c3")
    ap.add_argument("--sizes", default="1920x1080,512x512")
    ap.add_argument("--repeats", type=int, default=9)
    ap.add_argument("--spp", type=int, default=4)
    ap.add_argument("--no-quality", action="store_true")
    a = ap.parse_args()
    import numpy as np
    from renderbaby_amd import Engine, RenderConfig, denoise, engine, scenes
    dflt = denoise.default_params()
    n_it = int(dflt["iterations"])
    print(f"# {engine.device_name(0)}; repeats {a.repeats} after one warm-up; ms as median (max - min); defaults {dflt}")
    os.environ.pop("RB_DENOISE_VARIANT", None)
    for name in a.configs.split(","):
        for size in a.sizes.split(","):
            w, h = (int(x) for x in size.split("x"))
            s = scene_of(name).with_params(width=w, height=h, spp=a.spp)
            rc = RenderConfig.from_scene(s)
            e = Engine.new(rc, device=0)
            e.render(rc)
            import torch
            d_img = torch.empty((h, w, 4), dtype=torch.uint8, device="cuda:0")

            def run(p):
                e.denoise(p, out=d_img)
                return e.last_denoise_ms()
            _, guide_ms = run(dflt)   # the first denoise after the update builds the guides
            cls = e.denoise_guides()["cls"]
            # one 1-spp pass of this scene and frame, the same session
            pass_ms = []
            for _ in range(a.repeats + 1):
                e.clear()
                e.dispatch(0, 1)
                e.sync()
                pass_ms.append(e.last_dispatch_ms())
            e.render(rc)
            run(dflt)
            total = [run(dflt)[0] for _ in range(a.repeats + 1)][1:]
            by_k = []
            for k in range(n_it + 1):
                p = denoise.params(iterations=k)
                by_k.append([run(p)[0] for _ in range(a.repeats + 1)][1:])
            per_it = [statistics.median(by_k[k]) - statistics.median(by_k[k - 1]) for k in range(1, n_it + 1)]
            tb = tap_bytes(cls, n_it)
            (t, ts), (pm, ps) = med(total), med(pass_ms[1:])
            print(f"{name} {w}x{h}: {100.0 * (cls != 0).mean():.1f} % of the pixels filterable; guide build {guide_ms:.3f} ms; one 1-spp pass [{e.last_kernel_name()}] "
                  f"{pm:.3f} ({ps:.3f}) ms")
            print(f"  denoise, {n_it} iterations: {t:.3f} ({ts:.3f}) ms of kernels; prepare + finish {med(by_k[0])[0]:.3f} ({med(by_k[0])[1]:.3f}) ms")
            for i, (ms, b) in enumerate(zip(per_it, tb)):
                print(f"  iteration {i} (step {1 << i}): {ms:.3f} ms, {b / 1e6:.1f} MB of taps -> {b / ms / 1e9:.2f} TB/s")
            print(f"  all iterations: {sum(tb) / 1e6:.1f} MB -> {sum(tb) / sum(per_it) / 1e9:.2f} TB/s")
            # plain against LDS-staged for steps 1 and 2 (iterations = 2 holds exactly these), alternating
            p2, res = denoise.params(iterations=2), {"plain": [], "lds": []}
            for r in range(a.repeats + 1):
                for v in ("plain", "lds"):
                    with env("RB_DENOISE_VARIANT", v):
                        ms = run(p2)[0]
                    if r:
                        res[v].append(ms)
            base = statistics.median(by_k[0])
            (pl, pls), (ld, lds) = med(res["plain"]), med(res["lds"])
            print(f"  steps 1 + 2 with prepare + finish: plain {pl:.3f} ({pls:.3f}) ms, LDS-staged {ld:.3f} ({lds:.3f}) ms; "
                  f"the two iterations alone: plain {pl - base:.3f} ms, LDS-staged {ld - base:.3f} ms", flush=True)
            e.close()
    if a.no_quality:
        return
    for name, make in (("cornell", lambda spp: scenes.cornell(256, 256, spp, 4)), ("mesh", lambda spp: scenes.mesh_scene(48, 48, 256, 256, spp, 4, seed=3))):
        out = {}
        for spp in (1024, 4):
            rc = RenderConfig.from_scene(make(spp))
            e = Engine.new(rc, device=0)
            e.render(rc)
            out[spp] = e.denoise(denoise.params(iterations=0), linear=True)
            if spp == 4:
                den = e.denoise(linear=True)
            e.close()
        m_raw, m_den = tone_mse(out[4], out[1024]), tone_mse(den, out[1024])
        print(f"quality {name} 256x256 depth 4, MSE of x/(x+1) against 1024 spp: raw 4 spp {m_raw:.6g}, denoised 4 spp {m_den:.6g}, ratio {m_den / m_raw:.4f}")


if __name__ == "__main__":
    main()
