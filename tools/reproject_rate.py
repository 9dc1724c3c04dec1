"""Times and quality of the temporal reprojection on one MI355X:

    python tools/reproject_rate.py [--configs c2,c3] [--sizes 1920x1080,512x512] [--repeats 9] [--no-speed] [--no-quality] [--sweep]

Speed.  Per configuration, frame size and camera turn (still, 0.5 and 5 degrees about y, alternating between two cameras), after
one warm-up and as median (max - min) over the repeats, from HIP events on the engine's stream: steps 2 + 3 of
rb_denoise_history (REPROJECT + MERGE: the first call after an update), step 3 alone (MERGE: a second call in the same update),
the filter behind them, and the yardsticks of the same session: rb_denoise and one 1-spp pass.  Steps 2 + 3 against their
compulsory traffic of 160 B per pixel: 48 + 16 current, 64 previous at one texel per pixel, 16 out, 16 base.

Quality.  Section 13.4's set-up: 256 x 256, depth 4, mean squared error of x / (x + 1) against a 1024-spp render at the final
camera.  The camera turns in 16 steps of 0.5 degrees; per step one 1-spp pass and rb_denoise_history.  At the last step: the raw
frame, rb_denoise, the history alone (rb_history_read) and history + filter -- with the colour term off and on -- and per step
the share of filterable pixels that had no history.  ``--sweep``: the last step's history + filter over normal_min x max_history.
"""
import argparse, os, sys
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from _rate import med, scene_of


def turned(uniforms, degrees):
    """a copy of the uniforms with the camera turned about the y axis"""
    import numpy as np
    u = uniforms.copy()
    d = np.asarray(u["camera"]["dir"][0], np.float64)
    c, s = np.cos(np.radians(degrees)), np.sin(np.radians(degrees))
    u["camera"]["dir"][0] = (c * d[0] + s * d[2], d[1], -s * d[0] + c * d[2])
    return u


def tone_mse(lin, ref):
    import numpy as np
    a, b = lin[..., :3].astype(np.float64), ref[..., :3].astype(np.float64)
    return float((((a / (a + 1)) - (b / (b + 1))) ** 2).mean())


def speed(a):
    import torch
    from renderbaby_amd import Change, Engine, RenderConfig
    for name in a.configs.split(","):
        for size in a.sizes.split(","):
            w, h = (int(x) for x in size.split("x"))
            s = scene_of(name).with_params(width=w, height=h, spp=1)
            rc = RenderConfig.from_scene(s)
            e = Engine.new(rc, device=0)
            e.render(rc)
            d_img = torch.empty((h, w, 4), dtype=torch.uint8, device="cuda:0")
            for deg in (0.0, 0.5, 5.0):
                cams = (s.uniforms, turned(s.uniforms, deg))
                e.history_reset()
                both, merge, filt, plain, pass_ms, none = [], [], [], [], [], []
                for r in range(a.repeats + 2):   # the first has no history, the second is the warm-up
                    e.update(RenderConfig(uniforms=Change.update(cams[r & 1])))
                    e.clear()
                    e.dispatch(0, 1)
                    e.sync()
                    pass_ms.append(e.last_dispatch_ms())
                    e.denoise(out=d_img)   # (builds this update's guides, outside the timed calls)
                    plain.append(e.last_denoise_ms()[0])
                    e.denoise_history(out=d_img)
                    both.append(e.last_reproject_ms())
                    filt.append(e.last_denoise_ms()[0])
                    e.denoise_history(out=d_img)
                    merge.append(e.last_reproject_ms())
                    if r == a.repeats + 1:
                        g, F = e.denoise_guides(), e.history()
                        live = g["cls"] != 0
                        none = float(((F[..., 3] == 1) & live).sum()) / max(int(live.sum()), 1)
                (b, bs), (m, ms), (f, fs), (p, ps), (t, ts) = (med(x[2:]) for x in (both, merge, filt, plain, pass_ms))
                print(f"{name} {w}x{h} turn {deg} deg: steps 2 + 3 {b:.4f} ({bs:.4f}) ms = {160.0 * w * h / b / 1e6:.0f} GB/s of 160 B/pixel; "
                      f"step 3 alone {m:.4f} ({ms:.4f}) ms; filter behind them {f:.4f} ({fs:.4f}) ms; rb_denoise {p:.4f} ({ps:.4f}) ms; "
                      f"one 1-spp pass [{e.last_kernel_name()}] {t:.3f} ({ts:.3f}) ms; {100 * none:.1f} % of the filterable pixels without history",
                      flush=True)
            e.close()


def quality(a):
    import numpy as np
    from renderbaby_amd import Change, Engine, RenderConfig, denoise, scenes, temporal
    steps, step_deg = 16, 0.5
    for name, make in (("cornell", lambda spp: scenes.cornell(256, 256, spp, 4)), ("mesh", lambda spp: scenes.mesh_scene(48, 48, 256, 256, spp, 4, seed=3))):
        s = make(1024)
        final = turned(s.uniforms, steps * step_deg)
        rc = RenderConfig.from_scene(s)
        e = Engine.new(rc, device=0)
        e.update(rc)
        e.render(RenderConfig(uniforms=Change.update(final)))
        ref = e.denoise(denoise.params(iterations=0), linear=True)
        e.close()

        def run(rparams, dparams):
            s1 = make(1)
            rc1 = RenderConfig.from_scene(s1)
            e = Engine.new(rc1, device=0)
            e.update(rc1)
            shares = []
            for k in range(steps + 1):
                e.update(RenderConfig(uniforms=Change.update(turned(s1.uniforms, k * step_deg))))
                e.clear()
                e.dispatch(0, 1)
                e.sync()
                out = e.denoise_history(rparams, dparams, linear=True)
                F, live = e.history(), e.denoise_guides()["cls"] != 0
                shares.append(float(((F[..., 3] == 1) & live).sum()) / max(int(live.sum()), 1))
            res = dict(raw=tone_mse(e.denoise(denoise.params(iterations=0), linear=True), ref), denoise=tone_mse(e.denoise(dparams, linear=True), ref),
                       history=tone_mse(F, ref), both=tone_mse(out, ref), count=float(F[..., 3][live].mean()))
            e.close()
            return res, shares
        for sc in (0.0, 4.0):
            res, shares = run(temporal.default_params(), denoise.params(sigma_color=sc))
            print(f"quality {name} 256x256 depth 4, 16 x 0.5 deg, sigma_color {sc}: MSE of x/(x+1) against 1024 spp at the final camera: raw 1 spp "
                  f"{res['raw']:.6g}, rb_denoise {res['denoise']:.6g}, history alone {res['history']:.6g}, history + filter {res['both']:.6g}; "
                  f"mean count of the filterable pixels {res['count']:.2f}")
            if sc == 0.0:
                print(f"  share of filterable pixels without history per step: {' '.join(f'{100 * x:.1f}' for x in shares[1:])} %", flush=True)
        if a.sweep:
            for nm in (0.5, 0.8, 0.9, 0.97):
                for mh in (8.0, 16.0, 32.0, 64.0):
                    res, _ = run(temporal.params(normal_min=nm, max_history=mh), denoise.default_params())
                    print(f"  sweep {name}: normal_min {nm} max_history {mh:.0f}: history alone {res['history']:.6g}, history + filter {res['both']:.6g}", flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--configs", default="c2,c3")
    ap.add_argument("--sizes", default="1920x1080,512x512")
    ap.add_argument("--repeats", type=int, default=9)
    ap.add_argument("--no-speed", action="store_true")
    ap.add_argument("--no-quality", action="store_true")
    ap.add_argument("--sweep", action="store_true")
    a = ap.parse_args()
    from renderbaby_amd import engine, temporal
    print(f"# {engine.device_name(0)}; repeats {a.repeats} after a warm-up; ms as median (max - min); defaults {temporal.default_params()}")
    if not a.no_speed:
        speed(a)
    if not a.no_quality:
        quality(a)


if __name__ == "__main__":
    main()
