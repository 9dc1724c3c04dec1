"""Rates of the closest-hit queries next to the project's nearest existing work, a depth-1 render:

    python tools/query_rate.py [--configs c3,lamp,c4,c5] [--repeats 7] [--rays 16777216] [--yardstick-tree DIR]

Per configuration at its BASELINE frame size: (a) rb_render_hits -- kernel ms (HIP events around the kernels,
rb_last_query_ms) and call ms (wall clock, read-back included), median and spread over the repeats after one warm-up;
(b) the yardstick -- rb_dispatch(e, 0, 1) with max_depth = 1 and 1 spp on the same scene and frame: one primary segment per
pixel through the same walk, kernel ms from rb_last_dispatch_ms.  With --yardstick-tree the yardstick runs in a child
process on the package and library of that directory (a checkout of the parent commit with its library built: the number
then does not come from the code under test); without it, on this build.  Then rb_cast_rays rays/s for random rays into the last configuration, pageable and
page-locked, and rb_pick latency.
"""
import argparse, ctypes as C, json, os, statistics, subprocess, sys, time
# (the yardstick child imports the package of the tree it was pointed at)
sys.path.insert(0, os.environ.get("RB_QUERY_RATE_TREE") or os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from _rate import med, scene_of


def yardstick(name, repeats):
    from renderbaby_amd import Engine, RenderConfig
    s = scene_of(name).with_params(spp=1, max_depth=1)
    rc = RenderConfig.from_scene(s)
    e = Engine.new(rc, device=0)
    e.update(rc)
    ms = []
    for i in range(repeats + 1):
        e.clear()
        e.dispatch(0, 1)
        e.sync()
        ms.append(e.last_dispatch_ms())
    k = e.last_kernel_name()
    e.close()
    return dict(kernel=k, ms=ms[1:])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--configs", default="c3,lamp,c4,c5")
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--rays", type=int, default=1 << 24)
    ap.add_argument("--yardstick-tree", default=None)
    ap.add_argument("--yardstick-child", default=None, help=argparse.SUPPRESS)
    a = ap.parse_args()
    if a.yardstick_child:
        print("YARDSTICK " + json.dumps(yardstick(a.yardstick_child, a.repeats)))
        return
    import numpy as np
    from renderbaby_amd import Engine, RenderConfig, abi, engine
    from renderbaby_amd._lib import load
    print(f"# {engine.device_name(0)}; repeats {a.repeats} after one warm-up; ms as median (max - min)")
    e = s = None
    for name in a.configs.split(","):
        if a.yardstick_tree:
            env = dict(os.environ, RB_QUERY_RATE_TREE=os.path.abspath(a.yardstick_tree))
            env.pop("RB_LIBRARY_PATH", None)
            out = subprocess.run([sys.executable, os.path.abspath(__file__), "--yardstick-child", name, "--repeats", str(a.repeats)],
                                 env=env, capture_output=True, text=True, timeout=900, cwd=env["RB_QUERY_RATE_TREE"])
            line = [ln for ln in out.stdout.splitlines() if ln.startswith("YARDSTICK ")]
            if out.returncode != 0 or not line:
                raise SystemExit(f"yardstick child failed ({out.returncode}): {out.stderr[-400:]}")
            y = json.loads(line[0][10:])
        else:
            y = yardstick(name, a.repeats)
        if e is not None:
            e.close()
        s = scene_of(name)
        rc = RenderConfig.from_scene(s)
        e = Engine.new(rc, device=0)
        e.update(rc)
        kms, cms, cms_h = [], [], []
        for i in range(a.repeats + 1):
            t0 = time.perf_counter()
            e.render_hits(surfaces=True)
            cms.append((time.perf_counter() - t0) * 1e3)
            kms.append(e.last_query_ms())
            t0 = time.perf_counter()
            e.render_hits()
            cms_h.append((time.perf_counter() - t0) * 1e3)
        (k, ks), (c, cs), (ch, chs), (ym, ys) = med(kms[1:]), med(cms[1:]), med(cms_h[1:]), med(y["ms"])
        verdict = "within" if k <= ym + ys else "ABOVE"
        print(f"{name:5s} {s.width}x{s.height}  render_hits[{e.last_query_kernel_name()}] kernel {k:.3f} ({ks:.3f}) ms, call with surfaces {c:.1f} ({cs:.1f}) ms, "
              f"hits only {ch:.1f} ({chs:.1f}) ms | depth-1 dispatch[{y['kernel']}{' on the yardstick tree' if a.yardstick_tree else ''}] "
              f"kernel {ym:.3f} ({ys:.3f}) ms | query {verdict} yardstick + spread", flush=True)
    # rays into the last configuration, from the camera towards the scene
    n = a.rays
    rng = np.random.default_rng(1)
    rays = np.zeros(n, dtype=abi.RAY)
    rays["origin"] = s.uniforms["camera"]["pos"][0]
    d = rng.normal(size=(n, 3)).astype(np.float32) * np.float32(0.3) + np.asarray(s.uniforms["camera"]["dir"][0], np.float32)
    rays["dir"] = d
    lib = load()
    for label in ("pageable", "page-locked"):
        if label == "page-locked":
            pr, ph = lib.rb_host_alloc(n * 32), lib.rb_host_alloc(n * 48)
            r2 = np.ctypeslib.as_array((C.c_uint8 * (n * 32)).from_address(pr)).view(abi.RAY)
            r2[:] = rays
            hits = np.ctypeslib.as_array((C.c_uint8 * (n * 48)).from_address(ph)).view(abi.HIT)
        else:
            r2, hits = rays, np.empty(n, dtype=abi.HIT)
        ts, ks = [], []
        for i in range(a.repeats + 1):
            t0 = time.perf_counter()
            e.cast_ray_records(r2, hits_out=hits)
            ts.append(time.perf_counter() - t0)
            ks.append(e.last_query_ms())
        t, tsp = med(ts[1:])
        print(f"cast_rays {n} rays, {label}: {n / t / 1e6:.1f} M rays/s per call ({t * 1e3:.1f} ({tsp * 1e3:.1f}) ms), kernels {med(ks[1:])[0]:.2f} ms "
              f"= {n / med(ks[1:])[0] / 1e3:.0f} M rays/s; {int((hits['kind'] == abi.HIT_TRIANGLE).sum())} triangle hits", flush=True)
        if label == "page-locked":
            del r2, hits
            lib.rb_host_free(pr)
            lib.rb_host_free(ph)
    ts = []
    for i in range(200):
        t0 = time.perf_counter()
        e.pick(i % s.width, i % s.height)
        ts.append((time.perf_counter() - t0) * 1e6)
    print(f"pick: median {statistics.median(ts[20:]):.0f} us, min {min(ts[20:]):.0f} us per call (kernel {e.last_query_ms() * 1e3:.0f} us)")
    e.close()


if __name__ == "__main__":
    main()
