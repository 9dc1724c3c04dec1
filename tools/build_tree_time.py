"""Times the reference-layout tree builders (RB_FLAG_BUILD_TREE) on C3, the lamp fixture and C5: rb_bvh_build,
rb_bvh_build_canonical and rb_bvh_build_device on host arrays -- ONE call per build into arrays allocated beforehand, as
bench.py's end_to_end calls rb_bvh_build (best and median of --reps, after one warm-up) --, the engine's own build
(rb_tree_builder ms), and end to end in bench.py's end_to_end pieces twice in the same process: bench.end_to_end itself
(the caller builds the tree with rb_bvh_build) and with the flag (reference_tree_build is zero, create covers create +
upload + the tree).  One JSON line per scene.

    python tools/build_tree_time.py [--scenes c3,lamp,c5] [--spp 32] [--reps 5] [--e2e-reps 3] [--device 0]
"""
import argparse
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import numpy as np  # noqa: E402

import ctypes as C  # noqa: E402

import bench  # noqa: E402
from renderbaby_amd import Engine, RenderConfig, _lib, abi, bvh, refscenes, scenes  # noqa: E402


def _best(fn, reps):
    fn()
    ts = []
    for _ in range(reps):
        t = time.perf_counter()
        fn()
        ts.append((time.perf_counter() - t) * 1e3)
    return min(ts), float(np.median(ts))


def _one_call(fn, prefix, tris):
    """fn(*prefix, tris, n, nodes_out, capacity, &n_nodes, indices_out) with the arrays allocated beforehand: one build per call."""
    n = len(tris)
    nodes = np.zeros(max(bvh.node_count(n), 1), dtype=abi.BVH_NODE)
    idx = np.zeros(max(n, 1), dtype=np.uint32)
    n_nodes = C.c_size_t(0)

    def call():
        rc = fn(*prefix, tris.ctypes.data, n, nodes.ctypes.data, len(nodes), C.byref(n_nodes), idx.ctypes.data)
        assert rc == 0, rc
    return call


def _scene(name, spp):
    if name == "c3":
        return scenes.mesh_c3()
    if name == "c5":
        return scenes.mesh_c5()
    return refscenes.ref_lamp()


def _end_to_end(scene, spp, device, builder):
    scene.uniforms["total_samples"] = spp
    rc = RenderConfig.from_scene(scene, with_tree=False)
    out = {"reference_tree_build_ms": 0.0}
    t = time.perf_counter()
    eng = Engine.new(rc, device=device, build_tree=builder)
    eng.update(rc)
    eng.sync()
    out["create_upload_tree_ms"] = (time.perf_counter() - t) * 1e3
    out["tree"], out["tree_ms"] = eng.tree_builder()
    t = time.perf_counter()
    eng.dispatch(0, 0)
    eng.sync()
    out["prep_ms"] = (time.perf_counter() - t) * 1e3
    out["chunk_tree"], out["chunk_tree_build_ms"] = eng.chunk_tree_builder()
    t = time.perf_counter()
    eng.reserve(spp)
    out["alloc_ms"] = (time.perf_counter() - t) * 1e3
    t = time.perf_counter()
    eng.clear()
    eng.dispatch(0, spp)
    eng.sync()
    out["render_ms"] = (time.perf_counter() - t) * 1e3
    frame = np.zeros((scene.height, scene.width, 4), dtype=np.uint8)
    t = time.perf_counter()
    eng._check(eng._lib.rb_read_rgba(eng._h, frame.ctypes.data))
    out["readback_ms"] = (time.perf_counter() - t) * 1e3
    eng.close()
    out["total_ms"] = sum(out[k] for k in ("create_upload_tree_ms", "prep_ms", "alloc_ms", "render_ms", "readback_ms"))
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--scenes", default="c3,lamp,c5")
    ap.add_argument("--spp", type=int, default=32)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--device", type=int, default=0)
    ap.add_argument("--e2e-reps", type=int, default=3, help="end_to_end runs per leg")
    a = ap.parse_args()
    for name in a.scenes.split(","):
        sc = _scene(name, a.spp)
        tris = np.ascontiguousarray(sc.bvh_triangles, dtype=abi.GPU_TRIANGLE)
        lib = _lib.load()
        rec = {"scene": name, "triangles": int(len(tris)), "fingerprint": _lib.source_fingerprint()}
        rec["rb_bvh_build_ms"] = _best(_one_call(lib.rb_bvh_build, (), tris), a.reps)
        rec["rb_bvh_build_canonical_ms"] = _best(_one_call(lib.rb_bvh_build_canonical, (), tris), a.reps)
        rec["rb_bvh_build_device_ms"] = _best(_one_call(lib.rb_bvh_build_device, (a.device,), tris), a.reps)
        h = bvh.build_canonical(tris)
        d = bvh.build_device(tris, a.device)
        rec["device_equals_host"] = bool(h[0].tobytes() == d[0].tobytes() and np.array_equal(h[1], d[1]))
        for k in range(a.e2e_reps):   # single fresh-engine runs are noisy (first touches, allocations): several, interleaved
            plain = _scene(name, a.spp)
            plain.uniforms["total_samples"] = a.spp
            caller = bench.end_to_end(plain, {}, 0, a.device)[0]   # without the flag: bench.py's own leg
            caller.pop("note", None)
            rec.setdefault("end_to_end_caller", []).append(caller)
            for builder in ("device", "host"):
                rec.setdefault("end_to_end_" + builder, []).append(_end_to_end(_scene(name, a.spp), a.spp, a.device, builder))
        for leg in ("caller", "device", "host"):
            runs = rec["end_to_end_" + leg]
            rec["median_total_ms_" + leg] = float(np.median([r["total_ms"] for r in runs]))
            if leg != "caller":
                rec["median_tree_ms_" + leg] = float(np.median([r["tree_ms"] for r in runs]))
        rec["note"] = ("ms as (best, median) of --reps after a warm-up, one call per build into arrays allocated beforehand; "
                       "rb_bvh_build_device includes its uploads, scratch allocation and read-backs; end_to_end: wall clock per piece "
                       "on a fresh engine, %d spp; end_to_end_caller = bench.end_to_end (caller's rb_bvh_build tree) in the same process" % a.spp)
        print(json.dumps(rec), flush=True)


if __name__ == "__main__":
    main()
