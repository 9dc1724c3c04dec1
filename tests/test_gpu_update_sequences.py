"""One long-lived engine across sequences of partial updates, against the oracle on the scene tests/_update_model.py says the
engine now holds (gpu_wrapper.rs:116-300, :469-495): the frame and the accumulation bit for bit after every step, the tree
and the builders' bookkeeping, and -- where no kept count cuts a buffer short -- the queries and bakes word for word against a
fresh engine that received the merged scene in one Create.  tests/test_update_model.py shows on the oracle alone that every
accepted step of these scripts changes what is seen, so an engine that ignored an update cannot pass.

What the frame does not show is held as well.  The emitter table equals direct.scene_emitters under
the counts in force in every byte after every step, cut short or refused or not, and rb_direct_light on the scene's own
surfels equals the fold of the model in every word; which of the two is the first use after the update alternates.
test_caches_sequence adds the frame history (section 22.2): rb_denoise_history after every step against temporal.py and
denoise.py, through small camera moves, refused updates, a size change and back, and geometry steps.

A failure names (configuration, step index, step name) and what differed: the field the step sent and the structure that is
derived from it (prepared triangles, is_metal / fuzz, sph_scan, a tree, tex_info, a count) is where to look in apply_field,
update_fields, ensure_prepared and accel_params."""
import dataclasses
import functools

import numpy as np
import pytest

from renderbaby_amd import Engine, RenderConfig, RenderError, abi, aov, bvh, denoise, direct, engine, temporal
from renderbaby_amd.engine import Change
from tests import _oracle
from tests import _update_model as M
from tests.test_gpu_direct import model_sums
from tests.test_gpu_query import pixel_centre_rays

pytestmark = pytest.mark.gpu

# name -> (engine options, the base scene is the large one, the engine builds the tree itself)
CONFIGS = {
    "default": (dict(), False, False),
    "reference_walk": (dict(reference_walk=True), False, False),
    "fast_bvh": (dict(fast_bvh=True), False, False),
    "device_bvh": (dict(device_bvh=True), True, False),
    "device_lbvh": (dict(device_lbvh=True), True, False),
    "chunk_tree_host": (dict(chunk_tree="host"), False, False),
    "chunk_tree_device": (dict(chunk_tree="device"), False, False),
    "sphere_tree_host": (dict(sphere_tree="host"), False, False),
    "sphere_tree_device": (dict(sphere_tree="device"), False, False),
    "no_sphere_bvh": (dict(no_sphere_bvh=True), False, False),
    "kernel_queue": (dict(kernel=abi.KERNEL_QUEUE), False, False),
    "kernel_pixel": (dict(kernel=abi.KERNEL_PIXEL), False, False),
    "build_tree_device": (dict(build_tree="device"), False, True),
    "build_tree_host": (dict(build_tree="host"), False, True),
}
SCRIPTS = {"fixed": None, "random1": 1, "random2": 2, "random3": 3}
CACHES_CONFIGS = ["default", "reference_walk", "fast_bvh", "sphere_tree_device", "kernel_queue", "build_tree_device", "build_tree_host"]
N_SURFELS = 130   # two blocks of 64 surfels and a part
SAMPLES, FIRST_SAMPLE = 4, 3


def _u32(a):
    return np.ascontiguousarray(a).view(np.uint32)


def _bytes(a):
    return np.ascontiguousarray(a).view(np.uint8).reshape(-1)


def script_names(script, own_tree):
    if script == "caches":
        return M.caches_script(own_tree)
    return M.fixed_script(own_tree) if script == "fixed" else M.random_script(SCRIPTS[script], 10, own_tree)


# ------------------------------------------------------------------ the reference ---
@functools.lru_cache(maxsize=None)
def reference(script, large, own_tree):
    """The model over a script, once for every engine that runs it: the first scene, then per step
    dict(name, rc, refused, scene, kept, acc, rgba, segments, table) -- the oracle's frame of the scene the model holds after the
    step, and the model's emitter table (direct.scene_emitters) under the counts in force."""
    names = script_names(script, own_tree)

    def rendered(model, **more):
        acc, _, rgba, st = _oracle.render(model.scene, counts_kept=model.kept)
        n_spheres, _, n_triangles = M.effective_counts(model.scene, model.kept)
        table = direct.scene_emitters(model.scene, triangle_count=n_triangles, spheres_count=n_spheres)
        table.flags.writeable = False
        return dict(scene=model.scene, kept=model.kept, acc=_u32(acc), rgba=rgba, segments=st["segments"], table=table, **more)

    first = M.Model(bvh.build_canonical if own_tree else None)
    rc0 = M.create_config(M.base_scene(large), with_tree=not own_tree)
    assert first.apply(rc0) is None
    steps = [rendered(first, name="create", rc=rc0, refused=None)]
    for i, name, rc, why, model in M.run_script(names, script, own_tree, large, bvh.build_canonical):
        assert (why is not None) == (name in M.REFUSED), (i, name, why)
        steps.append(rendered(model, name=name, rc=rc, refused=why))
    return steps


# ------------------------------------------------------------ what is checked ---
def expected_builders(kw, scene, kept):
    """(sphere tree, chunk tree, own tree, reference-layout tree) builders an engine with options `kw` reports for the scene"""
    n_tri = M.effective_counts(scene, kept)[2]
    sphere = ""
    if len(scene.spheres) > 64 and not kw.get("no_sphere_bvh"):                       # built from the buffer, whatever the count
        sphere = "device-median" if kw.get("sphere_tree") == "device" else "host-median"
    own_named = any(kw.get(k) for k in ("fast_bvh", "device_bvh", "device_lbvh"))
    stream = kw.get("kernel", 0) in (0, abi.KERNEL_STREAM)
    takes_tree = not kw.get("reference_walk") and len(scene.bvh_nodes) > 1 and len(scene.bvh_indices) > 0 and n_tri > 0
    chunk = own = ""
    if takes_tree and stream and not own_named:
        chunk = "device" if kw.get("chunk_tree") == "device" else "host"            # (below 16384 slots the host's is the default)
    elif takes_tree and own_named:
        slots = int(sum((scene.bvh_indices[int(n["first_primitive"]):int(n["first_primitive"]) + int(n["primitive_count"])] < n_tri).sum()
                        for n in scene.bvh_nodes if n["primitive_count"] > 0))
        device = (kw.get("device_bvh") or kw.get("device_lbvh")) and slots >= 1024    # fewer slots: the host's builder
        own = ("device-lbvh" if kw.get("device_lbvh") else "device-ploc") if device else "host-sah"
    if kw.get("build_tree"):
        tree = kw["build_tree"] if len(scene.bvh_triangles) else ""
    else:
        tree = "caller" if len(scene.bvh_nodes) else ""
    return sphere, chunk, own, tree


def check_frame(eng, want, where, stats=True):
    if stats:
        eng.reset_stats()
    px = eng.render_current().pixels
    assert px.shape == want["rgba"].shape, (where, "frame size")
    assert np.array_equal(px, want["rgba"]), (where, "pixels differ from the oracle's", int((px != want["rgba"]).any(-1).sum()))
    assert np.array_equal(_u32(eng.read_accumulation()), want["acc"]), (where, "accumulation differs from the oracle's")
    if stats:
        assert eng.stats()["segments"] == want["segments"], (where, "segments")


def check_bookkeeping(eng, kw, want, where):
    scene = want["scene"]
    nodes, idx = eng.tree()
    assert nodes.tobytes() == scene.bvh_nodes.tobytes(), (where, "the tree the engine walks is not the model's")
    assert np.array_equal(idx, scene.bvh_indices if len(scene.bvh_nodes) else scene.bvh_indices[:0]), (where, "bvh_indices")
    got = (eng.sphere_tree_builder()[0], eng.chunk_tree_builder()[0], eng.fast_bvh_builder()[0], eng.tree_builder()[0])
    assert got == expected_builders(kw, scene, want["kept"]), (where, "builders (sphere tree, chunk tree, own tree, tree)",
                                                              len(scene.spheres), len(scene.bvh_triangles), M.effective_counts(scene, want["kept"]))
    census = eng.debug_chunk_tree()                                   # raises where an invariant is broken
    assert (census is not None) == bool(got[1]), (where, "chunk tree census")
    return got


def nothing_cut_short(want):
    s = want["scene"]
    return M.effective_counts(s, want["kept"]) == (len(s.spheres), len(s.bvh_nodes), len(s.bvh_triangles))


def queries(eng, scene, render_first, surfels=None):
    """{name: uint32 words} of the queries and bakes over the frame's pixel-centre rays; `surfels`: the (points, normals) direct
    light is asked for at, by default this engine's own scene_surfels"""
    O, D = pixel_centre_rays(scene)
    O, D = O.reshape(-1, 3), D.reshape(-1, 3)
    out = {}
    hits, surf = eng.cast_rays(O, D, surfaces=True)
    out["cast_rays hits"], out["cast_rays surfaces"] = _u32(hits), _u32(surf)
    with np.errstate(all="ignore"):
        t = hits["t"].astype(np.float32)
        out["occluded 0.99 t"] = eng.occluded(O, D, tmax=(t * np.float32(0.99)).astype(np.float32)).astype(np.uint32)
        out["occluded 1.01 t"] = eng.occluded(O, D, tmax=(t * np.float32(1.01)).astype(np.float32)).astype(np.uint32)
    out["trace_rays"] = _u32(eng.trace_rays(O, D, samples=2))
    s, owners = eng.lightmap_surfels(16, 16)
    out["lightmap surfels"], out["lightmap owners"] = _u32(s), _u32(owners)
    if render_first:
        eng.render_current()
    out["trace_form"] = np.array([eng.trace_form()], np.uint32)      # (a fresh engine derives its facts from one Create)
    out["denoise_guides"] = _u32(eng.denoise_guides())
    out["scene_emitters"] = _bytes(eng.scene_emitters())
    pts, nrm = scene_surfels(eng, scene) if surfels is None else surfels
    if len(pts):
        out["direct_light"] = _u32(eng.direct_light(pts, nrm, SAMPLES, first_sample=FIRST_SAMPLE))
    return out


def scene_surfels(eng, scene, m=N_SURFELS):
    """tests/test_gpu_hemisphere.py's scene_surfels -- the first m hit points of the pixel-centre rays, their normals turned
    towards the camera -- for a scene that may show fewer than m: then what there is"""
    _, pts, nrm = aov.ambient_occlusion_surfels(scene.uniforms, eng.render_hits())
    return np.ascontiguousarray(pts[:m]), np.ascontiguousarray(nrm[:m])


def check_emitters(eng, want, where, sums_first, sums=True):
    """The engine's emitter table against the model's in every byte, and the sums of rb_direct_light on the scene's own surfels
    against direct.fold of the model's contributions under the engine's own any-hit bytes, in every word; `sums_first`: which of
    the two is the first use of the table after the update; without `sums` the table alone.  Returns the surfels, or None."""
    table = want["table"]

    def check_table():
        got = eng.scene_emitters()
        assert got.shape == table.shape and np.array_equal(_bytes(got), _bytes(table)), \
            (where, "emitter table differs from the model's", len(got), len(table), M.effective_counts(want["scene"], want["kept"]))

    def check_sums():
        pts, nrm = scene_surfels(eng, want["scene"])
        if len(pts):
            got = eng.direct_light(pts, nrm, SAMPLES, first_sample=FIRST_SAMPLE)
            model = model_sums(eng, table, pts, nrm, SAMPLES, FIRST_SAMPLE, None, abi.MASK_ALL)[0]
            bad = np.nonzero((_u32(got).reshape(-1, 4) != _u32(model).reshape(-1, 4)).any(1))[0]
            assert len(bad) == 0, (where, "direct light differs from the fold of the model", len(bad), bad[:5], got[bad[:5]], model[bad[:5]])
        return pts, nrm
    if not sums:
        check_table()
        return None
    if sums_first:
        surfels = check_sums()
        check_table()
    else:
        check_table()
        surfels = check_sums()
    return surfels


class HistoryChain:
    """rb_denoise_history across the steps of one engine's life against temporal.py and denoise.py, on
    uint32 views with nothing left out.  `previous` is (F, guides, view) of the last accepted step, None before the first."""

    def __init__(self, eng):
        self.eng, self.previous = eng, None
        self.rp, self.dp = temporal.default_params(), denoise.default_params()
        self.shares, self.geometry = [], []     # (step, name, share of records that carry history), (step, name, carried, rejected)
        self.size_changes = self.refusals = self.plain_first = 0

    @staticmethod
    def same(got, want, where, what):
        bad = np.argwhere((_u32(got) != _u32(want)).any(-1))
        assert got.shape == want.shape and len(bad) == 0, (where, what, len(bad), bad[:4], [got[tuple(b)] for b in bad[:4]], [want[tuple(b)] for b in bad[:4]])

    def size_changed(self, where):
        """an accepted update to another size stands between the history and the next call: there is none to read"""
        with pytest.raises(RenderError):
            self.eng.history()
        assert self.previous is not None, (where, "the size changed without a live history")
        self.size_changes += 1

    def refused(self, where):
        """a refused update changed nothing: the base stayed valid and the call gives the previous step's F again"""
        self.eng.denoise_history(linear=True)
        self.same(self.eng.history(), self.previous[0], where, "F after a refused update")
        self.refusals += 1

    def accepted(self, scene, where, name, plain_first=False):
        eng = self.eng
        if plain_first:
            eng.denoise()                       # the guides are built, and the plane set flipped, by the other entry
            self.plain_first += 1
        out = eng.denoise_history(linear=True)
        F, g, acc = eng.history(), eng.denoise_guides(), eng.read_accumulation()
        view = engine.view_from_camera(scene.uniforms)
        cur = temporal.frame_records(acc)
        carried = self.previous is not None and self.previous[0].shape == F.shape
        if carried:
            Fp, gp, vp = self.previous
            want = temporal.merge(temporal.reproject(Fp, gp, vp, g, self.rp), g, cur)
        else:
            want = cur
        self.same(F, want, where, "F differs from the model's" + ("" if carried else " (no history of this size)"))
        self.same(out, denoise.filter(F, g, self.dp), where, "the filtered frame")
        self.same(eng.denoise_history(linear=True), out, where, "a second call's filtered frame")
        self.same(eng.history(), F, where, "a second call in the same step moved F")
        has = F[..., 3] > acc[..., 3]
        if name == "uniforms_camera_small":
            self.shares.append((where[1], name, float(has.mean())))
        if name.startswith(("triangles_", "own_triangles_")):
            self.geometry.append((where[1], name, int(has.sum()), int(((g["cls"] != 0) & ~has).sum())))
        self.previous = (F, g, view)

    def conditions(self, config):
        """what keeps the chain from passing vacuously"""
        print(config, "share of records with history after uniforms_camera_small:", self.shares, "geometry steps (carried, rejected):", self.geometry)
        assert self.shares and all(share >= 0.3 for _, _, share in self.shares), (config, self.shares)
        assert any(c > 0 and r > 0 for _, _, c, r in self.geometry), (config, self.geometry)
        assert (self.size_changes, self.refusals, self.plain_first) == (2, 2, 1), (config, self.size_changes, self.refusals, self.plain_first)


def check_against_fresh(eng, kw, own_tree, want, where, render_first=True, surfels=None):
    """the long-lived engine's queries word for word against an engine that was just created on the merged scene; both are asked
    for direct light at the same surfels, the long-lived engine's"""
    scene = want["scene"]
    if surfels is None:
        surfels = scene_surfels(eng, scene)
    rc = M.create_config(scene, with_tree=not own_tree)
    fresh = Engine.new(rc, device=0, **kw)
    try:
        fresh.update(rc)
        b = queries(fresh, scene, True, surfels)
    finally:
        fresh.close()
    a = queries(eng, scene, render_first, surfels)
    for name in b:
        assert a[name].shape == b[name].shape and np.array_equal(a[name], b[name]), (where, name, "differs from a fresh engine's: the update left something stale")


def run_sequence(config, script, history=False, sums_every=1):
    """`history`: rb_denoise_history is called after every step's frame and held to the model (HistoryChain); `sums_every`: the
    direct-light sums are held to the model at every step, or at every second one (the table at every step either way)"""
    kw, large, own_tree = CONFIGS[config]
    steps = reference(script, large, own_tree)
    eng = Engine.new(steps[0]["rc"], device=0, stats=True, **kw)
    seen = {}
    try:
        last = last_name = None
        chain = HistoryChain(eng) if history else None
        for i, st in enumerate(steps):
            where = (config, i - 1, st["name"])
            if st["refused"] is not None:
                with pytest.raises(RenderError):
                    eng.update(st["rc"])
                assert st["acc"] is last["acc"] or np.array_equal(st["acc"], last["acc"])      # the model did not move either
                assert np.array_equal(_bytes(st["table"]), _bytes(last["table"]))
            else:
                eng.update(st["rc"])
                if chain and last is not None and st["rgba"].shape != last["rgba"].shape:
                    chain.size_changed(where)
            check_frame(eng, st, where)
            if chain and st["refused"] is not None:
                chain.refused(where)
            elif chain:   # the second of two small camera moves in a row: rb_denoise builds the guides
                chain.accepted(st["scene"], where, st["name"], plain_first=st["name"] == last_name == "uniforms_camera_small")
            got = check_bookkeeping(eng, kw, st, where)
            # every step, cut short or not, refused or not; which call is the first use of the table alternates
            surfels = check_emitters(eng, st, where, sums_first=(i // sums_every) % 2 == 0, sums=i % sums_every == 0)
            if st["refused"] is None:
                if nothing_cut_short(st):
                    check_against_fresh(eng, kw, own_tree, st, where, surfels=surfels)
                last = st
            last_name = st["name"]
            s = st["scene"]
            seen.setdefault(got, set()).add((len(s.spheres), len(s.bvh_triangles)))
        if large:   # the device builders of the library's own tree were what ran where the config asked for them
            assert any(own.startswith("device-") for _, _, own, _ in seen), (config, seen)
        if chain:
            chain.conditions(config)
    finally:
        eng.close()
    return len(steps) - 1, seen


@pytest.mark.parametrize("script", sorted(SCRIPTS))
@pytest.mark.parametrize("config", sorted(CONFIGS))
def test_update_sequence(config, script):
    run_sequence(config, script, sums_every=2)   # (the sums at every step cost some of these cases half again their time)


@pytest.mark.parametrize("config", CACHES_CONFIGS)
def test_caches_sequence(config):
    """M.caches_script: the emitter table through emissive spheres, kept counts, dark lights and the colour hash, and the frame
    history through small camera moves, refused updates, a size change and back, and a geometry step
    (tests/test_update_model.py holds the script to what it must show)."""
    run_sequence(config, "caches", history=True)


# ------------------------------------------------- updates between iterator frames ---
ITERATOR_STEPS = {"meshes": "meshes_swap_metal", "uvs": "uvs_new_values", "textures": "textures_other", "lights": "lights_more",
                  "triangles": "triangles_shrink", "nodes+indices": "tree_swap"}


@pytest.mark.parametrize("passes_per_frame", [1, 3])
@pytest.mark.parametrize("field", sorted(ITERATOR_STEPS))
def test_update_between_iterator_frames(field, passes_per_frame):
    """One frame of an iterator, then the field alone is updated and the iterator restarted: the pass that was started ahead on
    the old scene is dropped, every delivered frame is the oracle's for the new scene."""
    base = M.base_scene().with_params(spp=4)
    model = M.Model()
    rc0 = M.create_config(base)
    assert model.apply(rc0) is None
    rc1 = M.STEPS[ITERATOR_STEPS[field]](model.scene, M.script_rng("iterator " + field))
    eng = Engine.new(rc0, device=0)
    try:
        it = eng.frame_iterator(rc0, passes_per_frame)
        assert np.array_equal(it.next().pixels, _oracle.render(base, 0, passes_per_frame)[2]), field
        assert model.apply(rc1) is None
        eng.update(rc1)
        rc2 = RenderConfig(uniforms=Change.update(M._uniforms(model.scene)))
        assert model.apply(rc2) is None
        frames = [f.pixels.copy() for f in eng.frame_iterator(rc2, passes_per_frame)]
        upto = list(range(passes_per_frame, 4, passes_per_frame)) + [4]
        assert len(frames) == len(upto)
        for frame, n in zip(frames, upto):
            assert np.array_equal(frame, _oracle.render(model.scene, 0, n, counts_kept=model.kept)[2]), (field, passes_per_frame, n)
    finally:
        eng.close()


# --------------------------------------------------- the multi-device handle, shards ---
def test_first_steps_on_a_multi_device_handle():
    steps = reference("fixed", False, False)[:9]
    eng = Engine.new(steps[0]["rc"], devices=[0, 0], gather_peer_copy=True)
    try:
        for i, st in enumerate(steps):
            where = ("devices=[0, 0]", i - 1, st["name"])
            if st["refused"] is not None:
                with pytest.raises(RenderError):
                    eng.update(st["rc"])
            else:
                eng.update(st["rc"])
            assert np.array_equal(eng.render_current().pixels, st["rgba"]), where
    finally:
        eng.close()


def test_first_steps_on_two_shards():
    steps = reference("fixed", False, False)[:9]
    ranks = [Engine.new(steps[0]["rc"], device=0, shard_rank=r, shard_count=2, stripe_rows=4) for r in range(2)]
    try:
        for i, st in enumerate(steps):
            h = st["rgba"].shape[0]
            covered = np.zeros(h, np.int32)
            for r, eng in enumerate(ranks):
                where = (f"shard {r} of 2", i - 1, st["name"])
                if st["refused"] is not None:
                    with pytest.raises(RenderError):
                        eng.update(st["rc"])
                else:
                    eng.update(st["rc"])
                px = eng.render_current().pixels
                acc = _u32(eng.read_accumulation())
                owned, padded = eng.local_rows()
                assert px.shape[0] == padded
                for lr in range(padded):
                    g = eng.global_row(lr)
                    if g < h:
                        covered[g] += 1
                        assert np.array_equal(px[lr], st["rgba"][g]), (where, "row", g)
                        assert np.array_equal(acc[lr], st["acc"][g]), (where, "accumulation row", g)
                assert (np.array([eng.global_row(lr) for lr in range(padded)]) < h).sum() == owned
            assert (covered == 1).all(), (i, st["name"])
    finally:
        for eng in ranks:
            eng.close()


# ------------------------------------------ a query as the first use after an update ---
@pytest.mark.parametrize("step", ["triangles_shrink", "uvs_new_values"])
@pytest.mark.parametrize("config", ["default", "fast_bvh", "build_tree_device"])
def test_a_query_is_the_first_use_after_an_update(config, step):
    """No render between the update and the queries: ensure_prepared is reached from the query path alone."""
    kw, large, own_tree = CONFIGS[config]
    model = M.Model(bvh.build_canonical if own_tree else None)
    rc0 = M.create_config(M.base_scene(large), with_tree=not own_tree)
    assert model.apply(rc0) is None
    rc1 = M.STEPS[step](model.scene, M.script_rng("query first " + step))
    eng = Engine.new(rc0, device=0, **kw)
    try:
        eng.update(rc0)
        eng.render_current()                         # everything prepared for the first scene
        assert model.apply(rc1) is None
        eng.update(rc1)
        scene = model.scene
        fresh_rc = M.create_config(scene, with_tree=not own_tree)
        fresh = Engine.new(fresh_rc, device=0, **kw)
        try:
            fresh.update(fresh_rc)
            O, D = (a.reshape(-1, 3) for a in pixel_centre_rays(scene))
            want = fresh.cast_rays(O, D, surfaces=True) + fresh.lightmap_surfels(16, 16)
        finally:
            fresh.close()
        if step == "triangles_shrink":
            got = eng.cast_rays(O, D, surfaces=True) + eng.lightmap_surfels(16, 16)
        else:
            got = eng.lightmap_surfels(16, 16) + eng.cast_rays(O, D, surfaces=True)
            got = got[2:] + got[:2]
        for name, a, b in zip(("cast_rays hits", "cast_rays surfaces", "lightmap surfels", "lightmap owners"), got, want):
            assert np.array_equal(_u32(a), _u32(b)), (config, step, name)
    finally:
        eng.close()


# ------------------------------------------------------ the engine's clamp, pinned ---
def test_a_kept_count_above_the_buffer_is_clamped_to_its_length():
    """The reference leaves a Keep count above the buffer's length to WGSL's robust access.  The engine clamps the count to the
    length (patch_count): the frame is that of the whole buffers, and the trees built for the whole buffers stay in use."""
    base = M.base_scene()
    sp = M.make_spheres(70, 5)
    rc0 = M.create_config(base)
    eng = Engine.new(rc0, device=0, stats=True)
    try:
        eng.update(rc0)
        u = M._uniforms(base)
        eng.update(RenderConfig(uniforms=Change.update(u), spheres=Change.update(sp)))
        whole = eng.render_current().pixels.copy()
        u2 = u.copy()
        u2["spheres_count"], u2["bvh_node_count"], u2["bvh_triangle_count"] = 70 + 7, len(base.bvh_nodes) + 3, len(base.bvh_triangles) + 100
        eng.update(RenderConfig(uniforms=Change.update(u2)))
        assert np.array_equal(eng.render_current().pixels, whole)
        assert np.array_equal(whole, _oracle.render(dataclasses.replace(base, spheres=sp))[2])
        assert eng.sphere_tree_builder()[0] == "host-median" and eng.chunk_tree_builder()[0] == "host"
    finally:
        eng.close()
