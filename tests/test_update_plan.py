"""What an rb_update decides before a buffer is touched (renderbaby_amd/csrc/rb_update_plan.hpp): the field table, plan_update,
the commit functions, patch_count and shard_layout.  Host code with no HIP in it, so it is compiled, together with rb_bvh.cpp,
into a stand-alone program under AddressSanitizer and UBSan and run on the host; no GPU, and nothing is loaded into Python.

Three parts.  Worked refusals: for every refusal of the planner one config that reaches it, code and complete text (the texts
are those of rb_runtime.cpp before the planner existed), and for configs that break two rules the one that has always fired
first.  (One site is out of reach: "too many triangles" of an engine that walks the caller's tree comes after the pass over
2^31 triangles for the largest mesh index; an engine that builds the tree says the same before it reads one.)  The replay:
tests/_update_model.py's scripts, and a list of refused steps of this file's own, are run through ``Model`` here and written
to a file, config by config with what the model says of each; the program replays them on a SceneFacts with plan_update and
the commit functions alone and must agree on refusal, actions, lengths and the three patched counts.  The sweep of
shard_layout: every row of a sharded frame belongs to exactly one rank."""
import os
import re
import struct
import subprocess
import textwrap

from renderbaby_amd import abi, bvh
from renderbaby_amd.engine import Change, RenderConfig
from tests import _update_model as M

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "renderbaby_amd", "csrc")

# ---- the model's reasons (digits -> N) and the RB_ERR_* each stands for; None: several codes, refusal only
with open(os.path.join(ROOT, "include", "rb_abi.h")) as _h:
    ERR = {name: int(value) for name, value in re.findall(r"\bRB_(ERR_\w+) = (\d+)", _h.read())}
REASON_CODE = {
    **{f"first update: {f} is not Create": ERR[f"ERR_INVALID_{f.upper()}"] for f in ("uniforms", "spheres", "uvs", "meshes", "lights", "textures")},
    "uniforms cannot be deleted": ERR["ERR_CANNOT_DELETE_NONEXISTENT"],
    "pane out of bounds": None,   # RB_ERR_PANE_DISTANCE_OUT_OF_BOUNDS or RB_ERR_PANE_WIDTH_OUT_OF_BOUNDS
    "camera direction is zero": ERR["ERR_INVALID_CAMERA_DIRECTION"],
    "spheres: a radius is not positive": ERR["ERR_INVALID_SPHERES"],
    "lights: a radius is not positive": ERR["ERR_INVALID_LIGHTS"],
    "uvs: odd length": ERR["ERR_INVALID_UVS"],
    **{f"{f}: Delete is not implemented": ERR["ERR_UNSUPPORTED_DELETE"] for f in M.NO_DELETE},
    "the engine builds the tree itself: bvh_nodes and bvh_indices must be Keep": ERR["ERR_INVALID_BVH"],
    "node N is reachable twice": ERR["ERR_INVALID_BVH"],
    "leaf N lies past the indices": ERR["ERR_INVALID_BVH"],
    "a triangle's mesh does not exist": ERR["ERR_INVALID_MESHES"],
    "a texture is empty": ERR["ERR_INVALID_TEXTURES"],
}


def reason_class(why):
    return re.sub(r"\d+", "N", why)


# ---- steps of this test's own, all refused: the reasons the scripts of tests/_update_model.py do not reach
def _camera(scene, **kw):
    u = M._uniforms(scene)
    for k, v in kw.items():
        u["camera"][k] = v
    return M._rc(scene, uniforms=u)


def _bad_radius(field):
    def step(scene):
        a = getattr(scene, field).copy()
        a["radius"][len(a) // 2] = 0.0
        return M._rc(scene, **{field: a})
    return step


def extra_steps():
    """the configs of one more engine: six first configs that do not create a field, the base scene, then refusals of validate"""
    s = M.base_scene()

    def first(**over):
        rc = M.create_config(s)
        for k, v in over.items():
            setattr(rc, k, v)
        return lambda scene: rc
    return [first(uniforms=Change.update(s.uniforms)), first(spheres=Change.keep()), first(uvs=Change.update(s.uvs)), first(meshes=Change.delete()),
            first(lights=Change.update(s.lights)), first(textures=Change.keep()), first(),
            lambda scene: RenderConfig(uniforms=Change.delete()),
            lambda scene: _camera(scene, pane_distance=100.5), lambda scene: _camera(scene, pane_width=-1.0),
            lambda scene: _camera(scene, dir=(0.0, 0.0, 0.0)), _bad_radius("spheres"), _bad_radius("lights"),
            *[(lambda scene, f=f: M._rc(scene, **{f: Change.delete()})) for f in M.NO_DELETE]]


def script_steps(names, script_id, own):
    rng = M.script_rng(script_id)
    first = M.create_config(M.base_scene(), with_tree=not own)
    return [lambda scene: first] + [(lambda scene, n=n: M.STEPS[n](scene, rng)) for n in names]


# ---- the file the program replays
def _field_bytes(f, ch):
    if ch.tag not in (abi.CREATE, abi.UPDATE):
        return struct.pack("<IQ", ch.tag, 0)
    if f == "textures":
        texs = M._textures(ch.value)
        return struct.pack("<IQ", ch.tag, len(texs)) + b"".join(struct.pack("<IIQ", w, h, len(d)) + d.astype("<u4").tobytes() for w, h, d in texs)
    a = M._array(f, ch.value)
    return struct.pack("<IQ", ch.tag, a.size) + a.tobytes()


def record(out, own, steps, seen, seen_steps):
    """one engine: every step's config and the model's word on it"""
    model = M.Model(bvh.build_canonical if own else None)
    out.append(struct.pack("<II", int(own), len(steps)))
    for step in steps:
        rc = step(model.scene)
        acts = [{None: 0, "take": 1, "delete": 2}[model._action(f, getattr(rc, f).tag)] for f in M.FIELDS]
        acts[0] = int(rc.uniforms.tag == (abi.UPDATE if model.initialized else abi.CREATE))
        why = model.apply(rc)
        seen_steps[0] += 1
        seen_steps[1] += why is not None
        out.append(b"".join(_field_bytes(f, getattr(rc, f)) for f in M.FIELDS))
        if why is not None:
            seen.add(reason_class(why))
            assert reason_class(why) in REASON_CODE, why
            out.append(struct.pack("<Ii", 1, REASON_CODE[reason_class(why)] or 0))
            continue
        lens = [len(getattr(model.scene, f)) for f in M.FIELDS[1:]]
        out.append(struct.pack("<Ii9I8II3I", 0, 0, *acts, *lens, model.kept, *M.effective_counts(model.scene, model.kept)))


def write_replay(path):
    out, seen, engines, seen_steps = [], set(), 0, [0, 0]   # steps, refused ones
    for own in (False, True):
        scripts = [("fixed", M.fixed_script(own))] + [(f"random{seed}", M.random_script(seed, 10, own)) for seed in (1, 2, 3, 4, 5)]
        for script_id, names in scripts:
            record(out, own, script_steps(names, script_id, own), seen, seen_steps)
            engines += 1
    record(out, False, extra_steps(), seen, seen_steps)
    assert seen == set(REASON_CODE), (sorted(set(REASON_CODE) - seen), sorted(seen - set(REASON_CODE)))   # every reason Model.refusal has
    with open(path, "wb") as f:
        f.write(struct.pack("<3I", engines + 1, *seen_steps) + b"".join(out))


SRC = textwrap.dedent(r'''
    #include <cmath>
    #include <cstdio>
    #include <cstring>
    #include <fstream>
    #include <iterator>
    #include <string>
    #include <vector>
    #include "rb_update_plan.hpp"
    using namespace rb;
    static int failures = 0;
    static std::string g_what;
    static void fail(int line, const char* text, const std::string& more = "") {
        if (failures++ < 20) std::printf("line %d: %s   [%s] %s\n", line, text, g_what.c_str(), more.c_str());
    }
    #define CHECK(c) do { if (!(c)) fail(__LINE__, #c); } while (0)

    static bool same(const SceneFacts& a, const SceneFacts& b) {
        const uint32_t x[] = {a.initialized, a.have_uniforms, a.n_spheres, a.n_lights, a.n_meshes, a.n_nodes, a.n_indices, a.n_tris, a.n_uvs, a.n_tex,
                              a.last_change_spheres, a.last_change_nodes, a.last_change_tris, a.last_spheres_sent, a.bvh_stack, a.max_mesh_index,
                              a.width, a.height, a.local_rows, a.padded_rows, a.own_tree, a.shard_rank, a.shard_count, a.stripe_rows};
        const uint32_t y[] = {b.initialized, b.have_uniforms, b.n_spheres, b.n_lights, b.n_meshes, b.n_nodes, b.n_indices, b.n_tris, b.n_uvs, b.n_tex,
                              b.last_change_spheres, b.last_change_nodes, b.last_change_tris, b.last_spheres_sent, b.bvh_stack, b.max_mesh_index,
                              b.width, b.height, b.local_rows, b.padded_rows, b.own_tree, b.shard_rank, b.shard_count, b.stripe_rows};
        return !std::memcmp(x, y, sizeof x) && !std::memcmp(&a.uniforms, &b.uniforms, sizeof a.uniforms) && a.host_nodes.size() == b.host_nodes.size() &&
               (a.host_nodes.empty() || !std::memcmp(a.host_nodes.data(), b.host_nodes.data(), a.host_nodes.size() * sizeof(rb_bvh_node)));
    }

    // a config that owns its arrays
    struct Scene {
        std::vector<rb_uniforms> uniforms;
        std::vector<rb_sphere> spheres;
        std::vector<float> uvs;
        std::vector<rb_mesh> meshes;
        std::vector<rb_point_light> lights;
        std::vector<rb_bvh_node> nodes;
        std::vector<uint32_t> indices;
        std::vector<rb_gpu_triangle> tris;
        std::vector<rb_texture> textures;
        std::vector<std::vector<uint32_t>> texels;
        rb_config cfg{};
        void point(uint32_t tag) {   // every field `tag`, pointing at the arrays
            cfg.uniforms = {tag, uniforms.data(), uniforms.size()}, cfg.spheres = {tag, spheres.data(), spheres.size()}, cfg.uvs = {tag, uvs.data(), uvs.size()};
            cfg.meshes = {tag, meshes.data(), meshes.size()}, cfg.lights = {tag, lights.data(), lights.size()}, cfg.bvh_nodes = {tag, nodes.data(), nodes.size()};
            cfg.bvh_indices = {tag, indices.data(), indices.size()}, cfg.bvh_triangles = {tag, tris.data(), tris.size()};
            for (size_t i = 0; i < textures.size(); i++) textures[i].rgba_data = texels[i].data();
            cfg.textures = {tag, textures.data(), textures.size()};
        }
    };

    // what the engine does with an accepted plan, the device left out
    static void commit_all(SceneFacts& sc, const UpdatePlan& pl, const rb_config* cfg) {
        for (uint32_t f = 0; f < kFieldCount; f++) commit_field(sc, pl, cfg, (Field)f);
        if (pl.own_tree != OwnTree::Keep) {
            const size_t n = pl.own_tree == OwnTree::Rebuild ? cfg->bvh_triangles.count : 0;
            TreeSkeleton sk;
            bvh_skeleton(n, sk);
            commit_own_tree(sc, std::move(sk.nodes), n);
        }
        commit_end(sc, pl);
    }

    // ------------------------------------------------------------------ worked refusals ---
    static Scene small() {
        Scene s;
        rb_uniforms u{};
        u.width = 8, u.height = 8, u.total_samples = 1, u.camera.pane_distance = 1.0f, u.camera.pane_width = 1.0f, u.camera.dir[2] = -1.0f, u.max_depth = 2;
        s.uniforms = {u};
        rb_sphere sp{};
        sp.radius = 1.0f;
        s.spheres = {sp, sp};
        s.uvs = {0.0f, 1.0f};
        s.meshes = {rb_mesh{}};
        rb_point_light l{};
        l.radius = 1.0f;
        s.lights = {l};
        rb_bvh_node leaf{};
        leaf.primitive_count = 1;
        s.nodes = {leaf};
        s.indices = {0u};
        rb_gpu_triangle t{};
        t.v1[0] = 1.0f, t.v2[1] = 1.0f;
        s.tris = {t};
        s.textures = {rb_texture{1, 1, nullptr}};
        s.texels = {{0xFFFFFFFFu}};
        return s;
    }
    static std::vector<rb_bvh_node> cyclic() {   // 1's children are the root
        std::vector<rb_bvh_node> n(3, rb_bvh_node{});
        n[0].left = 1, n[0].right = 2, n[2].primitive_count = 1;
        return n;
    }
    static void expect(int line, const SceneFacts& sc, const rb_config* cfg, int code, const char* text) {
        UpdatePlan pl;
        std::string why;
        const SceneFacts before = sc;
        const int rc = plan_update(sc, cfg, pl, why);
        if (rc != code || why != text) fail(line, text, "got " + std::to_string(rc) + " '" + why + "'");
        if (!same(sc, before)) fail(line, "a refusal changed the facts");
    }
    #define REFUSED(sc, s, code, text) do { expect(__LINE__, sc, &(s).cfg, code, text); } while (0)

    static void worked_refusals() {
        g_what = "worked refusals";
        SceneFacts fresh, live, own_fresh, own_live;
        own_fresh.own_tree = own_live.own_tree = true;
        {
            Scene s = small();
            s.point(RB_CREATE);
            UpdatePlan pl;
            std::string why;
            CHECK(plan_update(live, &s.cfg, pl, why) == RB_OK);
            commit_all(live, pl, &s.cfg);
            CHECK(live.initialized && live.have_uniforms && live.n_spheres == 2 && live.n_nodes == 1 && live.n_indices == 1 && live.n_tex == 1 && live.bvh_stack == 1);
            s.cfg.bvh_nodes = s.cfg.bvh_indices = rb_field{RB_KEEP, nullptr, 0};
            CHECK(plan_update(own_live, &s.cfg, pl, why) == RB_OK && pl.own_tree == OwnTree::Rebuild);
            commit_all(own_live, pl, &s.cfg);
            CHECK(own_live.n_nodes == 1 && own_live.n_indices == 1 && own_live.last_change_nodes == RB_CREATE);
        }
        // ---- tags, pointers, the uniforms' count
        expect(__LINE__, fresh, nullptr, RB_ERR_NULL_ARGUMENT, "config is NULL");
        { Scene s = small(); s.point(RB_UPDATE); s.cfg.lights.change = 4; REFUSED(live, s, RB_ERR_NULL_ARGUMENT, "lights: bad change tag 4"); }
        { Scene s = small(); s.point(RB_UPDATE); s.cfg.bvh_indices.ptr = nullptr; REFUSED(live, s, RB_ERR_NULL_ARGUMENT, "bvh_indices: count 1 with NULL pointer"); }
        { Scene s = small(); s.uniforms.push_back(s.uniforms[0]); s.point(RB_UPDATE); REFUSED(live, s, RB_ERR_INVALID_UNIFORMS, "uniforms: expected exactly one rb_uniforms, got 2"); }
        // ---- the first config creates six fields
        { Scene s = small(); s.point(RB_CREATE); s.cfg.uniforms.change = RB_UPDATE; REFUSED(fresh, s, RB_ERR_INVALID_UNIFORMS, "Invalid Uniforms"); }
        { Scene s = small(); s.point(RB_CREATE); s.cfg.spheres.change = RB_KEEP; REFUSED(fresh, s, RB_ERR_INVALID_SPHERES, "Invalid Spheres"); }
        { Scene s = small(); s.point(RB_CREATE); s.cfg.uvs.change = RB_DELETE; REFUSED(fresh, s, RB_ERR_INVALID_UVS, "Invalid UVs"); }
        { Scene s = small(); s.point(RB_CREATE); s.cfg.meshes.change = RB_UPDATE; REFUSED(fresh, s, RB_ERR_INVALID_MESHES, "Invalid Meshes"); }
        { Scene s = small(); s.point(RB_CREATE); s.cfg.lights.change = RB_KEEP; REFUSED(fresh, s, RB_ERR_INVALID_LIGHTS, "Invalid Lights"); }
        { Scene s = small(); s.point(RB_CREATE); s.cfg.textures.change = RB_UPDATE; REFUSED(fresh, s, RB_ERR_INVALID_TEXTURES, "Invalid Textures"); }
        // ---- later configs: values and refused Deletes
        { Scene s = small(); s.uniforms[0].camera.pane_distance = 100.5f; s.point(RB_UPDATE); REFUSED(live, s, RB_ERR_PANE_DISTANCE_OUT_OF_BOUNDS, "Pane-Distance is out of bounds"); }
        { Scene s = small(); s.uniforms[0].camera.pane_distance = NAN; s.point(RB_UPDATE); REFUSED(live, s, RB_ERR_PANE_DISTANCE_OUT_OF_BOUNDS, "Pane-Distance is out of bounds"); }
        { Scene s = small(); s.uniforms[0].camera.pane_width = 1000.5f; s.point(RB_UPDATE); REFUSED(live, s, RB_ERR_PANE_WIDTH_OUT_OF_BOUNDS, "Pane-Distance is out of bounds"); }
        { Scene s = small(); s.uniforms[0].camera.dir[2] = 0.0f; s.point(RB_UPDATE); REFUSED(live, s, RB_ERR_INVALID_CAMERA_DIRECTION, "Invalid camera direction"); }
        { Scene s = small(); s.point(RB_UPDATE); s.cfg.uniforms.change = RB_DELETE; REFUSED(live, s, RB_ERR_CANNOT_DELETE_NONEXISTENT, "Cannot delete none existent"); }
        { Scene s = small(); s.spheres[1].radius = 0.0f; s.point(RB_UPDATE); REFUSED(live, s, RB_ERR_INVALID_SPHERES, "Invalid Spheres"); }
        { Scene s = small(); s.uvs.push_back(0.5f); s.point(RB_UPDATE); REFUSED(live, s, RB_ERR_INVALID_UVS, "Invalid UVs"); }
        { Scene s = small(); s.point(RB_UPDATE); s.cfg.uvs.change = RB_DELETE; REFUSED(live, s, RB_ERR_UNSUPPORTED_DELETE, "not yet implemented: Implement UVs Deletion"); }
        { Scene s = small(); s.point(RB_UPDATE); s.cfg.meshes.change = RB_DELETE; REFUSED(live, s, RB_ERR_UNSUPPORTED_DELETE, "not yet implemented: Implement meshes Deletion"); }
        { Scene s = small(); s.lights[0].radius = -1.0f; s.point(RB_UPDATE); REFUSED(live, s, RB_ERR_INVALID_LIGHTS, "Invalid Lights"); }
        { Scene s = small(); s.point(RB_UPDATE); s.cfg.lights.change = RB_DELETE; REFUSED(live, s, RB_ERR_UNSUPPORTED_DELETE, "not yet implemented: Implement lights Deletion"); }
        { Scene s = small(); s.point(RB_UPDATE); s.cfg.textures.change = RB_DELETE; REFUSED(live, s, RB_ERR_UNSUPPORTED_DELETE, "not yet implemented: Implement textures Deletion"); }
        // ---- the scene the update would leave: the tree
        const char* own_keep = "the engine builds the tree itself (RB_FLAG_BUILD_TREE): bvh_nodes and bvh_indices must be Keep";
        { Scene s = small(); s.point(RB_UPDATE); REFUSED(own_live, s, RB_ERR_INVALID_BVH, own_keep); }
        { Scene s = small(); s.point(RB_CREATE); s.cfg.bvh_nodes.change = RB_KEEP; REFUSED(own_fresh, s, RB_ERR_INVALID_BVH, own_keep); }
        for (const SceneFacts* sc : {&own_live, &own_fresh}) {
            Scene s = small();
            s.point(sc->initialized ? RB_UPDATE : RB_CREATE);
            s.cfg.bvh_nodes = s.cfg.bvh_indices = rb_field{RB_KEEP, nullptr, 0};
            s.cfg.bvh_triangles.count = 1ull << 31;   // refused before one is read
            REFUSED(*sc, s, RB_ERR_INVALID_BVH, "too many triangles");
            s.tris.push_back(s.tris[0]);
            s.tris[1].v1[1] = INFINITY;
            s.cfg.bvh_triangles = {s.cfg.bvh_triangles.change, s.tris.data(), 2};
            REFUSED(*sc, s, RB_ERR_INVALID_BVH, "triangle 1 has a non-finite vertex coordinate");
        }
        { Scene s = small(); s.point(RB_UPDATE); s.cfg.bvh_nodes.count = 1ull << 31; REFUSED(live, s, RB_ERR_INVALID_BVH, "too many BVH nodes"); }
        { Scene s = small(); s.point(RB_UPDATE); s.cfg.bvh_indices.count = 1ull << 31; REFUSED(live, s, RB_ERR_INVALID_BVH, "too many BVH indices"); }
        { Scene s = small(); s.nodes = cyclic(); s.point(RB_UPDATE); REFUSED(live, s, RB_ERR_INVALID_BVH, "BVH node 0 is reachable twice (cycle or shared child)"); }
        {   // 40 inner nodes in a chain down the right children, each with a leaf on the left: popped at occupancies 1, 2, ..
            Scene s = small();
            s.nodes.assign(81, rb_bvh_node{});
            for (uint32_t k = 0; k < 40; k++) s.nodes[k].left = 40 + k, s.nodes[k].right = k < 39 ? k + 1 : 80;
            for (uint32_t k = 40; k < 81; k++) s.nodes[k].primitive_count = 1;
            s.point(RB_UPDATE);
            REFUSED(live, s, RB_ERR_INVALID_BVH, "BVH traversal needs a stack of 41 entries; kernels provide 32");
        }
        { Scene s = small(); s.nodes[0].primitive_count = 5; s.point(RB_UPDATE); REFUSED(live, s, RB_ERR_INVALID_BVH, "leaf 0 covers [0, +5) of 1 bvh_indices"); }
        {   // new nodes against the kept indices
            Scene s = small(); s.point(RB_KEEP); s.nodes[0].first_primitive = 1;
            s.cfg.bvh_nodes = {RB_UPDATE, s.nodes.data(), 1};
            REFUSED(live, s, RB_ERR_INVALID_BVH, "leaf 0 covers [1, +1) of 1 bvh_indices");
        }
        // ---- meshes, textures, the frame
        { Scene s = small(); s.tris[0].mesh_index = 9; s.point(RB_UPDATE); REFUSED(live, s, RB_ERR_INVALID_MESHES, "a triangle references mesh 9 of 1"); }
        { Scene s = small(); s.point(RB_KEEP); s.meshes.clear(); s.cfg.meshes = {RB_UPDATE, nullptr, 0}; REFUSED(live, s, RB_ERR_INVALID_MESHES, "a triangle references mesh 0 of 0"); }
        { Scene s = small(); s.textures.push_back(rb_texture{4, 0, nullptr}); s.texels.push_back({0u}); s.point(RB_UPDATE); REFUSED(live, s, RB_ERR_INVALID_TEXTURES, "texture 1 is empty"); }
        { Scene s = small(); s.point(RB_UPDATE); s.textures[0].rgba_data = nullptr; REFUSED(live, s, RB_ERR_INVALID_TEXTURES, "texture 0 has no data"); }
        { Scene s = small(); s.uniforms[0].width = 65536, s.uniforms[0].height = 32768; s.point(RB_UPDATE); REFUSED(live, s, RB_ERR_INVALID_UNIFORMS, "frame of 65536 x 32768 pixels is too large"); }
        {   // a shard's buffer is what counts: two ranks halve it
            SceneFacts half = live;
            half.shard_count = 2;
            Scene s = small(); s.uniforms[0].width = 65536, s.uniforms[0].height = 32768; s.point(RB_UPDATE);
            UpdatePlan pl;
            std::string why;
            CHECK(plan_update(half, &s.cfg, pl, why) == RB_OK && pl.resize && pl.frame.padded == 16384);
        }
        // ---- two rules broken at once: the one that has always fired first
        {   // tags and pointers of all fields before the uniforms' count
            Scene s = small(); s.uniforms.push_back(s.uniforms[0]); s.point(RB_UPDATE); s.cfg.textures.ptr = nullptr;
            REFUSED(live, s, RB_ERR_NULL_ARGUMENT, "textures: count 1 with NULL pointer");
        }
        {   // tags before values
            Scene s = small(); s.uniforms[0].camera.pane_distance = -1.0f; s.point(RB_UPDATE); s.cfg.textures.change = 7;
            REFUSED(live, s, RB_ERR_NULL_ARGUMENT, "textures: bad change tag 7");
        }
        {   // the uniforms' count before the first config's Creates
            Scene s = small(); s.uniforms.push_back(s.uniforms[0]); s.point(RB_CREATE); s.cfg.spheres.change = RB_KEEP;
            REFUSED(fresh, s, RB_ERR_INVALID_UNIFORMS, "uniforms: expected exactly one rb_uniforms, got 2");
        }
        {   // values in the order of the fields: the spheres' before the refused Delete of the uvs, that before the lights'
            Scene s = small(); s.spheres[0].radius = -1.0f; s.lights[0].radius = 0.0f; s.point(RB_UPDATE); s.cfg.uvs.change = RB_DELETE;
            REFUSED(live, s, RB_ERR_INVALID_SPHERES, "Invalid Spheres");
            s.spheres[0].radius = 1.0f;
            REFUSED(live, s, RB_ERR_UNSUPPORTED_DELETE, "not yet implemented: Implement UVs Deletion");
        }
        { Scene s = small(); s.lights[0].radius = -1.0f; s.nodes = cyclic(); s.point(RB_UPDATE); REFUSED(live, s, RB_ERR_INVALID_LIGHTS, "Invalid Lights"); }   // values before the tree
        { Scene s = small(); s.nodes = cyclic(); s.point(RB_CREATE); s.cfg.spheres.change = RB_KEEP; REFUSED(fresh, s, RB_ERR_INVALID_SPHERES, "Invalid Spheres"); }   // and the first config's Creates
        { Scene s = small(); s.lights[0].radius = -1.0f; s.point(RB_UPDATE); REFUSED(own_live, s, RB_ERR_INVALID_LIGHTS, "Invalid Lights"); }   // ... also before "must be Keep"
        { Scene s = small(); s.nodes = cyclic(); s.tris[0].mesh_index = 9; s.point(RB_UPDATE); REFUSED(live, s, RB_ERR_INVALID_BVH, "BVH node 0 is reachable twice (cycle or shared child)"); }   // the tree before the meshes
        { Scene s = small(); s.nodes[0].primitive_count = 5; s.tris[0].mesh_index = 9; s.point(RB_UPDATE); REFUSED(live, s, RB_ERR_INVALID_BVH, "leaf 0 covers [0, +5) of 1 bvh_indices"); }
        { Scene s = small(); s.tris[0].mesh_index = 9; s.textures[0].width = 0; s.point(RB_UPDATE); REFUSED(live, s, RB_ERR_INVALID_MESHES, "a triangle references mesh 9 of 1"); }   // the meshes before the textures
        {   // the textures before the frame
            Scene s = small(); s.textures[0].height = 0; s.uniforms[0].width = 65536, s.uniforms[0].height = 32768; s.point(RB_UPDATE);
            REFUSED(live, s, RB_ERR_INVALID_TEXTURES, "texture 0 is empty");
        }
        // ---- and what is no refusal: the colour hash reads no mesh; the first update acts on Create alone
        { Scene s = small(); s.tris[0].mesh_index = 9; s.uniforms[0].color_hash_enabled = 1; s.point(RB_UPDATE); UpdatePlan pl; std::string why; CHECK(plan_update(live, &s.cfg, pl, why) == RB_OK && pl.max_mesh_index == 9); }
        {
            Scene s = small(); s.nodes = cyclic(); s.point(RB_CREATE); s.cfg.bvh_nodes.change = RB_UPDATE;
            UpdatePlan pl; std::string why;
            CHECK(plan_update(fresh, &s.cfg, pl, why) == RB_OK && pl.act[kNodes] == Act::None && pl.act[kTriangles] == Act::Take && pl.len[kNodes] == 0);
        }
    }

    // ------------------------------------------------------------------------ the replay ---
    struct Reader {
        std::vector<char> buf;
        size_t at = 0;
        template <typename T> T get() { T v; take(&v, sizeof v); return v; }
        void take(void* dst, size_t n) {
            if (at + n > buf.size()) { fail(__LINE__, "the replay file is short"); std::exit(1); }
            if (n) std::memcpy(dst, buf.data() + at, n);
            at += n;
        }
        template <typename T> rb_field field(std::vector<T>& v) {
            const uint32_t tag = get<uint32_t>();
            v.resize((size_t)get<uint64_t>());
            take(v.data(), v.size() * sizeof(T));
            return rb_field{tag, v.empty() ? nullptr : v.data(), v.size()};
        }
    };

    static void replay(const char* path) {
        Reader r;
        std::ifstream in(path, std::ios::binary);
        r.buf.assign(std::istreambuf_iterator<char>(in), std::istreambuf_iterator<char>());
        const uint32_t engines = r.get<uint32_t>(), want_steps = r.get<uint32_t>(), want_refusals = r.get<uint32_t>();
        unsigned steps_run = 0, refusals = 0, own_rebuilds = 0;
        for (uint32_t e = 0; e < engines; e++) {
            SceneFacts sc;
            sc.own_tree = r.get<uint32_t>() != 0;
            const uint32_t steps = r.get<uint32_t>();
            for (uint32_t i = 0; i < steps; i++, steps_run++) {
                g_what = "replay: engine " + std::to_string(e) + " step " + std::to_string(i);
                Scene s;
                s.cfg.uniforms = r.field(s.uniforms), s.cfg.spheres = r.field(s.spheres), s.cfg.uvs = r.field(s.uvs), s.cfg.meshes = r.field(s.meshes);
                s.cfg.lights = r.field(s.lights), s.cfg.bvh_nodes = r.field(s.nodes), s.cfg.bvh_indices = r.field(s.indices), s.cfg.bvh_triangles = r.field(s.tris);
                const uint32_t tex_tag = r.get<uint32_t>();
                s.textures.resize((size_t)r.get<uint64_t>());
                s.texels.resize(s.textures.size());
                for (size_t k = 0; k < s.textures.size(); k++) {
                    s.textures[k].width = r.get<uint32_t>(), s.textures[k].height = r.get<uint32_t>();
                    s.texels[k].resize((size_t)r.get<uint64_t>());
                    r.take(s.texels[k].data(), s.texels[k].size() * 4);
                    s.textures[k].rgba_data = s.texels[k].data();
                }
                s.cfg.textures = {tex_tag, s.textures.empty() ? nullptr : s.textures.data(), s.textures.size()};
                const bool refused = r.get<uint32_t>() != 0;
                const int code = r.get<int32_t>();
                const SceneFacts before = sc;
                UpdatePlan pl;
                std::string why;
                const int rc = plan_update(sc, &s.cfg, pl, why);
                if ((rc != RB_OK) != refused) { fail(__LINE__, refused ? "the model refuses, the planner does not" : "the planner refuses, the model does not", why); if (!refused) r.at += 4 * 21; continue; }
                if (refused) {
                    refusals++;
                    if (code != 0 && rc != code) fail(__LINE__, "another RB_ERR_* than the model's reason stands for", std::to_string(rc) + " '" + why + "'");
                    CHECK(same(sc, before));
                    continue;
                }
                uint32_t act[9], len[8], eff[3];
                r.take(act, sizeof act), r.take(len, sizeof len);
                const uint32_t kept = r.get<uint32_t>();
                r.take(eff, sizeof eff);
                for (uint32_t f = 0; f < kFieldCount; f++) CHECK((uint32_t)pl.act[f] == act[f]);
                own_rebuilds += pl.own_tree == OwnTree::Rebuild;
                commit_all(sc, pl, &s.cfg);
                // the lengths as the kernels see them: an empty lights or indices vector still has one element
                const uint32_t want[kFieldCount] = {0, len[0], len[1], len[2], std::max(len[3], 1u), len[4], std::max(len[5], 1u), len[6], len[7]};
                const uint32_t have[kFieldCount] = {0, sc.n_spheres, sc.n_uvs, sc.n_meshes, sc.n_lights, sc.n_nodes, sc.n_indices, sc.n_tris, sc.n_tex};
                for (uint32_t f = 1; f < kFieldCount; f++) {
                    if (have[f] != want[f]) fail(__LINE__, kFields[f].name, "length " + std::to_string(have[f]) + ", the model's " + std::to_string(want[f]));
                    CHECK(pl.len[f] == have[f]);   // the plan said so
                }
                CHECK(sc.host_nodes.size() == sc.n_nodes && sc.initialized && sc.have_uniforms);
                CHECK(spheres_count(sc) == eff[0] && node_count(sc) == eff[1] && triangle_count(sc) == eff[2]);
                // a count the model calls kept is the caller's (clamped), every other one the buffer's length
                if (!(kept & 2u)) CHECK(node_count(sc) == sc.n_nodes);
                if (!(kept & 4u)) CHECK(triangle_count(sc) == sc.n_tris);
            }
        }
        g_what = "the replay itself";
        CHECK(r.at == r.buf.size());
        CHECK(steps_run == want_steps && refusals == want_refusals && want_steps > 200 && want_refusals > 30 && own_rebuilds > 10);
    }

    // ------------------------------------------------------------------- the shard layout ---
    static void shard_sweep() {
        for (uint32_t h = 0; h <= 70; h++) for (uint32_t n = 1; n <= 5; n++) for (uint32_t sr : {1u, 4u, 8u, 0u}) {
            g_what = "shard_layout: height " + std::to_string(h) + ", " + std::to_string(n) + " ranks, stripe_rows " + std::to_string(sr);
            std::vector<uint32_t> seen(h, 0);
            uint32_t owned = 0;
            const uint32_t stripe = sr ? sr : kDefaultStripeRows, padded = shard_layout(h, 0, n, sr).padded;
            for (uint32_t rank = 0; rank < n; rank++) {
                const ShardLayout l = shard_layout(h, rank, n, sr);
                CHECK(l.rank == rank && l.count == n && l.stripe == stripe && l.padded == padded);
                CHECK(l.owned <= l.whole_rows && l.whole_rows <= l.padded);
                if (n > 1) CHECK(l.padded % stripe == 0 && l.whole_rows % stripe == 0);
                else CHECK(l.padded == h && l.whole_rows == h);
                owned += l.owned;
                uint32_t inside = 0;
                for (uint32_t lr = 0; lr < l.padded; lr++) {
                    const uint32_t y = l.global_row(lr);
                    if (y < h) seen[y]++, inside++;
                    if (y < h) CHECK(lr < l.whole_rows);   // the rows a rank renders come first in its buffer
                }
                CHECK(inside == l.owned);
            }
            CHECK(owned == h);
            uint32_t wrong = 0;
            for (uint32_t y = 0; y < h; y++) wrong += seen[y] != 1;
            CHECK(wrong == 0);
        }
        g_what = "shard_layout: worked";
        ShardLayout l = shard_layout(70, 1, 4, 0);   // 9 stripes of 8: rank 1 has stripes 1 and 5
        CHECK(l.whole_rows == 16 && l.owned == 16 && l.padded == 24 && l.global_row(0) == 8 && l.global_row(9) == 41);
        l = shard_layout(70, 0, 4, 0);               // rank 0 has 0, 4 and 8, the last cut to 6 rows
        CHECK(l.whole_rows == 24 && l.owned == 22 && l.global_row(23) == 71);
    }

    int main(int argc, char** argv) {
        if (argc != 2) return 2;
        worked_refusals();
        replay(argv[1]);
        shard_sweep();
        CHECK(patch_count(RB_CREATE, 5, 9) == 9 && patch_count(RB_UPDATE, 50, 9) == 9 && patch_count(RB_DELETE, 5, 9) == 0 && patch_count(RB_KEEP, 5, 9) == 5 && patch_count(RB_KEEP, 50, 9) == 9);
        if (failures) return 1;
        std::puts("ok");
        return 0;
    }
''')


def test_update_plan_under_sanitizers(tmp_path):
    replay = tmp_path / "replay.bin"
    write_replay(replay)
    src = tmp_path / "update_plan.cpp"
    src.write_text(SRC)
    exe = tmp_path / "update_plan"
    gxx = ["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-pthread"]
    units = {str(src): str(tmp_path / "update_plan.o"), os.path.join(CSRC, "rb_bvh.cpp"): str(tmp_path / "rb_bvh.o")}
    jobs = [subprocess.Popen(gxx + ["-I", CSRC, "-c", unit, "-o", obj]) for unit, obj in units.items()]   # side by side: rb_bvh.cpp is the long one
    assert [j.wait() for j in jobs] == [0, 0]
    subprocess.check_call(gxx + list(units.values()) + ["-o", str(exe)])
    out = subprocess.run([str(exe), str(replay)], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stdout + out.stderr
    assert out.stdout.strip() == "ok"
