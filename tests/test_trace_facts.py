"""The scene facts the flat kernels of k_trace rest on (renderbaby_amd/csrc/rb_update_plan.hpp: untextured,
commit_trace_facts; DESIGN.md section 4, "Scenes that carry no u, v").  Host code with no HIP in it: compiled with rb_bvh.cpp
into a stand-alone program under AddressSanitizer and UBSan, as tests/test_update_plan.py does it, and run on the host.

Two parts.  The facts over hand-made material and triangle tables: index -1 everywhere, one mesh textured, one sphere textured,
only a light textured, an index past the textures, no elements.  Then a sequence of updates through plan_update and the commit
functions: after every step the facts equal the facts recomputed from scratch from the scene the engine then holds, and a field
that is taken, deleted or left alone follows the plan's Take / Delete / None."""
import os
import subprocess
import textwrap

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "renderbaby_amd", "csrc")

SRC = textwrap.dedent(r'''
    #include <cmath>
    #include <cstdio>
    #include <string>
    #include <vector>
    #include "rb_update_plan.hpp"
    using namespace rb;
    static int failures = 0;
    static std::string g_what;
    #define CHECK(c) do { if (!(c) && failures++ < 20) std::printf("line %d: %s   [%s]\n", __LINE__, #c, g_what.c_str()); } while (0)

    static rb_mesh mesh(int tex) { rb_mesh m{}; m.material.texture_index = tex; return m; }
    static rb_sphere sphere(int tex) { rb_sphere s{}; s.radius = 1.0f; s.material.texture_index = tex; return s; }
    static rb_point_light light(int tex) { rb_point_light l{}; l.radius = 1.0f; l.material.texture_index = tex; return l; }
    // a triangle at `at` whose first edge has the x component e1 and whose second has the y component e2
    static rb_gpu_triangle tri(float e1, float e2, float at = 0.0f) {
        rb_gpu_triangle t{};
        t.v0[0] = t.v0[1] = t.v0[2] = at;
        t.v1[0] = at + e1, t.v1[1] = at, t.v1[2] = at;
        t.v2[0] = at, t.v2[1] = at + e2, t.v2[2] = at;
        return t;
    }

    // ---- the scene an engine holds, and its facts from scratch: written out here, not through the header's functions
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
        std::vector<uint32_t> texels;
        bool lights_deleted = false;
    };
    struct Facts { bool meshes, spheres, lights, no_uv; };
    static Facts scratch(const Scene& s) {
        Facts f{true, true, true, true};
        for (const rb_mesh& m : s.meshes) f.meshes = f.meshes && m.material.texture_index < 0;
        for (const rb_sphere& m : s.spheres) f.spheres = f.spheres && m.material.texture_index < 0;
        for (const rb_point_light& m : s.lights) f.lights = f.lights && m.material.texture_index < 0;
        if (s.lights.empty() && !s.lights_deleted) f.lights = false;   // the zero-filled light of an empty vector: index 0
        f.no_uv = f.meshes && f.spheres;
        return f;
    }
    static bool agree(const SceneFacts& sc, const Facts& f) {
        return sc.untex_meshes == f.meshes && sc.untex_spheres == f.spheres && sc.untex_lights == f.lights && sc.no_uv == f.no_uv;
    }

    static Scene small() {
        Scene s;
        rb_uniforms u{};
        u.width = 8, u.height = 8, u.total_samples = 1, u.camera.pane_distance = 1.0f, u.camera.pane_width = 1.0f, u.camera.dir[2] = -1.0f, u.max_depth = 2;
        s.uniforms = {u};
        s.spheres = {sphere(-1), sphere(-1)};
        s.uvs = {0.0f, 1.0f};
        s.meshes = {mesh(-1), mesh(-1)};
        s.lights = {light(-1)};
        rb_bvh_node leaf{};
        leaf.primitive_count = 2;
        s.nodes = {leaf};
        s.indices = {0u, 1u};
        s.tris = {tri(1.0f, 1.0f), tri(2.0f, 0.5f, 3.0f)};
        s.tris[1].mesh_index = 1;
        s.texels = {0xFFFFFFFFu};
        s.textures = {rb_texture{1, 1, nullptr}};
        return s;
    }

    // ------------------------------------------------------------------ the tables ---
    static void tables() {
        g_what = "tables";
        {   // index -1 everywhere, and other negative indices
            std::vector<rb_mesh> m = {mesh(-1), mesh(-1), mesh(-7)};
            std::vector<rb_sphere> s = {sphere(-1)};
            std::vector<rb_point_light> l = {light(-1), light(-1)};
            CHECK(untextured(m.data(), m.size()) && untextured(s.data(), s.size()) && untextured(l.data(), l.size()));
        }
        { std::vector<rb_mesh> m = {mesh(-1), mesh(0), mesh(-1)}; CHECK(!untextured(m.data(), m.size())); }              // one mesh textured
        { std::vector<rb_sphere> s = {sphere(-1), sphere(-1), sphere(2)}; CHECK(!untextured(s.data(), s.size())); }       // one sphere textured
        { std::vector<rb_point_light> l = {light(3)}; CHECK(!untextured(l.data(), l.size())); }                          // a light
        { std::vector<rb_mesh> m = {mesh(1000000)}; CHECK(!untextured(m.data(), m.size())); }                            // an index past any n_tex is a texture still
        { std::vector<rb_mesh> m = {mesh(2147483647)}; CHECK(!untextured(m.data(), m.size())); }
        CHECK(untextured(static_cast<const rb_mesh*>(nullptr), 0));                                                       // nothing: vacuous
        CHECK(!untextured(static_cast<const rb_mesh*>(nullptr), 3));                                                      // unreadable: not established
    }

    // ------------------------------------------------------------------ a sequence of updates ---
    // what the engine does with an accepted plan, the device left out; the scene `have` follows it field by field
    static void step(int line, SceneFacts& sc, Scene& have, Scene next, const uint32_t (&tag)[kFieldCount]) {
        g_what = "sequence, step of line " + std::to_string(line);
        next.textures[0].rgba_data = next.texels.data();
        rb_config cfg{};
        cfg.uniforms = {tag[kUniforms], next.uniforms.data(), next.uniforms.size()}, cfg.spheres = {tag[kSpheres], next.spheres.data(), next.spheres.size()};
        cfg.uvs = {tag[kUvs], next.uvs.data(), next.uvs.size()}, cfg.meshes = {tag[kMeshes], next.meshes.data(), next.meshes.size()};
        cfg.lights = {tag[kLights], next.lights.data(), next.lights.size()}, cfg.bvh_nodes = {tag[kNodes], next.nodes.data(), next.nodes.size()};
        cfg.bvh_indices = {tag[kIndices], next.indices.data(), next.indices.size()}, cfg.bvh_triangles = {tag[kTriangles], next.tris.data(), next.tris.size()};
        cfg.textures = {tag[kTextures], next.textures.data(), next.textures.size()};
        UpdatePlan pl;
        std::string why;
        const SceneFacts before = sc;
        const int rc = plan_update(sc, &cfg, pl, why);
        if (rc != RB_OK) { CHECK(rc == RB_OK); std::printf("  refused: %s\n", why.c_str()); return; }
        for (uint32_t f = 0; f < kFieldCount; f++) commit_field(sc, pl, &cfg, (Field)f);
        commit_end(sc, pl);
        // a field the plan leaves alone keeps its fact; one it takes or deletes has the new vector's, or none
        if (pl.act[kMeshes] == Act::None) CHECK(sc.untex_meshes == before.untex_meshes); else have.meshes = pl.act[kMeshes] == Act::Take ? next.meshes : std::vector<rb_mesh>{};
        if (pl.act[kSpheres] == Act::None) CHECK(sc.untex_spheres == before.untex_spheres); else have.spheres = pl.act[kSpheres] == Act::Take ? next.spheres : std::vector<rb_sphere>{};
        if (pl.act[kLights] == Act::None) CHECK(sc.untex_lights == before.untex_lights);
        else have.lights = pl.act[kLights] == Act::Take ? next.lights : std::vector<rb_point_light>{}, have.lights_deleted = pl.act[kLights] == Act::Delete;
        const Facts f = scratch(have);
        if (!agree(sc, f) && failures++ < 20)
            std::printf("line %d: facts %d %d %d %d, from scratch %d %d %d %d\n", line, sc.untex_meshes, sc.untex_spheres, sc.untex_lights, sc.no_uv,
                        f.meshes, f.spheres, f.lights, f.no_uv);
    }
    #define STEP(next, ...) do { const uint32_t tag[kFieldCount] = {__VA_ARGS__}; step(__LINE__, sc, have, next, tag); } while (0)

    static void sequence() {
        const uint32_t K = RB_KEEP, C = RB_CREATE, U = RB_UPDATE, D = RB_DELETE;
        SceneFacts sc;
        Scene have;
        have.lights_deleted = true;   // nothing yet
        CHECK(!sc.no_uv && !sc.untex_lights);                       // nothing is established before the first update
        //                uniforms spheres uvs meshes lights nodes indices triangles textures
        Scene s = small();
        STEP(s, C, C, C, C, C, C, C, C, C);
        CHECK(sc.no_uv && sc.untex_lights);
        s.spheres[1] = sphere(0);     STEP(s, K, U, K, K, K, K, K, K, K);   CHECK(!sc.no_uv && sc.untex_meshes);      // a sphere gets a texture
        s.spheres[1] = sphere(-1);    STEP(s, K, U, K, K, K, K, K, K, K);   CHECK(sc.no_uv);                                            // and loses it
        s.meshes[0] = mesh(4);        STEP(s, K, K, K, U, K, K, K, K, K);   CHECK(!sc.no_uv && sc.untex_spheres);                       // a mesh, past the textures
        { Scene o = s; o.spheres[0] = sphere(0); o.meshes[0] = mesh(-1); STEP(o, K, K, K, K, K, K, K, K, K); }   // Keep: the incoming data says nothing
        CHECK(!sc.no_uv && sc.untex_spheres && !sc.untex_meshes);
        { Scene o = s; o.spheres[0] = sphere(0); STEP(o, K, C, K, K, K, K, K, K, K); }                            // Create after the first update is not acted on
        CHECK(sc.untex_spheres);
        s.meshes[0] = mesh(-1);       STEP(s, U, K, K, U, K, K, K, K, K);   CHECK(sc.no_uv);
        s.lights[0] = light(0);       STEP(s, K, K, K, K, U, K, K, K, K);   CHECK(sc.no_uv && !sc.untex_lights);                        // only a light: no_uv holds, the lights' part does not
        s.lights.clear();             STEP(s, K, K, K, K, U, K, K, K, K);   CHECK(!sc.untex_lights && sc.n_lights == 1);                // no lights: the phantom's index is 0
        s.lights = {light(-1), light(-2)}; STEP(s, K, K, K, K, U, K, K, K, K); CHECK(sc.untex_lights);
        s.tris[1] = tri(8.0f, 8.0f);
        s.tris[1].mesh_index = 1;     STEP(s, K, K, K, K, K, K, K, C, K);   CHECK(sc.no_uv);                                            // the triangles say nothing of it
        s.spheres[0] = sphere(7);     STEP(s, K, U, K, K, K, K, K, K, K);   CHECK(!sc.no_uv);
        STEP(s, K, D, K, K, K, K, K, K, K);                                 CHECK(sc.no_uv && sc.n_spheres == 0);                       // deleted spheres: none is read
        s.spheres = {sphere(-1), sphere(3)}; STEP(s, K, U, K, K, K, K, K, K, K); CHECK(!sc.no_uv);                                      // and created again
    }

    int main() {
        tables();
        sequence();
        if (failures) return 1;
        std::puts("ok");
        return 0;
    }
''')


def test_trace_facts_under_sanitizers(tmp_path):
    src = tmp_path / "trace_facts.cpp"
    src.write_text(SRC)
    exe = tmp_path / "trace_facts"
    gxx = ["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-pthread"]
    units = {str(src): str(tmp_path / "trace_facts.o"), os.path.join(CSRC, "rb_bvh.cpp"): str(tmp_path / "rb_bvh.o")}
    jobs = [subprocess.Popen(gxx + ["-I", CSRC, "-c", unit, "-o", obj]) for unit, obj in units.items()]
    assert [j.wait() for j in jobs] == [0, 0]
    subprocess.check_call(gxx + list(units.values()) + ["-o", str(exe)])
    out = subprocess.run([str(exe)], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stdout + out.stderr
    assert out.stdout.strip() == "ok"
