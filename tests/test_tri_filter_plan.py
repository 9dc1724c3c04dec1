"""The host side of the triangle sift (renderbaby_amd/csrc/rb_tri_filter.hpp; DESIGN.md section 4, "The triangle sift"): the group
table of a node's list, the decision whether a launch sifts, and the origin region.  Host code with no HIP in it: compiled into a
stand-alone program under AddressSanitizer and UBSan, as tests/test_trace_facts.py does it, and run on the host.

The program reads lists of prepared triangles this file writes, and prints each list's table and region.  Held here:
 * the tables are the numpy model's (renderbaby_amd/tri_filter_model.py build_table, table_region) -- same groups, every stored
   float within one float32 step (the two sides share the formulas, not the libm);
 * the rules: a group is a run of at most 4 consecutive slots and never straddles a block of 32; the Cornell box is six quads;
   invalid, non-finite, normal-less and over-long triangles form groups that always pass; fewer than 4 live triangles, or no group
   that can reject, or a list of more than 128, or a camera that is not finite: no sift."""
import os
import struct
import subprocess
import textwrap

import numpy as np

from renderbaby_amd import scenes
from renderbaby_amd import tri_filter_model as M

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "renderbaby_amd", "csrc")
F32 = np.float32

SRC = textwrap.dedent(r'''
    #include <cstdio>
    #include <cstring>
    #include <vector>
    #include "rb_tri_filter.hpp"
    using namespace rb;
    static uint32_t bits(float f) { uint32_t b; std::memcpy(&b, &f, 4); return b; }
    // input: u32 lists; per list: u32 n, u32 first, f32 extra[6], then n records of 10 words (v0, e1, e2, valid)
    int main(int argc, char** argv) {
        if (argc < 2) return 2;
        FILE* f = std::fopen(argv[1], "rb");
        if (!f) return 2;
        uint32_t lists = 0;
        if (std::fread(&lists, 4, 1, f) != 1) return 2;
        for (uint32_t l = 0; l < lists; l++) {
            uint32_t n = 0, first = 0;
            float extra[1][6];
            if (std::fread(&n, 4, 1, f) != 1 || std::fread(&first, 4, 1, f) != 1 || std::fread(extra, 4, 6, f) != 6) return 2;
            std::vector<PrepTri> t(first + n);
            for (uint32_t i = 0; i < n; i++) {
                float w[9];
                uint32_t valid = 0;
                if (std::fread(w, 4, 9, f) != 9 || std::fread(&valid, 4, 1, f) != 1) return 2;
                PrepTri& p = t[first + i];
                std::memcpy(p.v0, w, 12), std::memcpy(p.e1, w + 3, 12), std::memcpy(p.e2, w + 6, 12);
                p.valid = valid;
            }
            SiftTable tb;
            build_sift_table(t.data(), first, first + n, tb);
            const SiftRegion r = sift_region(tb, extra, 1);
            std::printf("list %u ngroups %zu live %u closed %u ends %08x pays %d on %d\n", l, tb.groups.size(), tb.live, tb.closed, tb.block_ends,
                        (int)sift_pays(tb), (int)r.on);
            for (const SiftGroup& g : tb.groups) {
                std::printf("g %u %u %u", g.first, g.count, g.closed);
                const float w[12] = {g.c[0], g.c[1], g.c[2], g.fk, g.h[0], g.h[1], g.h[2], g.cap, g.n[0], g.n[1], g.n[2], g.s};
                for (float x : w) std::printf(" %08x", bits(x));
                std::printf("\n");
            }
            if (r.on) {
                std::printf("r");
                const float w[11] = {r.lo[0], r.lo[1], r.lo[2], r.hi[0], r.hi[1], r.hi[2], r.kp, r.ks, r.kt, r.kd, r.rmax};
                for (float x : w) std::printf(" %08x", bits(x));
                std::printf("\n");
            }
        }
        std::fclose(f);
        return 0;
    }
''')

NAN = float("nan")


def _prepared(tris):
    a = np.asarray(tris, F32).reshape(-1, 3, 3)
    return a[:, 0], a[:, 1] - a[:, 0], a[:, 2] - a[:, 0]


def _soup(n, seed):
    rng = np.random.default_rng(seed)
    out = []
    while len(out) < n:
        c = rng.uniform(-4, 4, 3)
        a, b = rng.normal(size=3), rng.normal(size=3)
        q = scenes._quad(tuple(c - a - b), tuple(c + a - b), tuple(c + a + b), tuple(c - a + b))
        out += q if rng.uniform() < 0.6 else q[:1]
    return out[:n]


def _lists():
    corn = [t for _, g in scenes.cornell_groups() for t in g]
    odd = [((0, 1, -4), (0, 1, -4), (0, 1, -4)), ((-1, 1, -4), (0, 1, -4), (1, 1, -4)), ((NAN, 1, -4), (1, 1, -4), (0, 2, -4)),
           ((-1e30, -1e30, -9), (1e30, -1e30, -9), (0, 1e30, -9)), ((-2e9, 0, -9), (2e9, 0, -9), (0, 3e9, -9))]
    cam = (0.0, 3.0, 5.0)
    L = []   # (name, triangles, valid, first, camera)
    L.append(("cornell", corn, None, 0, cam))
    L.append(("cornell at slot 5", corn, None, 5, cam))
    L.append(("three live", corn[:3], None, 0, cam))
    L.append(("four live", corn[:4], None, 0, cam))
    L.append(("four, one invalid", corn[:4], [1, 1, 0, 1], 0, cam))
    L.append(("odd only", odd, None, 0, cam))
    L.append(("odd among ordinary", corn[:5] + odd + corn[5:], None, 0, cam))
    L.append(("a run of open ones", odd + odd + corn, None, 0, cam))
    L.append(("33: a quad across the block edge", _soup(31, 1) + corn[:2] + corn[4:6], None, 0, cam))
    L.append(("64", _soup(64, 2), None, 0, cam))
    L.append(("128", _soup(128, 3), None, 3, cam))
    L.append(("129", _soup(129, 4), None, 0, cam))
    L.append(("coplanar strip of eight", [t for k in range(4) for t in scenes._quad((k, 0, 0), (k + 1, 0, 0), (k + 1, 1, 0), (k, 1, 0))] + corn[:2], None, 0, cam))
    L.append(("camera not finite", corn, None, 0, (0.0, NAN, 5.0)))
    L.append(("camera far away", corn, None, 0, (0.0, 3e12, 5.0)))
    return L


def _run(tmp_path, lists):
    blob = [struct.pack("<I", len(lists))]
    for _, tris, valid, first, cam in lists:
        v0, e1, e2 = _prepared(tris)
        valid = np.ones(len(v0), np.uint32) if valid is None else np.asarray(valid, np.uint32)
        blob.append(struct.pack("<II", len(v0), first) + np.asarray(cam + cam, F32).tobytes())
        for k in range(len(v0)):
            blob.append(np.concatenate([v0[k], e1[k], e2[k]]).astype(F32).tobytes() + struct.pack("<I", int(valid[k])))
    data = tmp_path / "lists.bin"
    data.write_bytes(b"".join(blob))
    src = tmp_path / "tri_filter_plan.cpp"
    src.write_text(SRC)
    exe = tmp_path / "tri_filter_plan"
    gxx = ["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-pthread"]
    subprocess.check_call(gxx + ["-I", CSRC, "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)])
    out = subprocess.run([str(exe), str(data)], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stdout + out.stderr
    tables, cur = [], None
    for line in out.stdout.splitlines():
        w = line.split()
        if w[0] == "list":
            cur = dict(groups=[], region=None, **{w[i]: int(w[i + 1], 16 if w[i] == "ends" else 10) for i in range(2, len(w), 2)})
            tables.append(cur)
        elif w[0] == "g":
            cur["groups"].append((int(w[1]), int(w[2]), int(w[3]), np.array([int(x, 16) for x in w[4:]], np.uint32).view(F32)))
        else:
            cur["region"] = np.array([int(x, 16) for x in w[1:]], np.uint32).view(F32)
    return tables


def _close(a, b):
    """within one float32 step, infinities equal"""
    a, b = np.asarray(a, F32), np.asarray(b, F32)
    return bool(np.all((a == b) | (np.abs(a.view(np.int32).astype(np.int64) - b.view(np.int32).astype(np.int64)) <= 1)))


def test_tables_under_sanitizers(tmp_path):
    lists = _lists()
    tables = _run(tmp_path, lists)
    assert len(tables) == len(lists)
    by = {l[0]: t for l, t in zip(lists, tables)}
    for (name, tris, valid, first, cam), tb in zip(lists, tables):
        n = len(tris)
        if n > M.MAX_SLOTS:
            assert tb["groups"] == [] and not tb["pays"] and not tb["on"], name
            continue
        # the rules
        at = first
        for gf, gc, closed, w in tb["groups"]:
            assert gf == at and 1 <= gc <= M.GROUP_MAX and (gf - first) // 32 == (gf + gc - 1 - first) // 32, (name, gf, gc)
            if not closed:
                assert np.isinf(w[3]) and np.isinf(w[7]), (name, "an open group must fail f <= FMax")
            at += gc
        assert at == first + n, name
        ends = [(tb["ends"] >> (8 * b)) & 255 for b in range(4)]
        for b in range(4):
            assert ends[b] == sum(1 for gf, _, _, _ in tb["groups"] if gf - first < 32 * (b + 1)), (name, ends)
        # the model's table
        v0, e1, e2 = _prepared(tris)
        val = np.ones(n, bool) if valid is None else np.asarray(valid, bool)
        groups, live, closed = M.build_table(v0, e1, e2, val)
        assert (tb["live"], tb["closed"]) == (live, closed), name
        assert [(gf - first, gc, c) for gf, gc, c, _ in tb["groups"]] == [(a, c, int(g["closed"][0])) for a, c, g in groups], name
        for (_, _, c, w), (_, _, g) in zip(tb["groups"], groups):
            if c:
                mine = np.concatenate([g["c"][:, 0], g["fk"], g["h"][:, 0], g["cap"], g["nrm"][:, 0], g["s"]])
                assert _close(w, mine), (name, w, mine)
        pays = live >= M.MIN_LIVE and closed >= 1
        assert bool(tb["pays"]) == pays, name
        if tb["on"]:
            reg = M.table_region(groups, cam, cam)
            mine = np.concatenate([reg["lo"][:, 0], reg["hi"][:, 0], reg["kp"], reg["ks"], reg["kt"], reg["kd"], reg["rmax"]])
            assert _close(tb["region"], mine), (name, tb["region"], mine)
    assert [g[1] for g in by["cornell"]["groups"]] == [2] * 6 and by["cornell"]["closed"] == 6 and by["cornell"]["on"]
    assert [g[:3] for g in by["cornell at slot 5"]["groups"]] == [(5 + 2 * k, 2, 1) for k in range(6)]
    assert not by["three live"]["pays"] and by["four live"]["pays"] and not by["four, one invalid"]["pays"]
    assert by["odd only"]["closed"] == 0 and not by["odd only"]["pays"] and not by["odd only"]["on"]
    assert by["odd among ordinary"]["pays"] and sum(1 for g in by["odd among ordinary"]["groups"] if not g[2]) == 2     # five open ones: 4 + 1
    assert [g[:3] for g in by["33: a quad across the block edge"]["groups"]][-3:] == [(31, 1, 1), (32, 1, 1), (33, 2, 1)]
    assert [g[1] for g in by["coplanar strip of eight"]["groups"]] == [2, 2, 2, 2, 2], "a strip's union box outgrows its members'"
    assert by["camera not finite"]["pays"] and not by["camera not finite"]["on"]
    assert by["camera far away"]["pays"] and not by["camera far away"]["on"]
