"""The launch plan of the stream kernels (renderbaby_amd/csrc/rb_color_plan.hpp): how many passes a launch takes and how many
colour parts the launches alternate between.  Plain integer arithmetic, so it is compiled into a stand-alone program under
AddressSanitizer and UBSan and run on the host; no GPU, and nothing is loaded into Python."""
import os
import subprocess
import textwrap

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

SRC = textwrap.dedent(r'''
    #include <cstdio>
    #include <cstdlib>
    #include "rb_color_plan.hpp"
    using rb::ColorPlan; using rb::plan_colors;
    static int failures = 0;
    #define CHECK(c) do { if (!(c)) { std::printf("line %d: %s\n", __LINE__, #c); failures++; } } while (0)

    int main() {
        // C2: 1920 x 1080 = 240 x 135 tiles of 64 items, 1024 passes, 4 GiB: 129 passes would fit; two halves of 64
        const uint64_t c2 = 240ull * 135 * 64, gib4 = (4ull << 30) / 16;
        ColorPlan p = plan_colors(c2, 1024, 0, gib4);
        CHECK(p.chunk == 64 && p.parts == 2 && p.launches(1024) == 16);
        CHECK(p.floats(c2) * 4 <= (4ull << 30));                         // resident memory does not grow past the budget
        p = plan_colors(c2, 129, 0, gib4);  CHECK(p.chunk == 129 && p.parts == 1 && p.launches(129) == 1);   // fits: one part, as ever
        p = plan_colors(c2, 130, 0, gib4);  CHECK(p.chunk == 64 && p.parts == 2 && p.launches(130) == 3);
        // 64 x 40 at 1 MiB: 2560 items per pass, 25 passes fit, 12 per half
        const uint64_t small = 8 * 5 * 64, mib = (1ull << 20) / 16;
        const unsigned want[] = {1, 25, 1,  26, 12, 3,  36, 12, 3,  37, 12, 4,  48, 12, 4,  49, 12, 5,  60, 12, 5};
        for (int i = 0; i < 7; i++) {
            p = plan_colors(small, want[3 * i], 0, mib);
            CHECK(p.launches(want[3 * i]) == want[3 * i + 2]);
            CHECK(p.parts == (want[3 * i + 2] > 1 ? 2u : 1u));
            if (p.parts == 2) CHECK(p.chunk == want[3 * i + 1] && p.floats(small) * 4 <= (1ull << 20));
        }
        // the caller's passes per launch: kept as given; one part when that is one launch
        p = plan_colors(small, 5, 1, mib);    CHECK(p.chunk == 1 && p.parts == 2 && p.launches(5) == 5);
        p = plan_colors(small, 5, 7, mib);    CHECK(p.chunk == 5 && p.parts == 1);
        p = plan_colors(small, 5, 5, mib);    CHECK(p.chunk == 5 && p.parts == 1);
        p = plan_colors(small, 6, 3, 0);      CHECK(p.chunk == 3 && p.parts == 2);     // the budget does not bind a fixed chunk
        // a budget below two passes: one part of one pass, as before
        p = plan_colors(small, 9, 0, small);          CHECK(p.chunk == 1 && p.parts == 1);
        p = plan_colors(small, 9, 0, 2 * small - 1);  CHECK(p.chunk == 1 && p.parts == 1);
        p = plan_colors(small, 9, 0, 2 * small);      CHECK(p.chunk == 1 && p.parts == 2);
        p = plan_colors(small, 9, 0, 0);              CHECK(p.chunk == 1 && p.parts == 1);
        // a launch counts items in 32 bits: below 2^31 whatever the budget or the caller say
        const uint64_t big = 1ull << 27;
        p = plan_colors(big, 100, 0, ~0ull);   CHECK(p.chunk == 16 && p.parts == 2 && big * p.chunk <= (1ull << 31));
        p = plan_colors(big, 100, 64, ~0ull);  CHECK(p.chunk == 16 && p.parts == 2);
        p = plan_colors(big, 16, 0, ~0ull);    CHECK(p.chunk == 16 && p.parts == 1);
        p = plan_colors((1ull << 31) + 1, 4, 0, ~0ull);  CHECK(p.chunk == 0 && p.launches(4) == 0);   // no launch can hold one pass
        p = plan_colors(0, 4, 0, 100);         CHECK(p.chunk == 4 && p.parts == 1);                   // (guarded division)
        // out of memory: the launch halves, the parts stay; it ends at one pass
        p = plan_colors(c2, 1024, 0, gib4);
        unsigned steps = 0;
        while (rb::halve(p)) { steps++; CHECK(p.parts == 2 && p.chunk >= 1); }
        CHECK(steps == 6 && p.chunk == 1 && !rb::halve(p));
        p.chunk = 5; CHECK(rb::halve(p) && p.chunk == 3);
        // every pass is launched exactly once
        for (unsigned n = 1; n <= 70; n++)
            for (uint64_t b = 0; b <= 40; b += 3) {
                p = plan_colors(small, n, 0, b * small);
                unsigned done = 0, launches = 0;
                while (done < n) { done += (n - done < p.chunk ? n - done : p.chunk); launches++; }
                CHECK(done == n && launches == p.launches(n) && (p.parts == 1 || launches >= 3));
                CHECK(p.parts == 1 || p.floats(small) <= b * small * 4);
            }
        if (failures) return 1;
        std::puts("ok");
        return 0;
    }
''')


def test_color_plan_under_sanitizers(tmp_path):
    src = tmp_path / "plan.cpp"
    src.write_text(SRC)
    exe = tmp_path / "plan"
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-fsanitize=address,undefined",
                           "-fno-sanitize-recover=all", "-I", os.path.join(ROOT, "renderbaby_amd", "csrc"), str(src), "-o", str(exe)])
    out = subprocess.run([str(exe)], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stdout + out.stderr
    assert out.stdout.strip() == "ok"
