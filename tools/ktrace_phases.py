"""Where k_trace's lanes are: per phase of its loop body, how often the code is executed by a wavefront
and with how many of its 64 lanes.  A profiling build (tools/walk_profile.sh) counts, at sixteen points, one execution and
popcount(exec) lanes; this prints them per segment, with the lane occupancy of every phase and -- weighted by the phase's
VALU instructions (counted from the product kernel's ISA, build/rb_kernels.s) -- each phase's share of the idle lane slots.

   RB_LIBRARY_PATH=$PWD/renderbaby_amd/variants/lib_walkprof.so python tools/ktrace_phases.py [c2|c1] [spp] [parked|plain]

The rejection loop of random_unit_vector has two counting points: its first try, which every lane at the draw runs, and one
further round (a try and four selects); of a round's lanes those are counted whose try is wanted -- the lanes still owed a
vector and the served ones searching for their next accepting try, not the parked ones.  `plain`: a profiling build with
-DRB_PARK_SEED=0, the loop without parking, one counting point (every try).  The last line puts both forms beside the model
(tools/unit_vector_rounds.py)."""
import ctypes as C, os, sys
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from renderbaby_amd import Engine, RenderConfig, scenes, _lib
w = sys.argv[1] if len(sys.argv) > 1 else "c2"
spp = int(sys.argv[2]) if len(sys.argv) > 2 else 64
parked = (sys.argv[3] if len(sys.argv) > 3 else "parked") == "parked"
s = scenes.cornell(1920, 1080, spp, 8) if w == "c2" else scenes.cornell(512, 512, spp, 4)
rc = RenderConfig.from_scene(s)
eng = Engine.new(rc, stats=True); eng.update(rc)
lib = _lib.load()
out = (C.c_uint64 * 64)()
eng.clear(); eng.dispatch(0, spp); eng.sync()
assert lib.rb_debug_walk_profile(out, 1) == 0, "not a profiling build (tools/walk_profile.sh)"
eng.reset_stats(); eng.clear(); eng.dispatch(0, spp); eng.sync()
lib.rb_debug_walk_profile(out, 1)
st = eng.stats(); seg = st["segments"]
# (name, slot, VALU instructions of one execution of the phase: rough counts from the ISA of k_trace<false, false, 8>; the rejection
# loop's are exact, from the block table of tools/isa_blocks.py (profiles/r15_ktrace_blocks_after.txt): the first try is block
# BB30_210, 39 -- three hashes of 9, three conversions, three fma, five for the dot product, the compare; a further round is the
# loop BB30_211, 43 = 39 + four selects.  Plain loop around the fused try: 39 a try; with the three roundings of the shader it
# was block BB29_211 of profiles/r15_ktrace_blocks_before.txt, 45.  r04 printed this row with 27, which was never the loop's count.)
TRY_FIRST, TRY_ROUND = (39, 43) if parked else (39, 39)
phases = [("path start (camera ray, two draws)", 8, 95), ("segment entry (triangle loop set-up, ground)", 9, 30),
          ("triangle test: cross, determinant", 10, 14), ("  ... reciprocal, u", 11, 22), ("  ... cross, v", 12, 16), ("  ... t, accept", 13, 14),
          ("sphere pass 1 (discriminant)", 14, 17), ("sphere pass 2 (sqrt, roots)", 15, 45), ("light pass 1", 16, 17), ("light pass 2", 17, 45),
          ("shading: winner's record, emission", 18, 70), ("unit vector: the first try", 7, TRY_FIRST), ("unit vector: one try of the rejection loop", 19, TRY_ROUND), ("metal scatter", 20, 45),
          ("lambert scatter", 21, 30), ("texture / checkerboard", 22, 40), ("path end (colour store)", 23, 12)]
print(f"{w} {spp} spp, {eng.last_kernel_name()}: segments {seg}, paths {st['paths']}")
print(f"{'phase':50s} {'exec / segment x 64':>20s} {'lanes / exec':>13s} {'VALU':>5s} {'wave-instr / seg':>17s} {'idle lane-instr / seg':>22s}")
tot_w = tot_idle = 0.0
for name, slot, valu in phases:
    n, lanes = out[2 * slot], out[2 * slot + 1]
    if n == 0:
        continue
    wi = n * valu / seg                       # wave-instructions per segment spent in this phase
    idle = (64 * n - lanes) * valu / seg / 64  # of which idle (in wave-instruction equivalents)
    tot_w += wi; tot_idle += idle
    print(f"{name:50s} {64 * n / seg:20.2f} {lanes / n:13.1f} {valu:5d} {wi:17.2f} {idle:22.2f}")
print(f"{'sum of the counted phases':50s} {'':20s} {'':13s} {'':5s} {tot_w:17.2f} {tot_idle:22.2f}   -> lane utilisation {1 - tot_idle / tot_w:.3f}")
n_shade, n_first, n_round, l_first, l_round = out[2 * 18], out[2 * 7], out[2 * 19], out[2 * 7 + 1], out[2 * 19 + 1]
if n_shade and n_first + n_round:
    calls = n_first if n_first else n_shade      # the plain build has no counting point in front of its loop: one call per shading pass
    print(f"rejection loop, all tries: executions / segment x 64 {64 * (n_first + n_round) / seg:.2f}, rounds per call {(n_first + n_round) / calls:.2f}, "
          f"lanes per round {(l_first + l_round) / (n_first + n_round):.1f}, vector instructions per call "
          f"{(n_first * TRY_FIRST + n_round * TRY_ROUND) / calls:.0f}   (model, tools/unit_vector_rounds.py: plain 6.69 rounds of 15.7 lanes, parked 5.04 of 31.9)")
eng.close()
