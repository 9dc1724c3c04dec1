"""Rounds of random_unit_vector's rejection loop per call, and the lanes that work in a round: a Monte-Carlo model of one
wavefront of k_trace, for the plain loop and for the loop that parks seeds (rb_device_math.hpp).  No GPU.

A try lands inside the unit sphere with probability pi / 6, so a lane needs a geometric number of tries (1.91 on average)
and the wave runs until its slowest lane is served.  In the parked form a served lane searches on through the rounds that
are left and stops in front of its next accepting try; at its next call that lane needs one try.  A path that ends takes
its parked seed with it.

The three inputs come from the phase table (tools/ktrace_phases.py, profiles/r04_ktrace_phases.txt, C2):
   lanes at the segment's entry (63.6), lanes that reach the shading and with it the draw (54.8), segments per path
   (342 045 875 / 66 355 200 = 5.15).
A lane that does not reach the draw has left the scene, its path is over; the others end after the draw as often as the
segments per path ask for.  The table's row to compare with is "unit vector: one try": executions per segment x 64 divided
by the shading row's (rounds per call), and lanes per execution.

   python tools/unit_vector_rounds.py [lanes at entry] [lanes at the draw] [segments per path] [calls, default 200000]"""
import math
import sys

import numpy as np


def model(entry=63.6, draw=54.8, seg_per_path=5.155, calls=200_000, seed=1):
    rng = np.random.default_rng(seed)
    p = math.pi / 6.0
    reach = draw / 64.0                                   # a lane takes part in a call
    end_total = 1.0 / seg_per_path                        # a path ends, per segment
    miss = 1.0 - draw / entry                             # ... before the draw
    end_after = max(0.0, (end_total - miss) / (1.0 - miss))
    out = {}
    for form in ("plain", "parked"):
        parked = np.zeros(64, bool)
        rounds = tries = 0
        n = 0
        for _ in range(calls):
            active = rng.random(64) < reach
            if not active.any():
                parked[:] = False
                continue
            need = rng.geometric(p, 64)                   # tries until the lane's vector
            if form == "parked":
                need = np.where(parked, 1, need)
            r = int(need[active].max())
            n += 1
            rounds += r
            if form == "plain":
                tries += int(need[active].sum())
            else:
                search = rng.geometric(p, 64)             # tries until the next accept: the last of them parks the lane
                left = r - need
                tries += int((need + np.minimum(search, left))[active].sum())
                parked = active & (search <= left)
                parked &= rng.random(64) >= end_after     # the path ended after its draw
            # a lane that sat this call out has started another path
        out[form] = (rounds / n, tries / rounds)
    return out


def main():
    a = [float(x) for x in sys.argv[1:4]]
    calls = int(sys.argv[4]) if len(sys.argv) > 4 else 200_000
    res = model(*a, calls=calls) if len(a) == 3 else model(calls=calls)
    for form, (rounds, lanes) in res.items():
        print(f"{form:7s} rounds per call {rounds:5.2f}   lanes per round {lanes:5.1f}   lane-rounds per call {rounds * lanes:6.1f}")
    (r0, _), (r1, _) = res["plain"], res["parked"]
    print(f"vector instructions per call: plain {r0 * 45:.0f} (45 a try), fused {r0 * 39:.0f} (39), "
          f"fused and parked {40 + (r1 - 1) * 43:.0f} (first try 40, then 43 a round)")


if __name__ == "__main__":
    main()
