"""What the scalar unit sustains next to the vector units on this device (rb_measure_salu_mix, k_salu_mix in rb_debug.hip):
a loop of independent v_fma_f32 at 8 waves per SIMD on every CU with 0, 4, 8, 12 or 16 independent scalar adds among each 16 of
them, without and with one never-taken s_cbranch_execz per 16.  Prints the table DESIGN.md section 9 quotes
(profiles/rNN_salu_mix.txt): shader clocks per vector instruction and SIMD -- 2 is the vector unit's own limit at one wave64
instruction per 2 clocks (a 16-lane SIMD would be 4) -- and from them the scalar instructions a CU retires per clock.

   python tools/salu_mix.py [device]
"""
import ctypes as C
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from renderbaby_amd import _lib  # noqa: E402


def main():
    device = int(sys.argv[1]) if len(sys.argv) > 1 else 0
    lib = _lib.load()
    base = {}
    print("# scalar/16 vector  branch/16   clocks per vector instr. and SIMD   vs. no scalar   scalar instr. per CU-clock   GHz      ms")
    for branch in (0, 1):
        for scalar in (0, 4, 8, 12, 16):
            v = (C.c_double * 3)()
            rc = lib.rb_measure_salu_mix(device, scalar, branch, v)
            if rc != 0:
                print(f"{scalar:10d} {branch:10d}   failed (rc {rc})", flush=True)
                continue
            base.setdefault(branch, v[0])
            # per 64 vector instructions a wave issues 4 * scalar adds, 4 * branch branches and the loop's own three
            per_valu = (4 * scalar + 4 * branch + 3) / 64.0
            salu_rate = 4.0 * per_valu / v[0]          # four SIMDs share the CU's scalar unit
            print(f"{scalar:10d} {branch:10d} {v[0]:28.3f} {v[0] / base[0]:22.3f} {salu_rate:22.3f} {v[1]:16.3f} {v[2]:8.3f}", flush=True)


if __name__ == "__main__":
    main()
