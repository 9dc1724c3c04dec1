"""The rejection loop of random_unit_vector (rb_device_math.hpp) without a GPU.

 * rnd_pm1: `rnd(seed) * 2.0f - 1.0f` is three float32 operations on c = (float)seed; the kernels compute it as one fma,
   RN(c * 2^-31 - 1).  Checked here for EVERY value c can take: 0 and the 2^28 + 1 floats from 1.0f to 4294967296.0f.
 * the parked loop: a lane that has its vector goes on trying and stops in front of its next accepting try.  A scalar
   model (pcg in Python integers, coordinates in numpy float32) draws the same vectors as the plain loop, bit for bit,
   whatever number of search rounds follows each accept.
 * the compiled loop: three v_fma_f32, and no more vector instructions per trip than the 45 of the loop it replaces."""
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import isa_blocks  # noqa: E402

from tests.test_ktrace_isa import KERNELS, _makefile_flags  # noqa: E402

f32, f64 = np.float32, np.float64
M32 = 0xFFFFFFFF


# ------------------------------------------------------------------------------------------------ rnd_pm1, every value
def three_operations(c):
    """rnd(seed) * 2.0f - 1.0f on c = (float)seed, each operation rounded to float32"""
    return (c / f32(4294967296.0)) * f32(2.0) - f32(1.0)


def one_rounding(c):
    """RN(c * 2^-31 - 1), what v_fma_f32 returns.  c * 2^-31 is exact in double; the subtraction is exact there too unless
    c < 4, where the result lies within 2^-29 of -1 and half an ulp of float32 is 2^-26: the double's own rounding
    cannot carry it across a float32 midpoint."""
    return (c.astype(f64) * f64(2.0 ** -31) - f64(1.0)).astype(f32)


def test_one_rounding_equals_three_for_every_float_of_a_seed():
    lo, hi = int(np.array(1.0, f32).view(np.uint32)), int(np.array(4294967296.0, f32).view(np.uint32))
    assert hi - lo == 1 << 28
    mismatches, step = 0, 1 << 24
    for b0 in range(lo, hi + 1, step):
        c = np.arange(b0, min(b0 + step, hi + 1), dtype=np.uint32).view(f32)
        mismatches += int((three_operations(c).view(np.uint32) != one_rounding(c).view(np.uint32)).sum())
    zero = np.zeros(1, f32)
    mismatches += int((three_operations(zero).view(np.uint32) != one_rounding(zero).view(np.uint32)).sum())
    assert mismatches == 0


def test_every_seed_converts_to_a_checked_float():
    # (float)seed of a u32 is 0 or lies in [1, 2^32]: the range above is the whole range
    s = np.array([0, 1, 2, 3, 0x00FFFFFF, 0x01000001, 0x7FFFFFFF, 0x80000000, 0xFFFFFF7F, 0xFFFFFF80, 0xFFFFFFFF], np.uint32)
    c = s.astype(f32)
    assert ((c == 0) | ((c >= 1) & (c <= f32(4294967296.0)))).all()
    assert c[-1] == f32(4294967296.0) and c[-3] == f32(4294967040.0)


# ------------------------------------------------------------------------------------------------ the parked loop, a model
def pcg(seed):
    state = (seed * 747796405 + 2891336453) & M32
    word = (((state >> ((state >> 28) + 4)) ^ state) * 277803737) & M32
    return (word >> 22) ^ word


def try_plain(seed):
    """one try as the shader has it -> (seed after it, the point, inside the unit sphere?)"""
    p = np.zeros(3, f32)
    for k in range(3):
        seed = pcg(seed)
        p[k] = (f32(seed) / f32(4294967296.0)) * f32(2.0) - f32(1.0)
    return seed, p, bool((p[0] * p[0] + p[1] * p[1]) + p[2] * p[2] < f32(1.0))


def try_fused(seed):
    p = np.zeros(3, f32)
    for k in range(3):
        seed = pcg(seed)
        p[k] = f32(f64(f32(seed)) * f64(2.0 ** -31) - f64(1.0))
    return seed, p, bool((p[0] * p[0] + p[1] * p[1]) + p[2] * p[2] < f32(1.0))


def plain_vectors(seed, n):
    out = []
    for _ in range(n):
        while True:
            seed, p, inside = try_plain(seed)
            if inside:
                break
        out.append(p)
    return out


def parked_vectors(seed, n, rounds_of_search, seen):
    """the device's loop for one lane: the tries it is owed, then `rounds_of_search()` more rounds under the parking rule"""
    out, parked = [], False
    for _ in range(n):
        first = True
        while True:
            seed, p, inside = try_fused(seed)
            assert inside or not (parked and first), "a parked seed's next try must accept"
            first = False
            if inside:
                break
        out.append(p)
        parked, rounds = False, rounds_of_search()
        for r in range(rounds):
            before = seed
            seed, _, inside = try_fused(seed)
            if inside:
                seed, parked = before, True        # from here on every round repeats this try and restores again
                seen["parks on its first try"] += r == 0
                break
        seen["runs out of rounds unparked"] += rounds > 0 and not parked
        seen["parked"] += parked
    return out


def test_parked_loop_draws_the_plain_loop_s_vectors():
    rng = np.random.default_rng(20240915)
    starts = [0, 1, M32, 0x80000000] + [int(x) for x in rng.integers(0, 1 << 32, 2044, dtype=np.uint64)]
    assert len(starts) >= 2048
    seen = {"parks on its first try": 0, "runs out of rounds unparked": 0, "parked": 0}
    for s in starts:
        want = plain_vectors(s, 12)
        got = parked_vectors(s, 12, lambda: int(rng.integers(0, 7)), seen)
        assert all(np.array_equal(a.view(np.uint32), b.view(np.uint32)) for a, b in zip(want, got)), s
    print(seen)
    assert seen["parks on its first try"] > 0 and seen["runs out of rounds unparked"] > 0 and seen["parked"] > 0


# ------------------------------------------------------------------------------------------------ the compiled loop
@pytest.fixture(scope="module")
def asm(tmp_path_factory):
    hipcc, flags = _makefile_flags()
    if not (os.path.isfile(hipcc) or __import__("shutil").which(hipcc)):
        pytest.skip("hipcc is not installed")
    s = str(tmp_path_factory.mktemp("rnd_fused_isa") / "rb_kernels.s")
    subprocess.check_call([hipcc, *flags, "-S", "--cuda-device-only", "-o", s, os.path.join(ROOT, "renderbaby_amd/csrc/rb_kernels.hip")],
                          cwd=ROOT)
    return s


@pytest.mark.parametrize("kernel", [k[0] for k in KERNELS])
def test_rejection_loop_isa(asm, kernel):
    blocks = isa_blocks.parse_blocks(asm, kernel)
    loops = []
    for h in (b for b in blocks if b.inner_header):
        body = isa_blocks.loop_blocks(blocks, h.name)
        ops = [i.op for b in body for i in b.instrs]
        if sum(o.startswith("v_mul_lo_u32") for o in ops) == 6:
            loops.append((h.name, ops, sum(len(b.valu) for b in body)))
    assert len(loops) == 1, [l[0] for l in loops]
    name, ops, valu = loops[0]
    print(kernel, name, "VALU per trip", valu, "of them v_fma_f32", sum(o.startswith("v_fma_f32") for o in ops))
    assert sum(o.startswith("v_fma_f32") for o in ops) == 3
    assert valu <= 45
    assert not [o for o in ops if o.startswith("scratch_")]
