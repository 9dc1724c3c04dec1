"""The numpy model of the irradiance probes (renderbaby_amd/probes.py), the part that needs no device: the
basis is the orthonormal real SH of bands 0-2 in the stated order, the rays are unit, uniform and seeded by rb_trace_rays' rule,
and the projection of a constant colour gives that colour back as irradiance over pi."""
import numpy as np
import pytest

from renderbaby_amd import abi, hemisphere, probes
from renderbaby_amd.camera import pcg, random_float

f32, f64 = np.float32, np.float64
AXES = np.array([(1, 0, 0), (-1, 0, 0), (0, 1, 0), (0, -1, 0), (0, 0, 1), (0, 0, -1)], f32)
A, B, C20, C22, Y0 = f32(0.488602512), f32(1.09254843), f32(0.315391565), f32(0.546274215), f32(0.282094792)


def _u32(a):
    return np.ascontiguousarray(a).view(np.uint32)


def test_basis_is_orthonormal():
    """the integral of Y_i Y_j over a 512 x 1024 latitude-longitude midpoint grid, in float64 from the model's float32 values:
    within 1e-4 of the identity (the float32 basis is good to about 1e-7, the quadrature to about 1e-5)"""
    nt, nph = 512, 1024
    th = (np.arange(nt) + 0.5) * np.pi / nt
    ph = (np.arange(nph) + 0.5) * 2.0 * np.pi / nph
    d = np.stack([np.outer(np.sin(th), np.cos(ph)), np.outer(np.sin(th), np.sin(ph)), np.outer(np.cos(th), np.ones(nph))], axis=-1)
    y = probes.basis(d.reshape(-1, 3).astype(f32))
    assert y.dtype == f32 and y.shape == (nt * nph, 9)
    w = (np.sin(th) * (np.pi / nt) * (2.0 * np.pi / nph))[:, None].repeat(nph, 1).reshape(-1)
    gram = (y.astype(f64) * w[:, None]).T @ y.astype(f64)
    assert np.abs(gram - np.eye(9)).max() <= 1e-4, gram


def test_axis_directions_give_the_hand_written_rows():
    """the order y, z, x / xy, yz, z^2, xz, x^2 - y^2 and the five constants"""
    z = f32(0)
    lo, hi = f32(-C20), f32(C20 * f32(2.0))
    want = np.array([(Y0, z, z, A, z, z, lo, z, C22), (Y0, z, z, -A, z, z, lo, z, C22),
                     (Y0, A, z, z, z, z, lo, z, -C22), (Y0, -A, z, z, z, z, lo, z, -C22),
                     (Y0, z, A, z, z, z, hi, z, z), (Y0, z, -A, z, z, z, hi, z, z)], f32)
    assert np.array_equal(probes.basis(AXES), want)
    # the second band's mixed terms, on the diagonals of the coordinate planes
    h = f32(0.5)
    got = probes.basis(np.array([(1, 1, 0), (0, 1, 1), (1, 0, 1)], f32) * h)
    assert got[0, 4] == f32(B * f32(0.25)) and got[1, 5] == f32(B * f32(0.25)) and got[2, 7] == f32(B * f32(0.25))
    assert got[0, 5] == 0 and got[0, 7] == 0 and got[1, 4] == 0 and got[1, 7] == 0 and got[2, 4] == 0 and got[2, 5] == 0


def test_rays_are_unit_and_the_poles_are_reached_without_a_nan():
    o, d, _ = probes.rays(np.array([(1, 2, 3), (-4, 5, 6)], f32), 7, 4096)
    assert o.dtype == f32 and d.dtype == f32 and d.shape == (8192, 3)
    assert np.array_equal(o, np.repeat(np.array([(1, 2, 3), (-4, 5, 6)], f32), 4096, axis=0))
    length = np.sqrt((d.astype(f64) ** 2).sum(1))
    assert np.abs(length - 1.0).max() <= 4 * float(np.spacing(f32(1)))
    # u2 == 1.0f: z = -1, r = 0; u2 == 0: z = 1
    pole = probes.direction(f32([0.0, 0.3, 1.0, 0.5]), f32([1.0, 1.0, 1.0, 0.0]))
    assert not np.isnan(pole).any()
    assert np.array_equal(pole, np.array([(0, 0, -1)] * 3 + [(0, 0, 1)], f32))
    # a draw can be exactly 1.0f: the largest seeds round up
    assert random_float(np.array([0], np.uint32))[1].max() < 1 and (np.array([2 ** 32 - 1], np.uint32).astype(f32) / f32(4294967296.0))[0] == 1


def test_a_non_finite_position_gives_the_zero_direction_record():
    pos = np.array([(0, 0, 0), (np.inf, 1, 2), (1, np.nan, 2), (1, 2, -np.inf), (3e38, 3e38, 3e38)], f32)
    o, d, s = probes.rays(pos, 0, 3)
    assert np.array_equal(_u32(o), _u32(np.repeat(pos, 3, axis=0)))   # the position as given, NaN bits and all
    gone = (d == 0).all(1).reshape(5, 3)
    assert np.array_equal(gone.all(1), [False, True, True, True, False]) and np.array_equal(gone.any(1), gone.all(1))
    assert np.array_equal(_u32(d[3:12]), np.zeros((9, 3), np.uint32))   # +0, not -0
    # the draws are made all the same: the seeds do not depend on the position
    assert np.array_equal(s, probes.rays(np.zeros((5, 3), f32), 0, 3)[2])


@pytest.mark.parametrize("ids", [None, np.array([5, 0xFFFFFFFF, 123456789, 0], np.uint32)], ids=["index", "seeds"])
def test_seeds_follow_the_rule_of_rb_trace_rays(ids):
    n, first, samples = 4, 0xFFFFFFF0, 9   # (first_sample + k stays below 2^32)
    _, d, s = probes.rays(np.zeros((n, 3), f32), first, samples, seeds=ids)
    dr = hemisphere.draws(n, first, samples, ids)
    assert np.array_equal(s, dr["seed"])
    sid = np.arange(n, dtype=np.uint64) if ids is None else ids.astype(np.uint64)
    k = np.arange(samples, dtype=np.uint64)
    seed = pcg((sid[:, None] + pcg(np.uint64(first) + k)[None, :].astype(np.uint64)) & np.uint64(0xFFFFFFFF)).reshape(-1)
    seed, u1 = random_float(seed)
    seed, u2 = random_float(seed)
    assert np.array_equal(s, seed)   # exactly two draws
    assert np.array_equal(_u32(d), _u32(probes.direction(u1, u2)))


def test_directions_are_uniform_on_the_sphere():
    """N = 2^16 draws of one probe: every component's mean within 6 sigma of 0, sigma = sqrt(1 / (3 N)) (a component of a
    uniform unit vector has variance 1 / 3)"""
    n = 1 << 16
    _, d, _ = probes.rays(np.zeros((1, 3), f32), 0, n)
    mean = d.astype(f64).mean(0)
    assert np.abs(mean).max() <= 6.0 * np.sqrt(1.0 / (3.0 * n)), mean
    # and both hemispheres of every axis are drawn from
    assert ((d > 0).mean(0) > 0.48).all() and ((d < 0).mean(0) > 0.48).all()


def test_projection_of_a_constant_colour():
    samples = 1024
    c = np.array([0.5, 1.0, 2.0], f32)
    pos = np.array([(0, 0, 0), (1, 2, 3), (-7, 0, 2)], f32)
    _, d, _ = probes.rays(pos, 3, samples)
    sh = probes.project(d, np.tile(c, (len(d), 1)), samples)
    assert sh.dtype == abi.SH9 and sh.shape == (3,) and (sh["weight"] == samples).all()
    # sum[0]: the ordered float32 sum of c * Y0, bit for bit
    want = np.zeros(3, f32)
    for _ in range(samples):
        want = (want + (c * Y0).astype(f32)).astype(f32)
    assert np.array_equal(_u32(sh["sum"][:, 0, :]), _u32(np.tile(want, (3, 1))))
    # E / pi = c within 6 sigma, sigma = 1.283 c / sqrt(samples): the l = 1 and l = 2 estimators' variances 4 pi c^2 / samples
    # per coefficient, folded with A_l / pi and sum_m Y_lm(n)^2
    e = probes.irradiance(sh, AXES) / np.pi
    assert e.shape == (3, 6, 3)
    sigma = 1.283 * c.astype(f64) / np.sqrt(samples)
    assert (np.abs(e - c.astype(f64)) <= 6.0 * sigma).all(), (e, sigma)
    # the weight column: an item of weight 0 (an invalid sample's {0, 0, 0, 0} slot) changes no bit of any sum
    col4 = np.concatenate([np.tile(c, (len(d), 1)), np.ones((len(d), 1), f32)], axis=1)
    assert np.array_equal(_u32(probes.project(d, col4, samples).view(f32)), _u32(sh.view(f32)))
    d2, c2 = np.insert(d, 5, 0, axis=0)[:len(d)], np.insert(col4, 5, 0, axis=0)[:len(d)]
    d2[samples:], c2[samples:] = d[samples:], col4[samples:]
    sh2 = probes.project(d2, c2, samples)
    one = probes.project(np.delete(d2[:samples], 5, axis=0), np.delete(c2[:samples], 5, axis=0), samples - 1)
    assert sh2["weight"][0] == samples - 1 and np.array_equal(_u32(sh2["sum"][0]), _u32(one["sum"][0]))
    assert np.array_equal(_u32(sh2[1:].view(f32)), _u32(sh[1:].view(f32)))


def test_host_conveniences():
    sh = np.zeros(2, dtype=abi.SH9)
    sh["sum"][0, 0], sh["weight"][0] = (2.0, 4.0, 8.0), 16
    L = probes.radiance_coefficients(sh)
    assert L.shape == (2, 9, 3) and np.allclose(L[0, 0], np.array([2.0, 4.0, 8.0]) * 4 * np.pi / 16) and (L[1] == 0).all()
    assert np.array_equal(L, probes.radiance_coefficients(sh.view(f32).reshape(2, 28)))
    g = probes.grid((0, 0, 0), (4, 2, 1), (4, 2, 1))
    assert g.dtype == f32 and g.shape == (8, 3) and np.array_equal(g[:5], f32([(0.5, 0.5, 0.5), (1.5, 0.5, 0.5), (2.5, 0.5, 0.5), (3.5, 0.5, 0.5), (0.5, 1.5, 0.5)]))
    r = probes.records(g)
    assert r.dtype == abi.PROBE and np.array_equal(r["pos"], g) and (r["_pad"] == 0).all()
    with pytest.raises(ValueError):
        probes.grid((0, 0, 0), (1, 1, 1), (1, 0, 1))
    with pytest.raises(ValueError):
        probes.project(np.zeros((5, 3), f32), np.zeros((5, 3), f32), 2)
