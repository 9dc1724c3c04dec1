"""renderbaby_amd.bake, the part that needs no device: the rays of the free cameras and of the irradiance estimator."""
import numpy as np
import pytest

from renderbaby_amd import abi, aov, bake

f32 = np.float32


def _len(v):
    v = v.astype(np.float64)
    return np.sqrt((v * v).sum(-1))


@pytest.mark.parametrize("kind", bake.KINDS)
def test_camera_rays_shapes_and_unit_directions(kind):
    O, D = bake.camera_rays(kind, 37, 19, (1, 2, 3), dir=(0.3, -0.2, -1), aperture=0.2, focus_distance=4.0, seed=5)
    assert O.shape == D.shape == (19, 37, 3) and O.dtype == D.dtype == np.float32
    assert np.isfinite(O).all() and np.isfinite(D).all()
    assert np.abs(_len(D) - 1.0).max() <= 2.0 ** -23   # 1 ulp of 1
    with pytest.raises(ValueError):
        bake.camera_rays("fisheye", 4, 4, (0, 0, 0))
    with pytest.raises(ValueError):
        bake.camera_rays(kind, 0, 4, (0, 0, 0))
    with pytest.raises(ValueError):
        bake.camera_rays(kind, 4, 4, (0, 0, 0), dir=(0, 1, 0), up=(0, 2, 0))


def test_equirect_poles_and_seam():
    w, h = 64, 32
    O, D = bake.camera_rays("equirect", w, h, (1, 2, 3), dir=(0, 0, -1))
    assert (O == np.array([1, 2, 3], f32)).all()
    # rows run from just below the north pole to just above the south pole; no ray is a pole itself
    assert (D[0, :, 1] > 0.99).all() and (D[-1, :, 1] < -0.99).all() and (np.abs(D[..., 1]) < 1).all()
    assert np.allclose(D[:, :, 1], D[:, :1, 1], atol=1e-6)   # latitude depends on the row only
    assert (np.diff(D[:, 0, 1]) < 0).all()
    # the centre columns straddle `dir`, the seam columns straddle -dir, and the seam closes: first and last column mirror
    mid = h // 2
    assert D[mid, w // 2 - 1, 2] < -0.99 and D[mid, w // 2, 2] < -0.99 and D[mid, w // 2 - 1, 0] < 0 < D[mid, w // 2, 0]
    assert D[mid, 0, 2] > 0.99 and D[mid, -1, 2] > 0.99
    assert np.allclose(D[:, 0, 0], -D[:, -1, 0], atol=1e-6) and np.allclose(D[:, 0, 2], D[:, -1, 2], atol=1e-6)
    assert D[mid, w // 4, 0] < -0.9 and D[mid, 3 * w // 4, 0] > 0.9   # longitude grows to the right
    # the whole sphere, evenly in longitude: the directions of a row sum to nothing sideways
    assert np.abs(D[mid, :, [0, 2]].sum(1)).max() < 1e-4


def test_ortho_rays_are_parallel():
    O, D = bake.camera_rays("ortho", 16, 8, (0, 1, 5), dir=(0, -1, -1), ortho_width=4.0)
    assert (D.view(np.uint32) == D[0, 0].view(np.uint32)).all()
    fwd = D[0, 0].astype(np.float64)
    assert np.abs((O.astype(np.float64) - np.array([0, 1, 5.0])) @ fwd).max() < 1e-6   # the window is perpendicular to dir
    assert abs(_len(O[0, -1] - O[0, 0]) - 4.0 * 15 / 16) < 1e-5 and abs(_len(O[-1, 0] - O[0, 0]) - 2.0 * 7 / 8) < 1e-5
    assert O[0, 0, 0] < O[0, -1, 0] and O[0, 0, 1] > O[-1, 0, 1]   # column 0 on the left, row 0 on top


def test_thin_lens_rays_of_one_pixel_meet_at_the_focus_distance():
    kw = dict(dir=(0.2, 0.1, -1), fov_deg=50.0, focus_distance=3.5)
    _, pin = bake.camera_rays("thin_lens", 9, 7, (1, 1, 1), aperture=0.0, **kw)
    focus = np.array([1, 1, 1], np.float64) + 3.5 * pin.astype(np.float64)
    origins = []
    for seed in range(4):
        O, D = bake.camera_rays("thin_lens", 9, 7, (1, 1, 1), aperture=0.5, seed=seed, **kw)
        O64, D64 = O.astype(np.float64), D.astype(np.float64)
        t = ((focus - O64) * D64).sum(-1, keepdims=True)
        assert np.abs(O64 + t * D64 - focus).max() < 1e-5          # every lens sample's ray passes its pixel's focus point
        assert (_len(O64 - np.array([1, 1, 1.0])) <= 0.25 + 1e-6).all()   # on the lens
        origins.append(O)
    assert not np.array_equal(origins[0], origins[1])               # its own seeded lens samples
    again, _ = bake.camera_rays("thin_lens", 9, 7, (1, 1, 1), aperture=0.5, seed=0, **kw)
    assert np.array_equal(again, origins[0])


def test_cosine_weighted_rays_lie_in_the_normals_hemisphere():
    rng = np.random.default_rng(3)
    N = rng.normal(size=(50, 3)).astype(f32)
    N[:3] = np.eye(3, dtype=f32)
    P = rng.uniform(-5, 5, (50, 3)).astype(f32)
    O, D = bake.irradiance_rays(P, N * f32(3.0), 32, seed=2)
    assert O.shape == D.shape == (50 * 32, 3)
    n = (N / np.sqrt((N * N).sum(-1, keepdims=True))).astype(np.float64)
    cos = (D.reshape(50, 32, 3) * n[:, None, :]).sum(-1)
    assert (cos >= -1e-6).all() and np.abs(_len(D) - 1.0).max() < 1e-5
    assert 0.55 < cos.mean() < 0.78                                 # E[cos] = 2 / 3 under the cosine-weighted density
    off = ((O.reshape(50, 32, 3) - P[:, None, :]) * n[:, None, :]).sum(-1)
    assert (off > 0).all() and (O.reshape(50, 32, 3) == O.reshape(50, 32, 3)[:, :1]).all()   # off the surface, one origin per point
    # the generator is ambient_occlusion's
    assert np.array_equal(D, aov.cosine_directions(bake._unit(N * f32(3.0)), 32, 2).reshape(-1, 3))


def test_tone_map_of_sums_and_weights():
    rad = np.zeros((2, 3), dtype=abi.RADIANCE)
    rad["sum"][0, 0], rad["weight"][0, 0] = (4, 4, 4), 4        # mean 1 -> 0.5 -> sqrt -> 181
    rad["sum"][0, 1], rad["weight"][0, 1] = (0, 0, 0), 16
    rad["sum"][1, 2], rad["weight"][1, 2] = (9, 9, 9), 0        # an invalid ray: no weight, black
    img = bake.tone_map(rad)
    assert img.shape == (2, 3, 4) and img.dtype == np.uint8 and (img[..., 3] == 255).all()
    assert tuple(img[0, 0, :3]) == (181, 181, 181) and not img[0, 1, :3].any() and not img[1, 2, :3].any()
