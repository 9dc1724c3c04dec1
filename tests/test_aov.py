"""renderbaby_amd.aov on hand-made records: orientation, the values of NONE / INVALID pixels, id colours."""
import numpy as np

from renderbaby_amd import abi, aov
from tests import _oracle


def _records():
    """2 rows x 3 columns: [0] ground, sphere 7, none; [1] triangle 517 of mesh 2, light 0, invalid."""
    hits = np.zeros((2, 3), dtype=abi.HIT)
    surf = np.zeros((2, 3), dtype=abi.SURFACE)
    hits["prim"] = hits["mesh"] = abi.NO_INDEX
    hits["t"] = np.float32(1e20)
    kinds = [[abi.HIT_GROUND, abi.HIT_SPHERE, abi.HIT_NONE], [abi.HIT_TRIANGLE, abi.HIT_LIGHT, abi.HIT_INVALID]]
    hits["kind"] = np.array(kinds, dtype=np.uint32)
    hits["t"][0, 0], hits["t"][0, 1], hits["t"][1, 0], hits["t"][1, 1] = 2.0, 4.0, 10.0, 6.0
    hits["prim"][0, 1], hits["prim"][1, 0], hits["prim"][1, 1] = 7, 517, 0
    hits["mesh"][1, 0] = 2
    hits["normal"][0, 0] = (0, 1, 0)
    hits["normal"][0, 1] = (-1, 0, 0)
    hits["normal"][1, 0] = (0, 0, 1)
    hits["normal"][1, 1] = (1, 0, 0)
    surf["albedo"][0, 0] = (0.5, 0.5, 0.5)
    surf["albedo"][0, 1] = (0.25, 1.0, 0.0)
    surf["emissive"][0, 2] = (0.5, 0.7, 1.0)   # NONE carries the sky colour
    surf["emissive"][1, 1] = (15.0, 15.0, 15.0)
    return hits, surf


def test_images_keep_the_orientation_of_the_records():
    """Records arrive mirrored like the frame; record [r, c] must become pixel [r, c] in every image."""
    hits, surf = _records()
    for name in aov.NAMES:
        img = aov.image(name, hits, surf)
        assert img.shape == (2, 3, 4) and img.dtype == np.uint8 and (img[..., 3] == 255).all(), name
    n = aov.normal(hits)
    assert tuple(n[0, 0, :3]) == (128, 255, 128) and tuple(n[0, 1, :3]) == (0, 128, 128)
    assert tuple(n[1, 0, :3]) == (128, 128, 255) and tuple(n[1, 1, :3]) == (255, 128, 128)
    d = aov.depth(hits)
    assert d.dtype == np.float32 and d[0, 0] == 2.0 and d[0, 1] == 4.0 and d[1, 0] == 10.0 and d[1, 1] == 6.0
    d8 = aov.depth_u8(hits)
    assert d8[0, 0, 0] == 255 and d8[1, 0, 0] == 1 and d8[0, 1, 0] > d8[1, 1, 0] > d8[1, 0, 0]


def test_none_and_invalid_have_defined_values():
    hits, surf = _records()
    d = aov.depth(hits)
    assert np.isinf(d[0, 2]) and np.isinf(d[1, 2])
    for img in (aov.depth_u8(hits), aov.normal(hits), aov.albedo(hits, surf), aov.primitive_id(hits), aov.mesh_id(hits)):
        assert tuple(img[0, 2]) == (0, 0, 0, 255) and tuple(img[1, 2]) == (0, 0, 0, 255)
    em = aov.emission(hits, surf)
    assert tuple(em[1, 2]) == (0, 0, 0, 255)
    sky = _oracle.color_map(np.array([0.5, 0.7, 1.0], np.float32))
    assert tuple(em[0, 2, :3]) == (sky & 255, (sky >> 8) & 255, (sky >> 16) & 255)
    assert tuple(em[1, 1, :3]) == (255, 255, 255)   # above 1: clamped, not wrapped


def test_albedo_uses_the_librarys_colour_mapping():
    hits, surf = _records()
    al = aov.albedo(hits, surf)
    for rc in ((0, 0), (0, 1)):
        ref = _oracle.color_map(surf["albedo"][rc])
        assert tuple(al[rc][:3]) == (ref & 255, (ref >> 8) & 255, (ref >> 16) & 255)


def test_id_colours_are_the_shaders_hash():
    hits, _ = _records()
    pid, mid = aov.primitive_id(hits), aov.mesh_id(hits)
    for img, rc, n in ((pid, (0, 1), 7), (pid, (1, 0), 517), (pid, (1, 1), 0), (mid, (1, 0), 2)):
        ref = _oracle.color_map(_oracle.hash_to_color(n + 1))
        assert tuple(img[rc][:3]) == (ref & 255, (ref >> 8) & 255, (ref >> 16) & 255), (rc, n)
    assert tuple(pid[0, 0]) == (0, 0, 0, 255)   # the ground has no index
    assert tuple(mid[0, 1]) == (0, 0, 0, 255)   # a sphere has no mesh
    ids = np.arange(0, 5000, 7, dtype=np.uint32)
    got = aov.hash_to_color(ids)
    for i, n in enumerate(ids):
        assert np.array_equal(got[i].view(np.uint32), _oracle.hash_to_color(int(n)).view(np.uint32))
