"""The canonical reference-layout tree (rb_bvh_build_canonical) on the host: a small numpy model of the
rule, rb_bvh_build's shape and node count, refusal of non-finite input, and the device builder's size query (no device)."""
import numpy as np
import pytest

from renderbaby_amd import abi, bvh, scenes
from renderbaby_amd.engine import RenderError
from tests.test_bvh import _check_tree


def _ord(a):
    """float32 -> u32 under the total order in which -0 < +0."""
    b = np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)
    return np.where(b & np.uint32(0x80000000), ~b, b | np.uint32(0x80000000)).astype(np.uint32)


def _unord(k):
    k = np.asarray(k, dtype=np.uint32)
    return np.where(k & np.uint32(0x80000000), k & np.uint32(0x7FFFFFFF), ~k).astype(np.uint32).view(np.float32)


def _nodes_of(count):
    return 1 if count <= 128 else 1 + _nodes_of(count // 2) + _nodes_of(count - count // 2)


def canonical_model(tris):
    """The rule, restated level by level: per node the (centroid along the axis, index) order by np.lexsort in f32."""
    n = len(tris)
    v = np.stack([tris["v0"], tris["v1"], tris["v2"]], axis=1).astype(np.float32)   # (n, 3, 3)
    cen = ((v[:, 0] + v[:, 1]) + v[:, 2]) / np.float32(3.0)
    kv = _ord(v)
    tmn, tmx = kv.min(axis=1), kv.max(axis=1)
    nodes = np.zeros(_nodes_of(n) if n else 0, dtype=abi.BVH_NODE)
    idx = np.arange(n, dtype=np.uint32)
    level = [(0, n, 0)] if n else []
    while level:
        nxt = []
        for first, count, me in level:
            ids = idx[first:first + count]
            mn, mx = _unord(tmn[ids].min(axis=0)), _unord(tmx[ids].max(axis=0))
            nodes[me]["aabb_min"], nodes[me]["aabb_max"] = mn, mx
            if count <= 128:
                nodes[me]["first_primitive"], nodes[me]["primitive_count"] = first, count
                idx[first:first + count] = np.sort(ids)
                continue
            ex, ey, ez = mx - mn
            axis = 0 if (ex > ey and ex > ez) else (1 if ey > ez else 2)
            idx[first:first + count] = ids[np.lexsort((ids, cen[ids, axis]))]
            half = count // 2
            left, right = me + 1, me + 1 + _nodes_of(half)
            nodes[me]["left"], nodes[me]["right"] = left, right
            nxt += [(first, half, left), (first + half, count - half, right)]
        level = nxt
    return nodes, idx


def _soup(n, seed, scale=10.0):
    rng = np.random.default_rng(seed)
    t = np.zeros(n, dtype=abi.GPU_TRIANGLE)
    c = rng.uniform(-scale, scale, size=(n, 1, 3)).astype(np.float32)
    p = (c + rng.uniform(-0.5, 0.5, size=(n, 3, 3))).astype(np.float32)
    t["v0"], t["v1"], t["v2"] = p[:, 0], p[:, 1], p[:, 2]
    t["mesh_index"] = 0
    return t


def _from_vertices(p):
    t = np.zeros(len(p), dtype=abi.GPU_TRIANGLE)
    p = np.asarray(p, dtype=np.float32)
    t["v0"], t["v1"], t["v2"] = p[:, 0], p[:, 1], p[:, 2]
    return t


def _terrain(nx=24, nz=20):
    return _from_vertices(scenes.terrain_tris(nx, nz, seed=7))   # C3's grid: many equal centroids along x and z


def _identical(n):
    return _from_vertices(np.tile(np.array([[[0, 0, 0], [1, 0, 0], [0, 1, 0]]], np.float32), (n, 1, 1)))


def _shared_centroid(n, seed=5):
    rng = np.random.default_rng(seed)
    d = rng.uniform(-1, 1, size=(n, 3)).astype(np.float32)
    return _from_vertices(np.stack([d, -d, np.zeros_like(d)], axis=1))   # every centroid is (0, 0, 0) (or -0)


def _signed_zeros(n, seed=9):
    rng = np.random.default_rng(seed)
    p = rng.choice(np.array([0.0, -0.0, 1.0, -1.0], np.float32), size=(n, 3, 3)).astype(np.float32)
    return _from_vertices(p)


# the inputs of the model comparison; the device test (tests/test_gpu_build_tree.py) uses the same sets
def model_sets():
    sets = {f"soup{n}": _soup(n, n) for n in (1, 2, 100, 128, 129, 130, 255, 256, 257, 258, 1000, 5000)}
    sets["terrain"] = _terrain()
    sets["identical"] = _identical(1000)
    sets["identical129"] = _identical(129)
    sets["shared_centroid"] = _shared_centroid(777)
    sets["signed_zeros"] = _signed_zeros(600)
    sets["tiny_scale"] = _soup(2000, 3, scale=0.01)   # crowded centroids
    return sets


SETS = model_sets()


@pytest.mark.parametrize("name", sorted(SETS))
def test_canonical_matches_the_numpy_model(name):
    tris = SETS[name]
    nodes, idx = bvh.build_canonical(tris)
    m_nodes, m_idx = canonical_model(tris)
    assert nodes.tobytes() == m_nodes.tobytes()
    assert np.array_equal(idx, m_idx)
    if len(tris) > 0:
        ref_nodes, _ = bvh.build(tris)
        assert len(nodes) == len(ref_nodes)


@pytest.mark.parametrize("name", ["soup1000", "soup5000", "terrain", "signed_zeros"])
def test_canonical_tree_is_reference_shaped(name):
    tris = SETS[name]
    nodes, idx = bvh.build_canonical(tris)
    if name == "signed_zeros":   # the box check compares with np.min / np.max, which do not order -0 and +0
        tris = tris.copy()
        for f in ("v0", "v1", "v2"):
            tris[f] = tris[f] + np.float32(0.0)
        nodes = nodes.copy()
        nodes["aabb_min"] = nodes["aabb_min"] + np.float32(0.0)
        nodes["aabb_max"] = nodes["aabb_max"] + np.float32(0.0)
    _check_tree(nodes, idx, tris)


@pytest.mark.parametrize("n,seed", [(1000, 1), (5000, 2), (20000, 3), (129, 4), (257, 5)])
def test_canonical_equals_rb_bvh_build_without_ties(n, seed):
    tris = _soup(2 * n, seed, scale=1000.0)
    v = np.stack([tris["v0"], tris["v1"], tris["v2"]], axis=1)
    cen = ((v[:, 0] + v[:, 1]) + v[:, 2]) / np.float32(3.0)
    alone = np.ones(len(tris), dtype=bool)
    for a in range(3):   # drop every triangle whose centroid coordinate another one shares
        _, inv, cnt = np.unique(cen[:, a], return_inverse=True, return_counts=True)
        alone &= cnt[inv] == 1
    tris = tris[alone][:n]
    v = np.stack([tris["v0"], tris["v1"], tris["v2"]], axis=1)
    cen = ((v[:, 0] + v[:, 1]) + v[:, 2]) / np.float32(3.0)
    for a in range(3):
        assert len(np.unique(cen[:, a])) == n, "the soup must be tie-free"
    nodes, idx = bvh.build_canonical(tris)
    r_nodes, r_idx = bvh.build(tris)
    assert nodes.tobytes() == r_nodes.tobytes()
    for nd in nodes[nodes["primitive_count"] > 0]:
        f, c = int(nd["first_primitive"]), int(nd["primitive_count"])
        assert np.array_equal(idx[f:f + c], np.sort(r_idx[f:f + c]))


def test_canonical_empty():
    nodes, idx = bvh.build_canonical(np.zeros(0, dtype=abi.GPU_TRIANGLE))
    assert len(nodes) == 0 and len(idx) == 0


@pytest.mark.parametrize("builder", [bvh.build_canonical, bvh.build_device], ids=["host", "device"])
@pytest.mark.parametrize("bad", [np.nan, np.inf, -np.inf])
def test_non_finite_vertices_are_refused(builder, bad):
    tris = _soup(300, 8)
    tris["v1"][217, 2] = bad
    with pytest.raises(RenderError) as ei:
        builder(tris)
    assert ei.value.code == 13 and "217" in ei.value.message   # RB_ERR_INVALID_BVH, naming the triangle
    bvh.build(tris)   # rb_bvh_build keeps accepting it


@pytest.mark.parametrize("n", [0, 1, 127, 128, 129, 256, 257, 1000, 50_176, 1_048_578])
def test_device_size_query_needs_no_device(n):
    tris = _soup(n, 11) if n <= 50_176 else np.zeros(n, dtype=abi.GPU_TRIANGLE)
    if n > 50_176:   # C5's count: a strip of distinct triangles keeps rb_bvh_build's splits cheap
        x = np.arange(n, dtype=np.float32)
        tris["v0"][:, 0], tris["v1"][:, 0], tris["v2"][:, 0] = x, x + 1, x
        tris["v2"][:, 1] = 1
    assert bvh.node_count(n) == len(bvh.build(tris)[0])
