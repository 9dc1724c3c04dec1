"""Per-cell emitter tables that learn visibility (rb_direct_light_grid_tally / rb_emitter_grid_learned and their device forms;
DESIGN.md section 25), bit for bit:

  the learned tables = direct.emitter_grid_cdf(tally=...), from one record to past four of k_grid_rows' chunks, for tallies
                       that are empty, saturated, random or have seen above tried, and of the scene's table through the device form;
  the count          = direct.tally under rb_occluded's bytes on the model's records: exact integers in any order -- on top of
                       a tally that is not zero, over two calls, with 64 lanes on one counter, in pieces below 64 surfels,
                       across a piece boundary, without sums, in every form;
  the sums           = rb_direct_light_grid's, and the sums of the older picks on the same engine do not move;
  a refused call has done nothing, the tally included; and end to end a lamp behind a wall loses weight and the mean stays.
"""
import numpy as np
import pytest

from renderbaby_amd import Engine, RenderConfig, abi, bake, direct, engine, hemisphere, scenes
from tests import _oracle
from tests.conftest import has_gpu
from tests.test_direct_abi import INVALID_OPTIONS, NULL_ARGUMENT, REFUSALS, _params
from tests.test_direct_grid_abi import CAP_REFUSALS
from tests.test_direct_grid_model import cells, spread
from tests.test_direct_learn_abi import BAD_PRIORS
from tests.test_direct_learn_model import random_tally, records
from tests.test_gpu_direct import M, PIECE, WALKS, mixed_surfels, tables
from tests.test_gpu_direct_cdf import same_rows
from tests.test_gpu_direct_grid import BOX, CHUNK, GRIDS, box_of
from tests.test_gpu_hemisphere import scene_surfels
from tests.test_gpu_query import _engine
from tests.test_gpu_radiance import _mesh, _u32, given_seeds
from tests.test_probe_light_abi import GRID_REFUSALS, _grid

pytestmark = [pytest.mark.gpu, pytest.mark.skipif(not has_gpu(), reason="needs a GPU")]

f32, u32 = np.float32, np.uint32
TALLY = abi.GRID_TALLY


def t32(t):
    """a tally as the uint32 words it is"""
    return np.ascontiguousarray(t).view(u32).reshape(-1)


def as_tensor(t):
    import torch
    return torch.from_numpy(np.ascontiguousarray(t).view(np.int32).reshape(-1, 2).copy()).cuda()


# ---- 1. the learned tables
@pytest.mark.parametrize("n", [1, 2, 3, 64, 65, CHUNK - 1, CHUNK, CHUNK + 1, 4 * CHUNK + 1])
def test_learned_tables_equal_the_model(n):
    rng = np.random.default_rng(300 + n)
    e = spread(n, rng)
    for k in (0, CHUNK - 1, CHUNK, n - 1):   # unweighable at the ends and on either side of the first chunk's edge
        if k < n and n > 1:
            e["area"][k] = (0.0, np.nan, -1.0, np.inf)[k % 4]
    differs = 0
    for counts in GRIDS:
        g = cells(*BOX, counts)
        m = int(np.prod(counts)) * n
        plain = direct.emitter_grid_cdf(e, g)
        tried = rng.integers(0, 1 << 32, m).astype(u32)
        for name, t, priors in (("zero", np.zeros(m, TALLY), (1.0,)), ("saturated", records(tried, tried), (1.0,)),
                                ("seen above tried", records(tried >> 1, tried), (0.5,)),
                                ("random", random_tally(m, rng), (1.0, 0.5, abi.MAX_PRIOR, 1e-3))):
            for prior in priors:
                want = direct.emitter_grid_cdf(e, g, t, prior)
                keep = t.copy()
                got = engine.emitter_grid_learned(e, g, t, prior, device=0)
                where = (n, counts, name, prior)
                assert got.dtype == u32 and got.shape == want.shape and np.array_equal(t, keep), where
                assert np.array_equal(got, want), (where, np.nonzero(got != want)[0][:5], got[got != want][:5], want[got != want][:5])
                if name != "random":
                    assert np.array_equal(got, plain), where   # the two identities
                else:
                    differs += not np.array_equal(got, plain)
    assert differs > 0 or n <= 3   # (at most one weighable record: its q is S whatever f is)
    assert len(engine.emitter_grid_learned(e[:0], cells(*BOX, (2, 1, 1)), np.zeros(0, TALLY), 1.0, device=0)) == 0


def test_the_scenes_table_through_the_learned_device_form():
    import torch
    s = scenes.feature_scene(width=24, height=16)
    table = direct.scene_emitters(s)
    n = len(table)
    g = bake.pick_grid(table, (3, 2, 2))
    rng = np.random.default_rng(5)
    t = random_tally(12 * n, rng)
    want = direct.emitter_grid_cdf(table, g, t, 2.0)
    assert not np.array_equal(want, direct.emitter_grid_cdf(table, g))
    e = _engine(s)
    try:
        st0 = e.stats()
        got = e.emitter_grid(g, tally=t, prior=2.0)   # d_emitters == NULL: the scene's kept table
        assert e.last_query_kernel_name() == "k_grid_rows_seen" and e.last_query_ms() > 0
        assert got.dtype == u32 and np.array_equal(got, want)
        assert np.array_equal(e.emitter_grid(g, emitters=table, tally=t, prior=2.0), want)
        out = torch.full((12 * n + 3,), 7, dtype=torch.int32, device="cuda")
        d_t = as_tensor(t)
        d_tab = torch.from_numpy(table.view(f32).reshape(-1, 16)).cuda()
        back = e.emitter_grid(g, emitters=d_tab, tally=d_t, prior=2.0, out=out[:12 * n])
        assert back.is_cuda and np.array_equal(back.cpu().numpy().view(u32), want) and (out[12 * n:] == 7).all().item()
        assert np.array_equal(t32(d_t.cpu().numpy()), t32(t)), "the build wrote the tally"
        # a tally that begins one word past an 8-byte boundary: 4-byte alignment is all the ABI asks
        odd = torch.zeros(24 * n + 3, dtype=torch.int32, device="cuda")
        assert odd.data_ptr() % 8 == 0
        d_odd = odd[1:1 + 24 * n].view(12 * n, 2)
        d_odd.copy_(d_t)
        assert d_odd.data_ptr() % 8 == 4 and d_odd.is_contiguous()
        assert np.array_equal(e.emitter_grid(g, emitters=d_tab, tally=d_odd, prior=2.0).cpu().numpy().view(u32), want)
        assert np.array_equal(e.emitter_grid(g), direct.emitter_grid_cdf(table, g)) and e.last_query_kernel_name() == "k_grid_rows"
        assert e.stats() == st0
    finally:
        e.close()


# ---- 2. the count
def model_call(e, table, g, tabs, pts, nrm, samples, first_sample, ids, mask, into=None, offset=1e-3, shorten=1e-3):
    """(direct.tally, direct.fold) of the model's items under rb_occluded's bytes on the model's own records and bounds"""
    surf = hemisphere.surfels(pts, nrm)
    o, d, tmax, contrib = direct.rays(table, surf, first_sample, samples, seeds=ids, offset=offset, shorten=shorten, grid=g, tables=tabs)
    rays = np.zeros(len(o), dtype=abi.RAY)
    rays["origin"], rays["dir"] = o, d
    occ = e.occluded_records(rays, tmax, mask)
    kept = direct.tally(table, surf, first_sample, samples, g, occ, tables=tabs, seeds=ids, offset=offset, shorten=shorten, into=into)
    return kept, direct.fold(contrib, occ, samples)


@pytest.mark.parametrize("name", ["feature", "mesh chunk"])
def test_the_count_equals_the_model(name):
    import torch
    make, kw, kernel = WALKS[name]
    s = make()
    table = direct.scene_emitters(s)
    n = len(table)
    assert n > 0
    e = _engine(s, **kw)
    try:
        pts, nrm = mixed_surfels(e, s)   # the invalid ones among them
        g = box_of(pts, (3, 2, 2))       # a little inside their box: some lie outside the grid
        o, st = g["origin"], g["step"]
        for k, i in enumerate((0, 1, 2, 3)):   # on faces: the box's first corner, inner faces, the last face
            pts[6 + 3 * k] = (o[0] + f32(i) * st[0], o[1] + f32(i % 3) * st[1], o[2] + f32(i % 3) * st[2])
        tabs = direct.emitter_grid_cdf(table, g)
        uniform = e.direct_light(pts, nrm, 4, first_sample=7)
        power = e.direct_light(pts, nrm, 4, first_sample=7, pick="power")
        plain = e.direct_light(pts, nrm, 4, first_sample=7, pick=("grid", g))
        st0 = e.stats()
        rng = np.random.default_rng(8)
        start = records(rng.integers(0, 1000, 12 * n).astype(u32), rng.integers(0, 1000, 12 * n).astype(u32))
        start["tried"][0], start["seen"][1] = 2 ** 32 - 1, 2 ** 32 - 1   # counters that wrap, should they be hit
        running, want_running = start.copy(), start
        tp, tn = torch.from_numpy(pts).cuda(), torch.from_numpy(nrm).cuda()
        d_running = as_tensor(start)
        for samples, first_sample, with_seeds, mask in ((3, 0, False, abi.MASK_ALL), (4, 7, True, abi.MASK_ALL & ~abi.MASK_LIGHTS)):
            ids = given_seeds(M) if with_seeds else None
            where = (name, samples, first_sample)
            ckw = dict(first_sample=first_sample, seeds=ids, mask=mask)
            want_t, want_s = model_call(e, table, g, tabs, pts, nrm, samples, first_sample, ids, mask)
            assert want_t["tried"].sum() > 40 and 0 < want_t["seen"].sum() <= want_t["tried"].sum()
            # from zero, with sums: rb_direct_light_grid's bits beside the model's count
            kept = np.zeros(12 * n, TALLY)
            got = e.direct_light(pts, nrm, samples, pick=("grid", g), tally=kept, **ckw)
            assert e.last_query_kernel_name() == kernel and e.last_query_ms() > 0 and 0 < e.last_camera_rays_ms() <= e.last_query_ms()
            assert np.array_equal(kept, want_t), (where, np.nonzero(t32(kept) != t32(want_t))[0][:6])
            same_rows(got, want_s, where)
            same_rows(got, e.direct_light(pts, nrm, samples, pick=("grid", g), **ckw), where)
            # without sums, with tables given, with a caller's table: the same count
            for more in (dict(pick=("grid", g), out=False), dict(pick=("grid", g, tabs)), dict(pick=("grid", g, tabs), emitters=table, out=False)):
                kept = np.zeros(12 * n, TALLY)
                res = e.direct_light(pts, nrm, samples, tally=kept, **more, **ckw)
                assert (res is None) == ("out" in more) and np.array_equal(kept, want_t), (where, more.keys())
            # on top of a tally that is not zero, call after call, in both forms
            want_running = direct.count(12 * n, np.zeros(0, np.int64), [], [], into=want_running)
            want_running["tried"] += want_t["tried"]
            want_running["seen"] += want_t["seen"]
            e.direct_light(pts, nrm, samples, pick=("grid", g), tally=running, out=False, **ckw)
            assert np.array_equal(running, want_running), where
            tids = None if ids is None else torch.from_numpy(ids.view(np.int32)).cuda()
            d_got = e.direct_light(tp, tn, samples, first_sample=first_sample, seeds=tids, mask=mask, pick=("grid", g), tally=d_running)
            same_rows(d_got.cpu().numpy(), got.view(f32).reshape(-1, 4), where)
            assert np.array_equal(t32(d_running.cpu().numpy()), t32(want_running)), where
        assert want_running["tried"][0] != start["tried"][0] or want_running["tried"].sum() > start["tried"].sum()
        # a numpy tally beside tensors is staged and copied back
        kept = np.zeros(12 * n, TALLY)
        assert e.direct_light(tp, tn, 3, pick=("grid", g), tally=kept, out=False) is None
        assert np.array_equal(kept, model_call(e, table, g, tabs, pts, nrm, 3, 0, None, abi.MASK_ALL)[0])
        # an empty table has nothing to count; the older picks' sums have not moved
        none = e.direct_light(pts, nrm, 4, emitters=table[:0], pick=("grid", g), tally=np.zeros(0, TALLY))
        assert not _u32(none["sum"]).any() and np.array_equal(none["weight"], uniform["weight"])
        same_rows(e.direct_light(pts, nrm, 4, first_sample=7), uniform, (name, "uniform after"))
        same_rows(e.direct_light(pts, nrm, 4, first_sample=7, pick="power"), power, (name, "power after"))
        same_rows(e.direct_light(pts, nrm, 4, first_sample=7, pick=("grid", g)), plain, (name, "grid after"))
        assert e.stats() == st0, "tallied queries moved rb_get_stats"
    finally:
        e.close()


def test_sixty_four_lanes_on_one_counter():
    """One emitter and one cell: every counted item of the call adds to the same two words -- 192 surfels, so whole waves of 64
    lanes hit one counter --, and with the feature scene's five emitters in one cell a wave spreads over five."""
    s = scenes.feature_scene(width=24, height=16)
    e = _engine(s)
    try:
        pts, nrm = scene_surfels(e, s, 192)
        g = box_of(pts, (1, 1, 1))
        for which in ("one", "scene"):
            table = tables()[which]
            tabs = direct.emitter_grid_cdf(table, g)
            kept = np.zeros(len(table), TALLY)
            got = e.direct_light(pts, nrm, 16, emitters=table, first_sample=3, pick=("grid", g), tally=kept)
            want_t, want_s = model_call(e, table, g, tabs, pts, nrm, 16, 3, None, abi.MASK_ALL)
            assert np.array_equal(kept, want_t), (which, kept, want_t)
            same_rows(got, want_s, which)
            assert kept["tried"].sum() > 64 * 4 and 0 < kept["seen"].sum() < kept["tried"].sum()
    finally:
        e.close()


def test_the_plain_form_counts_what_the_combining_form_counts(monkeypatch):
    """RB_GRID_TALLY=plain launches the count with one add per item (the form section 25.5 measures beside the one that is
    launched otherwise, which adds once per wave and record): the same sums, on a tally that begins at 4 mod 8 too."""
    import torch
    s = scenes.feature_scene(width=24, height=16)
    e = _engine(s)
    try:
        pts, nrm = scene_surfels(e, s, 192)
        tp, tn = torch.from_numpy(pts).cuda(), torch.from_numpy(nrm).cuda()
        for which, counts in (("one", (1, 1, 1)), ("scene", (3, 2, 2))):
            table = tables()[which]
            g = box_of(pts, counts)
            m = int(np.prod(counts)) * len(table)
            tabs = direct.emitter_grid_cdf(table, g)
            want = model_call(e, table, g, tabs, pts, nrm, 16, 3, None, abi.MASK_ALL)[0]
            for form in ("plain", "combined"):
                monkeypatch.setenv("RB_GRID_TALLY", form)
                kept = np.zeros(m, TALLY)
                e.direct_light(pts, nrm, 16, emitters=table, first_sample=3, pick=("grid", g), tally=kept, out=False)
                assert np.array_equal(kept, want), (which, form)
                odd = torch.zeros(2 * m + 3, dtype=torch.int32, device="cuda")
                d_odd = odd[1:1 + 2 * m].view(m, 2)
                assert d_odd.data_ptr() % 8 == 4
                e.direct_light(tp, tn, 16, emitters=table, first_sample=3, pick=("grid", g), tally=d_odd, out=False)
                assert np.array_equal(t32(d_odd.cpu().numpy()), t32(want)), (which, form)
                assert odd[0].item() == 0 and not odd[1 + 2 * m:].any().item()
            monkeypatch.delenv("RB_GRID_TALLY")
    finally:
        e.close()


def test_pieces_below_64_surfels_and_a_forced_launch_shape():
    import torch
    s = _mesh()
    table = direct.scene_emitters(s)
    n = len(table)
    e = _engine(s)
    try:
        pts, nrm = mixed_surfels(e, s)
        g = box_of(pts, (3, 2, 2))
        tabs = direct.emitter_grid_cdf(table, g)
        ids = given_seeds(M)
        tp, tn = torch.from_numpy(pts).cuda(), torch.from_numpy(nrm).cuda()
        tids = torch.from_numpy(ids.view(np.int32)).cuda()
        # fewer than 64 surfels go in linear order: one surfel at many samples, 63, and 64 beside them
        for first, m, samples in ((0, 1, 64), (60, 63, 7), (60, 64, 7), (0, M, 5)):
            sl = slice(first, first + m)
            kept = np.zeros(12 * n, TALLY)
            got = e.direct_light(pts[sl], nrm[sl], samples, first_sample=2, seeds=ids[sl], pick=("grid", g), tally=kept)
            want_t, want_s = model_call(e, table, g, tabs, pts[sl], nrm[sl], samples, 2, ids[sl], abi.MASK_ALL)
            assert np.array_equal(kept, want_t), (first, m, samples)
            same_rows(got, want_s, (first, m, samples))
            d_kept = torch.zeros((12 * n, 2), dtype=torch.int32, device="cuda")
            assert e.direct_light(tp[sl], tn[sl], samples, first_sample=2, seeds=tids[sl], pick=("grid", g), tally=d_kept, out=False) is None
            assert np.array_equal(t32(d_kept.cpu().numpy()), t32(want_t)), (first, m, samples)
        whole = kept
        kept = np.zeros(12 * n, TALLY)
        assert len(e.direct_light(pts[:0], nrm[:0], 5, pick=("grid", g), tally=kept)) == 0 and not t32(kept).any()
        # the launch shape: reservations of 64 items on a grid of one block per CU
        o = _engine(s, queue_batch=64, blocks_per_cu=1)
        try:
            kept = np.zeros(12 * n, TALLY)
            o.direct_light(pts, nrm, 5, first_sample=2, seeds=ids, pick=("grid", g), tally=kept, out=False)
            assert np.array_equal(kept, whole), "forced shape"
        finally:
            o.close()
        for bad in (dict(tally=np.zeros(12 * n - 1, TALLY)), dict(tally=np.zeros(12 * n, u32)), dict(tally=np.zeros((12 * n, 2), np.int32))):
            with pytest.raises(ValueError):
                e.direct_light(pts, nrm, 1, pick=("grid", g), **bad)
    finally:
        e.close()


def test_a_call_across_a_piece_boundary():
    """RB_HEMI_PIECE_ITEMS + 77 * samples items at samples = 64 on the feature scene: two pieces add to the one device copy of
    the tally, which the host form uploads once and downloads once.  The whole call against two calls split at the boundary
    on one running tally, the surfels around the boundary against the model, both against the device form."""
    import torch
    samples = 64
    b = PIECE // samples
    n = b + 77
    s = scenes.feature_scene(width=24, height=16)
    table = direct.scene_emitters(s)
    N = len(table)
    e = _engine(s)
    try:
        p0, n0 = scene_surfels(e, s, 200)
        g = box_of(p0, (3, 1, 3))
        tabs = direct.emitter_grid_cdf(table, g)
        idx = np.arange(n) % 200
        pts, nrm = np.ascontiguousarray(p0[idx]), np.ascontiguousarray(n0[idx])
        ids = np.arange(n, dtype=u32)
        start = records(np.arange(9 * N, dtype=u32), np.arange(9 * N, dtype=u32) % 3)
        one = start.copy()
        sums = e.direct_light(pts, nrm, samples, first_sample=7, pick=("grid", g), tally=one)
        assert e.last_query_kernel_name() == "k_occl" and e.last_query_ms() > 0
        same_rows(sums, e.direct_light(pts, nrm, samples, first_sample=7, pick=("grid", g)), "the sums")
        two = start.copy()
        e.direct_light(pts[:b], nrm[:b], samples, first_sample=7, pick=("grid", g), tally=two, out=False)
        e.direct_light(pts[b:], nrm[b:], samples, first_sample=7, seeds=ids[b:], pick=("grid", g), tally=two, out=False)
        assert np.array_equal(one, two), "split"
        added = t32(one).astype(np.int64) - t32(start)
        assert (added >= 0).all() and added[0::2].sum() > 1000 * samples // 4
        tail = slice(b - 32, n)
        kept = np.zeros(9 * N, TALLY)
        e.direct_light(pts[tail], nrm[tail], samples, first_sample=7, seeds=ids[tail], pick=("grid", g), tally=kept, out=False)
        assert np.array_equal(kept, model_call(e, table, g, tabs, pts[tail], nrm[tail], samples, 7, ids[tail], abi.MASK_ALL)[0]), "tail"
        d_pts, d_nrm = (torch.from_numpy(a).to(f"cuda:{e.query_device}") for a in (pts, nrm))
        d_one = as_tensor(start)
        dev = e.direct_light(d_pts, d_nrm, samples, first_sample=7, emitters=table, pick=("grid", g), tally=d_one)
        same_rows(dev.cpu().numpy(), sums.view(f32).reshape(n, 4), "device")
        assert np.array_equal(t32(d_one.cpu().numpy()), t32(one)), "device"
    finally:
        e.close()


def test_sharded_engine_and_multi_device_handle():
    import torch
    s = scenes.feature_scene(width=24, height=16)
    table = direct.scene_emitters(s)
    e = _engine(s)
    pts, nrm = scene_surfels(e, s)
    g = box_of(pts, (3, 2, 2))
    want_t = np.zeros(12 * len(table), TALLY)
    want = e.direct_light(pts, nrm, 2, first_sample=7, pick=("grid", g), tally=want_t)
    learned = e.emitter_grid(g, tally=want_t, prior=1.0)
    want_l = model_call(e, table, g, learned, pts, nrm, 2, 7, None, abi.MASK_ALL)[0]
    e.close()
    assert want_t["tried"].sum() > 0 and np.array_equal(learned, direct.emitter_grid_cdf(table, g, want_t, 1.0))
    tp, tn = torch.from_numpy(pts).cuda(), torch.from_numpy(nrm).cuda()
    for kw in (dict(shard_rank=1, shard_count=3, stripe_rows=8), dict(devices=[0, 0], gather_peer_copy=True)):
        p = _engine(s, **kw)
        try:
            kept = np.zeros(len(want_t), TALLY)
            same_rows(p.direct_light(pts, nrm, 2, first_sample=7, pick=("grid", g), tally=kept), want, kw)
            assert np.array_equal(kept, want_t), kw
            assert np.array_equal(p.emitter_grid(g, tally=kept, prior=1.0), learned), kw
            assert p.last_query_kernel_name() == "k_grid_rows_seen"
            d_kept = torch.zeros((len(want_t), 2), dtype=torch.int32, device="cuda")
            h_kept = np.zeros(len(want_t), TALLY)
            host = p.direct_light(pts, nrm, 2, first_sample=7, pick=("grid", g, learned), tally=h_kept)
            same_rows(p.direct_light(tp, tn, 2, first_sample=7, pick=("grid", g, learned), tally=d_kept).cpu().numpy(),
                      host.view(f32).reshape(-1, 4), kw)
            assert p.last_query_kernel_name() == "k_occl" and p.last_query_ms() > 0
            # the device form's count under the learned tables: the host form's, and the model's
            assert np.array_equal(t32(d_kept.cpu().numpy()), t32(h_kept)) and h_kept["tried"].sum() > 0, kw
            assert np.array_equal(h_kept, want_l), kw
        finally:
            p.close()


# ---- 3. refusals
def test_refusals_leave_the_engine_rendering_the_golden_frame():
    import torch
    from renderbaby_amd._lib import load
    lib = load()
    s = scenes.cornell(32, 32, 2, 4)
    rc = RenderConfig.from_scene(s)
    e = Engine.new(rc, device=0)
    pts = np.array([(0.1 * i, 0.25, -3.0) for i in range(4)], f32)
    nrm = np.tile(f32([0, 1, 0]), (4, 1))
    surf = hemisphere.surfels(pts, nrm)
    tab = direct.scene_emitters(s)
    assert len(tab) == 2
    g = _grid()   # 2 x 2 x 2 cells
    tabs = direct.emitter_grid_cdf(tab, g[0])
    try:
        e.update(rc)
        h = e._h
        base = _params()
        before = e.direct_light(pts, nrm, 2, pick=("grid", g))
        assert (before["sum"] != 0).any()
        d_surf = torch.from_numpy(surf.view(f32).reshape(-1, 8)).cuda()
        d_tab = torch.from_numpy(tab.view(f32).reshape(-1, 16)).cuda()
        d_tabs = torch.from_numpy(tabs.view(np.int32)).cuda()
        out = np.full(64, 7, dtype=abi.RADIANCE)
        d_out = torch.full((64, 4), 7, dtype=torch.float32, device="cuda")
        d_new = torch.full((64,), 7, dtype=torch.int32, device="cuda")
        kept = np.full(64, 5, dtype=u32).view(TALLY)
        d_kept = torch.full((32, 2), 5, dtype=torch.int32, device="cuda")
        gp = g.ctypes.data
        for fn, tp, cp, sp, o, kp in ((lib.rb_direct_light_grid_tally, tab.ctypes.data, tabs.ctypes.data, surf.ctypes.data, out.ctypes.data, kept.ctypes.data),
                                      (lib.rb_direct_light_grid_tally_device, d_tab.data_ptr(), d_tabs.data_ptr(), d_surf.data_ptr(), d_out.data_ptr(),
                                       d_kept.data_ptr())):
            for name, kw in REFUSALS:
                args = dict(n=4, first_sample=0, samples=2, params=base, n_emit=2)
                args.update(kw)
                tail = (sp, None, args["n"], args["params"].ctypes.data, args["first_sample"], args["samples"])
                for t_, c_ in ((tp, cp), (tp, None), (None, None)):
                    assert fn(h, t_, gp, c_, args["n_emit"], *tail, o, kp) == INVALID_OPTIONS, name
                    assert fn(h, t_, gp, c_, args["n_emit"], *tail, None, kp) == INVALID_OPTIONS, name   # a training-only call too
                assert lib.rb_last_error(h)
            good = (sp, None, 4, base.ctypes.data, 0, 2)
            for name, kw in GRID_REFUSALS:
                assert fn(h, tp, _grid(**kw).ctypes.data, None, 2, *good, o, kp) == INVALID_OPTIONS, name
                assert fn(h, None, _grid(**kw).ctypes.data, None, 2, None, None, 0, base.ctypes.data, 0, 2, None, kp) == INVALID_OPTIONS, name
            for name, kw, n_emit in CAP_REFUSALS:
                assert fn(h, tp, _grid(**kw).ctypes.data, None, n_emit, *good, o, kp) == INVALID_OPTIONS, name
            assert fn(h, tp, gp, cp, 2, *good, o, None) == NULL_ARGUMENT and fn(h, tp, gp, cp, 2, *good, None, None) == NULL_ARGUMENT   # a NULL tally
            assert fn(h, None, gp, None, 2, None, None, 0, base.ctypes.data, 0, 2, None, None) == NULL_ARGUMENT   # ... in an empty call too
            assert fn(h, tp, None, cp, 2, *good, o, kp) == NULL_ARGUMENT                                               # a NULL grid
            assert fn(h, tp, gp, cp, 2, None, None, 4, base.ctypes.data, 0, 2, o, kp) == NULL_ARGUMENT
            assert fn(h, tp, gp, cp, 2, sp, None, 4, None, 0, 2, o, kp) == NULL_ARGUMENT
            for bad in (0, 1, 3):   # the scene's table under another count
                assert fn(h, None, gp, None, bad, *good, o, kp) == INVALID_OPTIONS, bad
            assert fn(h, None, gp, None, 2, None, None, 0, base.ctypes.data, 0, 2, None, kp) == 0   # an empty call
        # the device form's tally: in host memory, misaligned, in an allocation that ends before its records
        dev, bp = lib.rb_direct_light_grid_tally_device, base.ctypes.data
        good = (d_surf.data_ptr(), None, 4, bp, 0, 2, d_out.data_ptr())
        assert dev(h, d_tab.data_ptr(), gp, d_tabs.data_ptr(), 2, *good, kept.ctypes.data) == INVALID_OPTIONS
        assert dev(h, d_tab.data_ptr(), gp, d_tabs.data_ptr(), 2, *good, d_kept.data_ptr() + 2) == INVALID_OPTIONS
        assert dev(h, d_tab.data_ptr(), gp, None, 1 << 20, *good, d_kept.data_ptr()) == INVALID_OPTIONS   # allocations that end before their records
        assert dev(h, d_tab.data_ptr(), gp, d_tabs.data_ptr(), 2, d_surf.data_ptr(), None, 4, bp, 0, 2, out.ctypes.data, d_kept.data_ptr()) == INVALID_OPTIONS
        # the learned build's own refusals
        build = lib.rb_emitter_grid_learned_device
        for prior in BAD_PRIORS:
            assert build(h, d_tab.data_ptr(), 2, gp, d_kept.data_ptr(), prior, d_new.data_ptr()) == INVALID_OPTIONS, prior
            assert build(h, None, 2, gp, d_kept.data_ptr(), prior, d_new.data_ptr()) == INVALID_OPTIONS, prior
        for name, kw in GRID_REFUSALS:
            assert build(h, d_tab.data_ptr(), 2, _grid(**kw).ctypes.data, d_kept.data_ptr(), 1.0, d_new.data_ptr()) == INVALID_OPTIONS, name
        for name, kw, n_emit in CAP_REFUSALS:
            assert build(h, d_tab.data_ptr(), n_emit, _grid(**kw).ctypes.data, d_kept.data_ptr(), 1.0, d_new.data_ptr()) == INVALID_OPTIONS, name
        assert build(h, d_tab.data_ptr(), 2, None, d_kept.data_ptr(), 1.0, d_new.data_ptr()) == NULL_ARGUMENT
        assert build(h, d_tab.data_ptr(), 2, gp, None, 1.0, d_new.data_ptr()) == NULL_ARGUMENT
        assert build(h, d_tab.data_ptr(), 2, gp, d_kept.data_ptr(), 1.0, None) == NULL_ARGUMENT
        assert build(h, d_tab.data_ptr(), 2, gp, kept.ctypes.data, 1.0, d_new.data_ptr()) == INVALID_OPTIONS          # a host pointer
        assert build(h, d_tab.data_ptr(), 2, gp, d_kept.data_ptr() + 2, 1.0, d_new.data_ptr()) == INVALID_OPTIONS     # misaligned
        assert build(h, d_tab.data_ptr(), 1 << 20, gp, d_kept.data_ptr(), 1.0, d_new.data_ptr()) == INVALID_OPTIONS   # allocations that end before their records
        assert build(h, None, 3, gp, d_kept.data_ptr(), 1.0, d_new.data_ptr()) == INVALID_OPTIONS                     # not the scene's count
        lib.rb_sync(h)
        assert (out.view(u32) == f32(7).view(u32)).all() and (d_out == 7).all().item() and (d_new == 7).all().item()
        assert (kept.view(u32) == 5).all() and (d_kept == 5).all().item(), "a refused call wrote the tally"
        # after the refusals: the count and the sums, the learned build, the golden frame
        d_zero = torch.zeros((16, 2), dtype=torch.int32, device="cuda")
        assert dev(h, None, gp, None, 2, *good, d_zero.data_ptr()) == 0 and lib.rb_sync(h) == 0
        same_rows(d_out.cpu().numpy()[:4], before.view(f32).reshape(4, -1), "after the refusals")
        assert (d_out[4:] == 7).all().item()
        host = np.zeros(16, TALLY)
        same_rows(e.direct_light(pts, nrm, 2, pick=("grid", g), tally=host), before, "host, after the refusals")
        assert np.array_equal(t32(d_zero.cpu().numpy()), t32(host)) and host["tried"].sum() > 0
        assert build(h, None, 2, gp, d_zero.data_ptr(), 1.0, d_new.data_ptr()) == 0 and lib.rb_sync(h) == 0
        assert np.array_equal(d_new.cpu().numpy().view(u32)[:16], direct.emitter_grid_cdf(tab, g[0], host, 1.0)) and (d_new[16:] == 7).all().item()
        assert np.array_equal(e.render(rc).pixels, _oracle.render(s)[2])
    finally:
        e.close()
    cold = Engine.new(rc, device=0)   # no update yet: not ready, and still a refusal first
    try:
        kept = np.full(32, 5, dtype=u32).view(TALLY)
        call = lib.rb_direct_light_grid_tally
        assert call(cold._h, None, gp, None, 2, surf.ctypes.data, None, 4, base.ctypes.data, 0, 2, None, kept.ctypes.data) not in (0, INVALID_OPTIONS)
        assert call(cold._h, None, gp, None, 2, surf.ctypes.data, None, 4, base.ctypes.data, 0, 0, None, kept.ctypes.data) == INVALID_OPTIONS
        assert (kept.view(u32) == 5).all()
        assert np.array_equal(cold.render(rc).pixels, _oracle.render(s)[2])
    finally:
        cold.close()


# ---- 4. end to end
def two_lamps_and_a_wall():
    """Lamps of equal power at (4, 3, 0) and (-4, 3, 0) over the ground and a sphere of radius 1.2 at (-2, 1.5, 0), which hides
    the second lamp whole from every point within 0.4 of the origin"""
    s = scenes.spheres_scene(n=3, width=16, height=16, spp=1, max_depth=2)
    sp = s.spheres.copy()
    sp["center"], sp["radius"] = [(4, 3, 0), (-4, 3, 0), (-2, 1.5, 0)], (0.3, 0.3, 1.2)
    sp["material"]["emissive"] = [(30, 30, 30), (30, 30, 30), (0, 0, 0)]
    sp["material"]["diffuse"] = [(0, 0, 0), (0, 0, 0), (0.5, 0.5, 0.5)]
    return scenes.Scene(s.uniforms, sp, s.lights, s.meshes, s.bvh_nodes, s.bvh_indices, s.bvh_triangles, s.uvs, name="two lamps")


def test_a_lamp_behind_a_wall_loses_weight_and_the_mean_stays():
    """64 surfels of one cell train one round of 64 samples from sample 2^20 on.  The hidden lamp's q in that row falls below
    section 24's, the other row is section 24's still.  Then 64 x 256 items, one surfel per sample so that every item's value
    comes back, samples the training did not see: the learned mean within 4 combined standard errors of the uniform pick's."""
    s = two_lamps_and_a_wall()
    table = direct.scene_emitters(s)
    assert len(table) == 2 and (table["a"][:, 0] == (4, -4)).all()
    rng = np.random.default_rng(12)
    pts = np.stack([rng.uniform(0.05, 0.35, 64), np.zeros(64), rng.uniform(-0.2, 0.2, 64)], axis=1).astype(f32)
    nrm = np.tile(f32([0, 1, 0]), (64, 1))
    g = cells((-1, -1, -1), (1, 1, 1), (2, 1, 1))
    assert (direct.grid_cell(pts, g) == 1).all()
    e = _engine(s)
    try:
        base = e.emitter_grid(g)
        tabs, kept = bake.learn_grid(e, g, hemisphere.surfels(pts, nrm), 1, 64, prior=1.0)
        assert np.array_equal(base, direct.emitter_grid_cdf(table, g))
        assert not t32(kept[:2]).any() and kept["tried"][2] > 500 and kept["seen"][2] > 0.98 * kept["tried"][2]
        assert kept["tried"][3] > 500 and kept["seen"][3] == 0            # every ray towards the hidden lamp was blocked
        assert np.array_equal(tabs, direct.emitter_grid_cdf(table, g, kept, 1.0))
        q0, q1 = np.diff(base.reshape(2, 2), prepend=0, axis=1), np.diff(tabs.reshape(2, 2), prepend=0, axis=1)
        assert q1[1, 1] * 100 < q0[1, 1] and q1[1, 1] >= 1 and q1[1, 0] == q0[1, 0] and np.array_equal(q1[0], q0[0])
        P, N = np.repeat(pts, 256, axis=0), np.repeat(nrm, 256, axis=0)
        uni = e.direct_light(P, N, 1)
        lrn = e.direct_light(P, N, 1, pick=("grid", g, tabs))
        assert (uni["weight"] == 1).all() and (lrn["weight"] == 1).all()
        u, v = uni["sum"].astype(np.float64).mean(1), lrn["sum"].astype(np.float64).mean(1)
        se = np.hypot(u.std(ddof=1), v.std(ddof=1)) / np.sqrt(len(u))
        print(f"uniform {u.mean():.5f}, learned {v.mean():.5f}, {abs(u.mean() - v.mean()) / se:.2f} combined standard errors; "
              f"variance uniform / learned {u.var(ddof=1) / v.var(ddof=1):.2f}")
        assert u.mean() > 0 and abs(u.mean() - v.mean()) <= 4.0 * se
        # bake passes the pick through, training behind the rendered range
        mean = bake.direct_irradiance(e, pts, nrm, 16, pick=("learned", g, 1, 64))
        t2, _ = bake.learn_grid(e, g, hemisphere.surfels(pts, nrm), 1, 64, first_sample=16)
        assert np.array_equal(_u32(mean), _u32(bake.direct_irradiance(e, pts, nrm, 16, pick=("grid", g, t2))))
    finally:
        e.close()
