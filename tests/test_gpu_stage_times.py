"""The stage times an engine reports (rb_last_query_ms, rb_last_camera_rays_ms, rb_last_probe_project_ms,
rb_last_probe_depth_project_ms, rb_last_lightmap_ms, rb_last_denoise_ms, rb_last_reproject_ms), through one sequence of calls on
one engine: which call resets which time, which leaves it alone, and when a time that was not waited for is read.

Nothing here is compared with a clock: a time is 0, or above 0, or within another, or what it was bit for bit.
"""
import numpy as np
import pytest

from renderbaby_amd import abi, scenes
from renderbaby_amd._marshal import probe_records
from tests.conftest import has_gpu
from tests.test_gpu_query import _engine
from tests.test_probe_light_abi import INVALID_OPTIONS

pytestmark = [pytest.mark.gpu, pytest.mark.skipif(not has_gpu(), reason="needs a GPU")]

f32 = np.float32
PROBES, SAMPLES, REACH = 130, 4, 10.0


def times(e):
    """every stage time of `e`: query, generator, SH projection, depth projection, surfels, resolve, filter, guides, history"""
    return (e.last_query_ms(), e.last_camera_rays_ms(), e.last_probe_project_ms(), e.last_probe_depth_project_ms(),
            *e.last_lightmap_ms(), *e.last_denoise_ms(), e.last_reproject_ms())


def bits(ts):
    return np.asarray(ts, f32).view(np.uint32).tolist()


def box_points(n):
    """n points in the free space of the Cornell box (a few may lie inside a sphere: their rays are rays all the same)"""
    rng = np.random.default_rng(11)
    return np.ascontiguousarray(rng.uniform((-1.0, 1.0, -4.0), (1.0, 4.0, -2.0), size=(n, 3)).astype(f32))


def refused_call_leaves_the_times(e, pos):
    """a query refused in its argument check (samples = 0) has not come as far as the prologue: every time reads as before"""
    before = times(e)
    out = np.zeros(len(pos), dtype=abi.PROBE_DEPTH)
    rec = probe_records(pos)
    assert e._lib.rb_bake_probe_depth(e._h, rec.ctypes.data, None, len(rec), 0, 0, REACH, out.ctypes.data) == INVALID_OPTIONS
    assert bits(times(e)) == bits(before)


def test_one_engine_through_every_stage(monkeypatch):
    import torch
    s = scenes.cornell(32, 32, 1, 4)
    e = _engine(s)
    try:
        # 1. a fresh engine after an update
        assert times(e) == (0,) * 9 and e.last_query_kernel_name() == ""

        # 2. the depth bake in the host form, three pieces: 64 + 64 + 2 probes (a piece is whole blocks of 64)
        monkeypatch.setenv("RB_DEPTH_PIECE_ITEMS", "256")
        pos = box_points(PROBES)
        host = e.bake_probe_depth(pos, SAMPLES, REACH)
        q, gen, sh, depth = times(e)[:4]
        print("host form:", q, gen, sh, depth)
        assert q > 0 and 0 < gen <= q and 0 < depth <= q and sh == 0
        assert e.last_query_kernel_name().startswith("k_query")

        # 3. the same call in the device form, and nothing between it and the getters: no rb_sync, no copy.  The first read of
        # a time waits for its events (a read that did not would find them not ready and fail); the second has it
        rec = probe_records(pos)
        d_pos = torch.from_numpy(rec.view(f32).reshape(PROBES, 4)).cuda()
        d_out = torch.zeros((PROBES, 256), dtype=torch.float32, device="cuda")
        torch.cuda.synchronize()
        assert e._lib.rb_bake_probe_depth_device(e._h, d_pos.data_ptr(), None, PROBES, 0, SAMPLES, REACH, d_out.data_ptr()) == 0
        for getter in (e.last_query_ms, e.last_camera_rays_ms, e.last_probe_depth_project_ms):
            first, second = getter(), getter()
            print("device form:", getter.__name__, first, second)
            assert first > 0 and bits([first]) == bits([second])
        assert e.last_probe_project_ms() == 0
        assert 0 < e.last_camera_rays_ms() <= e.last_query_ms() and 0 < e.last_probe_depth_project_ms() <= e.last_query_ms()
        # (the query's time was waited for, so its results stand)
        assert np.array_equal(d_out.cpu().numpy().view(np.uint32), host.view(f32).reshape(PROBES, 256).view(np.uint32))
        monkeypatch.delenv("RB_DEPTH_PIECE_ITEMS")
        refused_call_leaves_the_times(e, pos)

        # 4. a query without a generator
        e.occluded(pos, np.tile(f32([0, 1, 0]), (PROBES, 1)))
        q, gen, sh, depth = times(e)[:4]
        assert q > 0 and (gen, sh, depth) == (0, 0, 0)

        # 5. the lightmap's times are a lightmap call's: a query after it leaves them
        surf = torch.empty((64, 8), dtype=torch.float32, device="cuda")
        own = torch.empty((64,), dtype=torch.int32, device="cuda")
        e.lightmap_surfels(8, 8, out=(surf, own))
        sm, rm = e.last_lightmap_ms()
        assert 0 < sm <= e.last_query_ms() and rm == 0
        e.cast_rays(pos, np.tile(f32([0, -1, 0]), (PROBES, 1)))
        assert e.last_query_kernel_name().startswith("k_query") and e.last_query_ms() > 0
        assert bits(e.last_lightmap_ms()) == bits((sm, 0))

        # 6. a query refused in its argument check
        refused_call_leaves_the_times(e, pos)

        # 7. the denoiser twice without an update between: the first call builds the guides, the second has them
        e.render_current()
        e.denoise()
        ms, guide_ms = e.last_denoise_ms()
        assert ms > 0 and guide_ms > 0
        e.denoise()
        ms, guide_ms = e.last_denoise_ms()
        assert ms > 0 and guide_ms == 0
        assert e.last_reproject_ms() == 0

        # 8. the history step's time is a denoise_history's: a reset and a plain denoise leave it
        e.denoise_history()
        rp = e.last_reproject_ms()
        assert rp > 0 and e.last_denoise_ms()[0] > 0
        e.history_reset()
        e.denoise()
        assert bits([e.last_reproject_ms()]) == bits([rp])
    finally:
        e.close()

    # 9. a multi-device handle (two parts on one device): the query's times are part 0's, the denoiser's its own -- it refuses
    # such a handle, so they read 0
    g = _engine(s, devices=[0, 0], gather_peer_copy=True)
    try:
        g.bake_probe_depth(pos[:5], SAMPLES, REACH)
        assert g.last_query_ms() > 0 and 0 < g.last_camera_rays_ms() <= g.last_query_ms()
        assert g.last_denoise_ms() == (0, 0) and g.last_reproject_ms() == 0
    finally:
        g.close()
