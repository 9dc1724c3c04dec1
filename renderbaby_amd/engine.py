"""Host-side mirror of the reference's renderer interface over the C ABI.

Names and semantics follow the reference so parity tests read like its own code:

* ``Change`` / ``RenderConfig`` / ``RenderConfigBuilder`` --
  crates/engine-config/src/render_config.rs:37-57,99-109,312-606
* ``Engine.new(rc)`` / ``Engine.render(rc)`` / ``Engine.frame_iterator(rc)`` --
  ``impl Renderer for Engine``, crates/engine-pathtracer/src/lib.rs:58-119
* ``Frame`` / ``FrameIterator.has_next/next/destroy`` --
  crates/frame-buffer/src/frame_iterator.rs:3-51

Everything that computes is in librenderbaby_hip.so; this file only marshals.
"""
import ctypes as C
from dataclasses import dataclass
from functools import partial
from typing import Any, List, Optional

import numpy as np

from . import abi
from ._lib import load
from .bvh import own_tree_readback, sphere_tree_readback
from ._marshal import (CDF, SEEDS, Form, device_new, device_tensor, download, grid_records, host_in, host_out, host_ptr, is_tensor, probe_records,
                       ray_records, surfel_records, torch_device, upload)


class RenderError(RuntimeError):
    """anyhow::Error of the reference; ``code`` is the rb_abi.h status."""

    def __init__(self, code, message):
        super().__init__(f"[{abi.ERR.get(code, code)}] {message}")
        self.code = code
        self.message = message


@dataclass
class Change:
    """``enum Change<T> { Keep, Create(T), Update(T), Delete }``"""
    tag: int
    value: Any = None

    @staticmethod
    def keep():
        return Change(abi.KEEP)

    @staticmethod
    def create(v):
        return Change(abi.CREATE, v)

    @staticmethod
    def update(v):
        return Change(abi.UPDATE, v)

    @staticmethod
    def delete():
        return Change(abi.DELETE)


_FIELDS = ("uniforms", "spheres", "uvs", "meshes", "lights", "bvh_nodes", "bvh_indices", "bvh_triangles",
           "textures")
_DTYPES = {"uniforms": abi.UNIFORMS, "spheres": abi.SPHERE, "uvs": np.float32, "meshes": abi.MESH,
           "lights": abi.POINT_LIGHT, "bvh_nodes": abi.BVH_NODE, "bvh_indices": np.uint32,
           "bvh_triangles": abi.GPU_TRIANGLE}


class RenderConfig:
    """``struct RenderConfig`` -- nine ``Change`` fields, default Keep."""

    def __init__(self, **kw):
        for f in _FIELDS:
            setattr(self, f, kw.get(f, Change.keep()))

    @staticmethod
    def builder():
        return RenderConfigBuilder()

    @staticmethod
    def from_scene(scene, create=True, with_tree=True):
        """What generate_full_render_command_builder emits
        (scene_engine_adapter.rs:463-490): all ``*_create`` on the first render;
        afterwards Update for everything except the three BVH fields, which stay Create.
        ``with_tree=False``: bvh_nodes and bvh_indices are Keep -- for an engine that builds the tree itself
        (``Engine(..., build_tree=...)``)."""
        mk = Change.create if create else Change.update
        return RenderConfig(
            uniforms=mk(scene.uniforms), spheres=mk(scene.spheres), uvs=mk(scene.uvs), meshes=mk(scene.meshes),
            lights=mk(scene.lights), bvh_nodes=Change.create(scene.bvh_nodes) if with_tree else Change.keep(),
            bvh_indices=Change.create(scene.bvh_indices) if with_tree else Change.keep(),
            bvh_triangles=Change.create(scene.bvh_triangles), textures=mk(scene.textures))

    # ---- marshalling
    def to_c(self):
        """Returns (abi.Config, keepalive list)."""
        cfg = abi.Config()
        keep: List[Any] = []
        for f in _FIELDS:
            ch: Change = getattr(self, f)
            fld = abi.Field()
            fld.change = ch.tag
            fld.ptr = None
            fld.count = 0
            if ch.tag in (abi.CREATE, abi.UPDATE):
                if f == "textures":
                    texs = ch.value or []
                    arr = (abi.Texture * max(len(texs), 1))()
                    for i, (w, h, data) in enumerate(texs):
                        d = np.ascontiguousarray(data, dtype=np.uint32)
                        keep.append(d)
                        arr[i].width, arr[i].height, arr[i].rgba_data = int(w), int(h), d.ctypes.data
                    keep.append(arr)
                    fld.ptr = C.cast(arr, C.c_void_p).value if texs else None
                    fld.count = len(texs)
                else:
                    a = np.ascontiguousarray(np.atleast_1d(ch.value), dtype=_DTYPES[f])
                    keep.append(a)
                    fld.ptr = host_ptr(a)
                    fld.count = a.size
            setattr(cfg, f, fld)
        return cfg, keep


class RenderConfigBuilder:
    """``RenderConfigBuilder``: ``x(v)`` = Update, ``x_create(v)``, ``x_no_change()``, ``x_delete()``."""

    def __init__(self):
        self._rc = RenderConfig()

    def build(self):
        return self._rc


def _add_builder_methods():
    for f in _FIELDS:
        def upd(self, v, _f=f):
            setattr(self._rc, _f, Change.update(v))
            return self

        def cre(self, v, _f=f):
            setattr(self._rc, _f, Change.create(v))
            return self

        def keep(self, _f=f):
            setattr(self._rc, _f, Change.keep())
            return self

        def dele(self, _f=f):
            setattr(self._rc, _f, Change.delete())
            return self
        setattr(RenderConfigBuilder, f, upd)
        setattr(RenderConfigBuilder, f + "_create", cre)
        setattr(RenderConfigBuilder, f + "_no_change", keep)
        setattr(RenderConfigBuilder, f + "_delete", dele)


_add_builder_methods()


@dataclass
class Frame:
    """``struct Frame { width, height, pixels: Vec<u8> }`` (RGBA8, x mirrored, A = 255)."""
    width: int
    height: int
    pixels: np.ndarray  # uint8, (height, width, 4)

    def expected_size(self):
        return self.width * self.height * 4

    def validate(self):
        if self.pixels.size != self.expected_size():
            raise RenderError(0, f"Frame pixel size mismatch: expected {self.expected_size()} bytes, got {self.pixels.size}")


def _sample_range(samples, first_sample):
    """(samples, first_sample) as the 32-bit unsigned numbers the ABI takes"""
    samples, first_sample = int(samples), int(first_sample)
    if not (0 <= samples < 2 ** 32 and 0 <= first_sample < 2 ** 32):
        raise ValueError("samples and first_sample are 32-bit unsigned numbers")
    return samples, first_sample


def _global_error():
    """the library's message for a call without an engine (comm_*, the engine-less forms, a create that failed)"""
    return (load().rb_last_error(None) or b"").decode()


def _check_global(rc):
    """raise the RenderError of a call without an engine that returned `rc`"""
    if rc != abi.RB_OK:
        raise RenderError(rc, _global_error())


_HOST = Form(None)   # the form of the engine-less calls: host arrays only


def _engineless(device):
    """(form, call) of an engine-less form on `device`: call(name, *args) makes the library's call and raises its error"""
    lib = load()
    return _HOST, lambda name, *args: _check_global(getattr(lib, name)(int(device), *args))


def _camera_region(cam, region):
    """(abi.CAMERA_EX[1], first_pixel, n_pixels) of a camera and a ``region`` of its image, by default all of it"""
    c = np.ascontiguousarray(cam, dtype=abi.CAMERA_EX).reshape(1)
    first, n = (0, int(c["width"][0]) * int(c["height"][0])) if region is None else (int(region[0]), int(region[1]))
    if first < 0 or n < 0:
        raise ValueError("region: (first_pixel, n_pixels), both at least 0")
    return c, first, n


def _visibility(normal_bias, min_visibility, wrap, depth):
    """abi.LIGHT_VISIBILITY[1] of light_points_visible's parameters"""
    from .probes import visibility_params
    return np.array([visibility_params(normal_bias, min_visibility, wrap, depth)], dtype=abi.LIGHT_VISIBILITY)


def _probe_stage(f, call, name, dtype, what, src, out=None, share=False):
    """a per-probe stage in the form `f`, made by `call` (Engine._staged or _engineless): the records `src` (`what` names the
    argument) -> ``out``, and with ``share`` one float32 per probe beside it"""
    if f.tensors and not is_tensor(src):
        raise ValueError(f"{what}: a tensor is needed beside a tensor out")
    src, sp = f.input(what, src, dtype)
    n = len(src)
    res, op = f.output("out", out, dtype, n)
    if not share:
        call(name, sp, n, op)
        return f.result(res, dtype)
    per_probe, pp = f.output("share", None, np.float32, n)
    call(name, sp, n, op, pp)
    return f.result(res, dtype), f.result(per_probe, np.float32)


def _light_points(f, call, grid, coeffs, points, normals, out=None, moments=None, visibility=None):
    """light_points, and with ``visibility`` (an abi.LIGHT_VISIBILITY[1]) light_points_visible, in the form `f`, made by `call`"""
    g, cells = grid_records(grid)
    coeffs, cp = f.input("coeffs", coeffs, abi.SH9, cells)
    moments, mp = f.optional("moments", moments, abi.PROBE_DEPTH, cells)
    surf, pp = f.input("points", surfel_records(points, normals), abi.SURFEL)
    m = len(surf)
    res, op = f.output("out", out, abi.LIT, m)
    if visibility is None:
        call("rb_light_points", g.ctypes.data, cp, pp, m, op)
    else:
        call("rb_light_points_visible", g.ctypes.data, cp, mp, pp, m, visibility.ctypes.data, op)
    return f.result(res, abi.LIT)


class Engine:
    """``engine_pathtracer::Engine`` for the HIP backend."""

    def __init__(self, rc: RenderConfig, device=-1, shard_rank=0, shard_count=1, stripe_rows=0,
                 passes_per_launch=0, kernel=abi.KERNEL_DEFAULT, stats=False, blocks_per_cu=0, color_budget_mib=0,
                 no_sphere_bvh=False, fast_bvh=False, lds_mode=0, device_bvh=False, no_leaf_stepping=False,
                 device_lbvh=False, reference_walk=False, host_bvh=False, devices=None, gather_peer_copy=False,
                 no_run_ahead=False, own_tree=False, skip_near_degenerate=False, queue_batch=0, chunk_walk=False,
                 sphere_tree=None, chunk_tree=None, build_tree=None):
        """``devices`` (list of HIP ordinals): one handle over several devices of this process
        (rb_create_multi): rows sharded in stripes, one RCCL gather per delivered frame.
        ``build_tree`` ("device" | "host"): the engine builds the reference-layout tree from the triangles itself
        (RB_FLAG_BUILD_TREE): send configs with ``RenderConfig.from_scene(scene, with_tree=False)``."""
        self._lib = load()
        cfg, keep = rc.to_c()
        self.uniforms = None   # set by the first update that succeeds (_remember)
        opt = abi.Options()
        opt.device = device
        opt.shard_rank, opt.shard_count, opt.stripe_rows = shard_rank, shard_count, stripe_rows
        opt.passes_per_launch = passes_per_launch
        opt.kernel = kernel
        # fast_bvh / host_bvh: the library's own tree, built on the host; device_bvh / device_lbvh: built on the
        # device; own_tree: the library's tree with the builder left to the library (by triangle count)
        host_bvh = host_bvh or fast_bvh
        own_tree = own_tree or host_bvh or device_bvh or device_lbvh
        opt.flags = (abi.FLAG_STATS if stats else 0) | (abi.FLAG_NO_SPHERE_BVH if no_sphere_bvh else 0) \
            | (abi.FLAG_FAST_BVH if own_tree else 0) | (abi.FLAG_DEVICE_BVH if (device_bvh or device_lbvh) else 0) \
            | (abi.FLAG_DEVICE_LBVH if device_lbvh else 0) | (abi.FLAG_REFERENCE_WALK if reference_walk else 0) \
            | (abi.FLAG_HOST_BVH if host_bvh else 0) | (abi.FLAG_GATHER_PEER_COPY if gather_peer_copy else 0) \
            | (abi.FLAG_NO_RUN_AHEAD if no_run_ahead else 0) | (abi.FLAG_SKIP_NEAR_DEGENERATE if skip_near_degenerate else 0) \
            | (abi.FLAG_CHUNK_WALK if chunk_walk else 0) \
            | {None: 0, "host": abi.FLAG_SPHERE_TREE_HOST, "device": abi.FLAG_SPHERE_TREE_DEVICE}[sphere_tree] \
            | {None: 0, "host": abi.FLAG_CHUNK_TREE_HOST, "device": abi.FLAG_CHUNK_TREE_DEVICE}[chunk_tree] \
            | {None: 0, "host": abi.FLAG_BUILD_TREE_HOST, "device": abi.FLAG_BUILD_TREE}[build_tree]   # who builds the chunked walk's tree / the reference-layout tree
        opt._reserved[0] = blocks_per_cu
        opt._reserved[1] = color_budget_mib
        opt._reserved[2] = queue_batch   # items a wave reserves per queue atomic (0 = the launcher's choice)
        opt._reserved[3] = 1 if no_leaf_stepping else 0   # ablation: per-segment traversal for multi-node trees
        opt._reserved[4] = int(lds_mode)   # LDS staging of small meshes: 0 = when it fits, 1 = never
        # who answers queries: devices[0], `device`, or for -1 the device that is current now, which is the one the library
        # takes in rb_create_ex just below (hipGetDevice of the one HIP runtime of this process)
        self.query_device = int(devices[0]) if devices is not None else int(device)
        if self.query_device < 0:
            cur = C.c_int(-1)
            if self._lib.hipGetDevice(C.byref(cur)) != 0 or cur.value < 0:
                raise RenderError(abi.RB_ERR_DEVICE, "device=-1: hipGetDevice names no current device")
            self.query_device = cur.value
        if devices is not None:
            devs = (C.c_int32 * len(devices))(*[int(d) for d in devices])
            self._h = self._lib.rb_create_multi(C.byref(cfg), C.byref(opt), devs, len(devices))
        else:
            self._h = self._lib.rb_create_ex(C.byref(cfg), C.byref(opt))
        del keep
        if not self._h:   # no handle to ask: the device error code with the library's message
            raise RenderError(abi.RB_ERR_DEVICE, _global_error() or "rb_create failed")
        self.shard_count = max(shard_count, 1)
        self.comm_rank = None   # set by comm_init_rank: rank 0 then receives whole frames

    @classmethod
    def new(cls, rc, **kw):
        return cls(rc, **kw)

    def close(self):
        if getattr(self, "_h", None):
            self._lib.rb_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def _remember(self, rc):
        """the uniforms the engine last accepted (abi.UNIFORMS[1]; called after the update succeeded): the camera of the pixel-centre rays, for aov.ambient_occlusion"""
        if rc.uniforms.tag in (abi.CREATE, abi.UPDATE):
            self.uniforms = np.array(np.atleast_1d(rc.uniforms.value), dtype=abi.UNIFORMS).reshape(-1)[:1].copy()

    def _check(self, rc):
        if rc != abi.RB_OK:
            raise RenderError(rc, (self._lib.rb_last_error(self._h) or b"").decode())

    # ---- Renderer
    def update(self, rc: RenderConfig):
        cfg, keep = rc.to_c()
        self._check(self._lib.rb_update(self._h, C.byref(cfg)))
        self._remember(rc)
        del keep

    def size(self):
        w, h = C.c_uint32(), C.c_uint32()
        self._check(self._lib.rb_get_size(self._h, C.byref(w), C.byref(h)))
        return w.value, h.value

    def _frame_shape(self):
        w, h = self.size()
        if self.shard_count > 1 and self.comm_rank is None:
            h = self.local_rows()[1]
        return w, h

    # ---- one process per device: the stripes are gathered to rank 0 inside rb_render / rb_iter_next
    @staticmethod
    def comm_available():
        """Raises unless this process can load RCCL (no communicator id is made: rb_comm_available)."""
        _check_global(load().rb_comm_available())

    @staticmethod
    def comm_unique_id() -> bytes:
        buf = (C.c_uint8 * abi.COMM_ID_BYTES)()
        _check_global(load().rb_comm_unique_id(buf))
        return bytes(buf)

    def comm_init_rank(self, comm_id: bytes, rank: int, nranks: int):
        buf = (C.c_uint8 * abi.COMM_ID_BYTES).from_buffer_copy(comm_id)
        self._check(self._lib.rb_comm_init_rank(self._h, buf, rank, nranks))
        self.comm_rank = rank

    def comm_info(self):
        """{"rccl_ranks", "rccl_rank", "gather_ms"}: the communicator as RCCL itself reports it (0 ranks when the
        exchange does not go through RCCL) and this rank's share of the last gather."""
        n, r, ms = C.c_uint32(), C.c_uint32(), C.c_float()
        self._check(self._lib.rb_comm_info(self._h, C.byref(n), C.byref(r), C.byref(ms)))
        return {"rccl_ranks": n.value, "rccl_rank": r.value, "gather_ms": ms.value}

    def render(self, rc: RenderConfig) -> Frame:
        self.update(rc)
        return self.render_current()

    def render_current(self) -> Frame:
        """rb_render without an update: all passes of the scene the engine already holds."""
        w, h = self._frame_shape()
        if self.comm_rank not in (None, 0):   # a non-root rank of a process group: its stripes go to rank 0
            self._check(self._lib.rb_render(self._h, None))
            return None
        out = np.empty((h, w, 4), dtype=np.uint8)
        self._check(self._lib.rb_render(self._h, out.ctypes.data))
        return Frame(w, h, out)

    def frame_iterator(self, rc: RenderConfig, passes_per_frame: int = 1) -> "FrameIterator":
        """``passes_per_frame`` > 1 (extension): one frame per that many samples instead of per sample."""
        cfg, keep = rc.to_c()
        self._check(self._lib.rb_iter_begin(self._h, C.byref(cfg)))
        self._remember(rc)
        del keep
        self._check(self._lib.rb_iter_set_passes_per_frame(self._h, passes_per_frame))
        return FrameIterator(self)

    # ---- lower-level control (bench, tests, multi-GPU)
    def clear(self):
        self._check(self._lib.rb_clear(self._h))

    def dispatch(self, first_pass, n_passes):
        self._check(self._lib.rb_dispatch(self._h, first_pass, n_passes))

    def reserve(self, n_passes):
        """rb_reserve: what a dispatch of n_passes passes would allocate lazily (no tracing)."""
        self._check(self._lib.rb_reserve(self._h, n_passes))

    def sync(self):
        self._check(self._lib.rb_sync(self._h))

    def read_rgba(self):
        w, h = self._frame_shape()
        out = np.empty((h, w, 4), dtype=np.uint8)
        self._check(self._lib.rb_read_rgba(self._h, out.ctypes.data))
        return out

    def read_accumulation(self):
        w, h = self._frame_shape()
        out = np.empty((h, w, 4), dtype=np.float32)
        self._check(self._lib.rb_read_accumulation(self._h, out.ctypes.data))
        return out

    def device_rgba(self):
        p, n = C.c_void_p(), C.c_size_t()
        self._check(self._lib.rb_device_rgba(self._h, C.byref(p), C.byref(n)))
        return p.value, n.value

    def local_rows(self):
        r, pr = C.c_uint32(), C.c_uint32()
        self._check(self._lib.rb_local_rows(self._h, C.byref(r), C.byref(pr)))
        return r.value, pr.value

    def global_row(self, local_row):
        g = C.c_uint32()
        self._check(self._lib.rb_global_row(self._h, local_row, C.byref(g)))
        return g.value

    def stats(self):
        s = abi.Stats()
        self._check(self._lib.rb_get_stats(self._h, C.byref(s)))
        return s.as_dict()

    def reset_stats(self):
        self._check(self._lib.rb_reset_stats(self._h))

    def last_kernel_name(self):
        return (self._lib.rb_last_kernel_name(self._h) or b"").decode()

    def trace_form(self):
        """abi.TRACE_FORM_* bits of the k_trace instantiation the last render ran (rb_debug_trace_form)"""
        return int(self._lib.rb_debug_trace_form(self._h))

    def tri_filter_masks(self, origins, directions):
        """rb_debug_tri_filter: the sift's candidate bits of n rays -> (bool [slots of the node's list][n], first slot)"""
        rays = np.ascontiguousarray(np.concatenate([np.asarray(origins, np.float32), np.asarray(directions, np.float32)], axis=1))
        out, lst = np.zeros((len(rays), 4), np.uint32), np.zeros(2, np.uint32)
        self._check(self._lib.rb_debug_tri_filter(self._h, rays.ctypes.data, len(rays), out.ctypes.data, lst.ctypes.data))
        bits = (out[:, :, None] >> np.arange(32, dtype=np.uint32)) & 1
        return bits.reshape(len(rays), 128)[:, :int(lst[1] - lst[0])].T.astype(bool), int(lst[0])

    # ---- the queries (rb_abi.h): every array argument goes through _marshal.Form, every call through _query
    _ray_records = staticmethod(ray_records)

    def _device_call(self, fn, *args):
        """a device form between torch's stream and the engine's: torch's queued work first, rb_sync after"""
        import torch
        torch.cuda.current_stream(self.query_device).synchronize()
        self._check(fn(self._h, *args))
        self._check(self._lib.rb_sync(self._h))

    def _query(self, form, name, *args):
        """the call of a query in the form `form`: the entry point `name`, or ``name_device`` as _device_call makes it"""
        if form.on_device:
            self._device_call(getattr(self._lib, name + "_device"), *args)
        else:
            self._check(getattr(self._lib, name)(self._h, *args))

    def _staged(self, *arrays):
        """(form, call) of a query over `arrays` that has a device form only (_marshal.Form's ``staged``)"""
        f = Form(self.query_device, *arrays, staged=True)
        return f, partial(self._query, f)

    def _last_ms(self, fn, count=1):
        """the `count` float32 milliseconds the getter `fn` reports: one as a float, several as a tuple"""
        ms = [C.c_float() for _ in range(count)]
        self._check(fn(self._h, *[C.byref(m) for m in ms]))
        return ms[0].value if count == 1 else tuple(m.value for m in ms)

    def _builder(self, fn):
        """(name, build milliseconds) as the getter `fn` reports them"""
        ms = C.c_float()
        name = (fn(self._h, C.byref(ms)) or b"").decode()
        return name, ms.value

    # ---- closest-hit queries (rb_abi.h)
    def cast_rays(self, origins, dirs, surfaces=False, hits_out=None, surfaces_out=None):
        """rb_cast_rays: (n, 3) origins and directions (any length: the device normalises) -> abi.HIT[n], or
        (abi.HIT[n], abi.SURFACE[n]) with ``surfaces``.  ``hits_out`` / ``surfaces_out``: arrays to fill instead of new
        ones (page-locked ones are filled by DMA): contiguous abi.HIT[n] / abi.SURFACE[n], anything else is a ValueError."""
        return self.cast_ray_records(ray_records(origins, dirs), surfaces, hits_out, surfaces_out)

    def cast_ray_records(self, rays, surfaces=False, hits_out=None, surfaces_out=None):
        """rb_cast_rays on an abi.RAY array as it stands (no copy when it is contiguous).  A float32 tensor of shape (n, 8) on
        the engine's device goes to rb_cast_rays_device instead: the records come back as float32 tensors of shape (n, 12) on
        the device (``.cpu().numpy().view(abi.HIT)`` names their fields), and nothing crosses to the host.  A ``hits_out`` or
        ``surfaces_out`` that is not n contiguous records of its dtype is a ValueError in either form."""
        f = Form(self.query_device, rays, hits_out, surfaces_out)
        rays, rp = f.input("rays", rays, abi.RAY, flat=False)
        n = len(rays)
        hits, hp = f.output("hits_out", hits_out, abi.HIT, n)
        surf, sp = f.output("surfaces_out", surfaces_out, abi.SURFACE, n) if (surfaces or surfaces_out is not None) else (None, None)
        self._query(f, "rb_cast_rays", rp, n, hp, sp)
        return hits if surf is None else (hits, surf)

    # ---- any-hit occlusion (rb_abi.h)
    def occluded(self, origins, dirs, tmax=None, mask=abi.MASK_ALL, out=None):
        """rb_occluded: is anything within (0.001, tmax) along each ray, among the stages of ``mask``?  (n, 3) origins and
        directions (any length: the device normalises), ``tmax`` n float32 or None (no bound) -> uint8[n] of abi.OCCL_*.
        Torch tensors on the engine's device go to rb_occluded_device and a uint8 tensor on the device comes back."""
        return self.occluded_records(ray_records(origins, dirs), tmax, mask, out)

    def occluded_records(self, rays, tmax=None, mask=abi.MASK_ALL, out=None):
        """rb_occluded on an abi.RAY array, or rb_occluded_device on a float32 tensor of shape (n, 8)."""
        f = Form(self.query_device, rays, tmax, out)
        rays, rp = f.input("rays", rays, abi.RAY, flat=False)
        n = len(rays)
        tmax, tp = f.optional("tmax", tmax, np.float32, n)
        res, op = f.output("out", out, np.uint8, n)
        self._query(f, "rb_occluded", rp, tp, n, int(mask), op)
        return res

    # ---- path-traced radiance along given rays (rb_abi.h)
    def trace_rays(self, origins, dirs, seeds=None, samples=1, first_sample=0, out=None):
        """rb_trace_rays: the radiance trace_ray returns along each ray, summed over ``samples`` samples in sample order.
        (n, 3) origins and directions (any length: the device normalises), ``seeds`` n uint32 ids or None (the ray's index)
        -> abi.RADIANCE[n] (``sum``, ``weight`` = samples; an invalid ray: zeros).  Torch tensors on the engine's device go
        to rb_trace_rays_device and an (n, 4) float32 tensor on the device comes back."""
        return self.trace_ray_records(ray_records(origins, dirs), seeds, samples, first_sample, out)

    def trace_ray_records(self, rays, seeds=None, samples=1, first_sample=0, out=None):
        """rb_trace_rays on an abi.RAY array, or rb_trace_rays_device on a float32 tensor of shape (n, 8) (``seeds``: an int32
        or uint32 tensor of n elements, its bits are the ids; ``out``: a float32 tensor of shape (n, 4))."""
        samples, first_sample = _sample_range(samples, first_sample)
        f = Form(self.query_device, rays, seeds, out)
        if not f.on_device and not isinstance(rays, np.ndarray):
            raise ValueError("rays: an abi.RAY array, or a float32 tensor of ray records, is needed")
        rays, rp = f.input("rays", rays, abi.RAY, flat=False)
        n = len(rays)
        seeds, sp = f.optional("seeds", seeds, SEEDS, n)
        res, op = f.output("out", out, abi.RADIANCE, n)
        self._query(f, "rb_trace_rays", rp, sp, n, first_sample, samples, op)
        return res

    # ---- camera rays made on the device (rb_abi.h)
    def trace_camera(self, cam, samples, first_sample=0, region=None, out=None):
        """rb_trace_camera: the radiance through an abi.CAMERA_EX camera (``camera.make``), every (pixel, sample) ray made on
        the device from its own random stream, summed over ``samples`` samples -> abi.RADIANCE[n] (``weight``: the valid
        samples).  ``region``: (first_pixel, n_pixels) of the row-major image, by default all of it.  ``out``: an
        abi.RADIANCE array of n elements to fill, or a float32 tensor of shape (n, 4) on the engine's device, which selects
        rb_trace_camera_device (nothing crosses to the host)."""
        c, first, n = _camera_region(cam, region)
        samples, first_sample = _sample_range(samples, first_sample)
        f = Form(self.query_device, out)
        res, op = f.output("out", out, abi.RADIANCE, n)
        self._query(f, "rb_trace_camera", c.ctypes.data, first, n, first_sample, samples, op)
        return res

    # ---- hemisphere rays made on the device (rb_abi.h)
    @staticmethod
    def _hemi_params(offset, radius=0.0, mask=0):
        prm = np.zeros(1, dtype=abi.HEMI_PARAMS)
        prm["offset"], prm["radius"], prm["mask"] = offset, radius, int(mask)
        return prm

    def _hemisphere(self, name, out_dtype, points, normals, samples, first_sample, seeds, prm, out):
        """the two forms of a hemisphere query: surfels from the points and normals, the call, the result"""
        samples, first_sample = _sample_range(samples, first_sample)
        surf = surfel_records(points, normals)
        f = Form(self.query_device, surf, seeds, out)
        surf, fp = f.input("points / normals", surf, abi.SURFEL)
        n = len(surf)
        seeds, sp = f.optional("seeds", seeds, SEEDS, n)
        res, op = f.output("out", out, out_dtype, n)
        self._query(f, name, fp, sp, n, prm.ctypes.data, first_sample, samples, op)
        return res

    def trace_hemisphere(self, points, normals, samples, first_sample=0, seeds=None, offset=1e-3, out=None):
        """rb_trace_hemisphere: the radiance arriving at (m, 3) surface points over the cosine-weighted hemisphere of their
        normals (any length: the device normalises), every (point, sample) ray made on the device from its own random
        stream -> abi.RADIANCE[m] (``sum`` over the samples, ``weight``: the valid samples; sum / weight is the irradiance
        over pi).  ``seeds``: m uint32 ids or None (the point's index).  Torch tensors on the engine's device for the points
        and normals, or for ``out`` ((m, 4) float32), go to rb_trace_hemisphere_device: nothing crosses to the host."""
        return self._hemisphere("rb_trace_hemisphere", abi.RADIANCE, points, normals, samples, first_sample, seeds,
                                self._hemi_params(offset), out)

    def openness(self, points, normals, samples, radius, mask=abi.MASK_ALL & ~abi.MASK_LIGHTS, first_sample=0, seeds=None, offset=1e-3,
                 out=None):
        """rb_openness_hemisphere: of ``samples`` cosine-weighted rays from each point, how many meet nothing of the stages of
        ``mask`` within ``radius`` (rb_occluded's tmax rules) -> abi.OPENNESS[m] (``open``, ``valid``; open / valid is the
        ambient-occlusion value).  Torch tensors select rb_openness_hemisphere_device and an (m, 2) int32 tensor comes back."""
        return self._hemisphere("rb_openness_hemisphere", abi.OPENNESS, points, normals, samples, first_sample, seeds,
                                self._hemi_params(offset, radius, mask), out)

    # ---- direct light at surface points (rb_abi.h)
    def scene_emitters(self, out=None):
        """rb_scene_emitters: the emitter table of the uploaded scene -- its emissive triangles, then spheres, then lights, as
        ``direct.scene_emitters`` models it -- made on the device by the first call after an update -> abi.EMITTER[count].
        ``out``: an (capacity, 16) float32 tensor on the engine's device selects rb_scene_emitters_device: its first
        min(count, capacity) rows are filled and (out, count) is returned; nothing but the count crosses to the host."""
        if out is not None:
            dev = self.query_device
            out, op = device_tensor("out", out, abi.EMITTER, dev)
            cnt = device_new(np.int32, 1, dev)
            self._device_call(self._lib.rb_scene_emitters_device, op, len(out), cnt.data_ptr())
            return out, int(cnt.cpu().numpy().view(np.uint32)[0])
        count = C.c_size_t(0)
        self._check(self._lib.rb_scene_emitters(self._h, None, 0, C.byref(count)))
        table = np.zeros(count.value, dtype=abi.EMITTER)
        self._check(self._lib.rb_scene_emitters(self._h, host_ptr(table), len(table), C.byref(count)))
        return table

    def scene_emitter_cdf(self, out=None):
        """rb_scene_emitter_cdf: the pick weights by power of the scene's emitter table (``direct.emitter_cdf`` of
        ``scene_emitters``), made on the device by the first call that needs them after an update ->
        uint32[count].  ``out``: a (capacity,) int32 or uint32 tensor on the engine's device selects
        rb_scene_emitter_cdf_device: (out, count) comes back, as ``scene_emitters`` has it."""
        if out is not None:
            dev = self.query_device
            out, op = device_tensor("out", out, CDF, dev)
            cnt = device_new(np.int32, 1, dev)
            self._device_call(self._lib.rb_scene_emitter_cdf_device, op, len(out), cnt.data_ptr())
            return out, int(cnt.cpu().numpy().view(np.uint32)[0])
        count = C.c_size_t(0)
        self._check(self._lib.rb_scene_emitter_cdf(self._h, None, 0, C.byref(count)))
        table = np.zeros(count.value, dtype=CDF)
        self._check(self._lib.rb_scene_emitter_cdf(self._h, host_ptr(table), len(table), C.byref(count)))
        return table

    def _tally_in(self, f, tally, entries):
        """(what the call takes, pointer, the caller's numpy array to copy back into or None) of a tally argument: abi.GRID_TALLY
        records in host memory, or an (entries, 2) int32 tensor on the engine's device; a numpy array beside tensors is staged"""
        if is_tensor(tally) or not f.on_device:
            if not is_tensor(tally) and not (isinstance(tally, np.ndarray) and tally.dtype == abi.GRID_TALLY and tally.flags.c_contiguous
                                             and tally.flags.writeable):
                raise ValueError("tally: a writable contiguous abi.GRID_TALLY array (it is added to in place) or a tensor is needed")
            t, p = f.input("tally", tally, abi.GRID_TALLY, entries)
            return t, p, None
        back = tally if isinstance(tally, np.ndarray) and tally.dtype == abi.GRID_TALLY else None
        t, p = f.input("tally", upload(host_in("tally", tally, abi.GRID_TALLY, entries)[0], abi.GRID_TALLY, self.query_device),
                       abi.GRID_TALLY, entries)
        return t, p, back

    def emitter_grid(self, grid, emitters=None, tally=None, prior=1.0, out=None):
        """rb_emitter_grid_cdf_device: the pick tables per grid cell (``direct.emitter_grid_cdf`` is the
        model) of an abi.PROBE_GRID whose counts count cells -- uint32[rows * n], row r at [r n, (r + 1) n).  ``emitters``: None
        for the scene's own table, or an abi.EMITTER table of the caller's.  Host arrays in, a numpy array out; a tensor for
        ``emitters`` or ``out`` (int32 / uint32, rows * n entries) keeps everything on the engine's device and the tensor comes
        back: ``direct_light(pick=("grid", grid, tables))`` takes it as it is.  The engine keeps no grid.
        ``tally``: rb_emitter_grid_learned_device, the tables that learn visibility -- the abi.GRID_TALLY
        records ``direct_light(tally=...)`` keeps (an array, or an (rows * n, 2) int32 tensor) and a ``prior`` in (0, 16777216]."""
        g, rows = grid_records(grid)
        f = Form(self.query_device, emitters, out, tally, staged=True)
        tp, n_emit = None, len(self.scene_emitters())
        if emitters is not None:
            table, tp = f.input("emitters", emitters, abi.EMITTER)
            n_emit = len(table)
        if rows * max(n_emit, 1) > abi.MAX_GRID_ENTRIES:
            raise ValueError("grid: at most 2^26 entries (cells times emitters) are taken")
        if out is None:
            out = device_new(np.int32, rows * n_emit, self.query_device)
        res, op = f.output("out", out, CDF, rows * n_emit)
        if tally is not None:
            kept, kp = f.input("tally", tally, abi.GRID_TALLY, rows * n_emit)
            self._device_call(self._lib.rb_emitter_grid_learned_device, tp, n_emit, g.ctypes.data, kp, float(prior), op)
            return f.result(res, CDF)
        self._device_call(self._lib.rb_emitter_grid_cdf_device, tp, n_emit, g.ctypes.data, op)
        return f.result(res, CDF)

    @staticmethod
    def _light_params(offset, shorten, mask=abi.MASK_ALL):
        prm = np.zeros(1, dtype=abi.LIGHT_PARAMS)
        prm["offset"], prm["shorten"], prm["mask"] = offset, shorten, int(mask)
        return prm

    def direct_light(self, points, normals, samples, emitters=None, first_sample=0, seeds=None, offset=1e-3, shorten=1e-3,
                     mask=abi.MASK_ALL, out=None, pick="uniform", tally=None):
        """rb_direct_light: what reaches (m, 3) surface points directly from the lights, by ``samples`` shadow rays per point,
        each aimed at a point drawn on a uniformly picked emitter and walked by rb_occluded among the stages of ``mask`` ->
        abi.RADIANCE[m] (``sum`` over the samples, ``weight``: the valid samples; sum / weight is the direct irradiance over
        pi -- trace_hemisphere's convention, so the two add and compare).  ``emitters``: None for the scene's own table
        (``scene_emitters``), or an abi.EMITTER table of the caller's -- one light, or one group of lights, gets a map of its
        own.  ``shorten``: the fraction of its length a shadow ray ends short of the sampled point.  Torch tensors on the
        engine's device for the points and normals, the table ((n, 16) float32) or ``out`` ((m, 4) float32) go to
        rb_direct_light_device: nothing crosses to the host.
        ``pick``: how a sample picks its emitter -- "uniform": rb_direct_light as it always was;
        "power": rb_direct_light_cdf by the table's power, the scene's kept weights (``scene_emitter_cdf``) or those made for
        the caller's table; or the caller's own inclusive weights beside the caller's ``emitters``, a uint32 array or an
        int32 / uint32 tensor with one entry per emitter.  The estimate keeps its mean as long as every emitter that can
        light a point keeps a weight above 0.
        ("grid", grid) or ("grid", grid, tables): rb_direct_light_grid, the pick per grid cell -- ``grid``
        an abi.PROBE_GRID whose counts count cells, ``tables`` what ``emitter_grid`` returns (None: made for this call).
        ``tally`` (with a grid pick): rb_direct_light_grid_tally -- abi.GRID_TALLY[rows * n_emit], or an
        (rows * n_emit, 2) int32 tensor, to which the call adds the shadow rays it tried and saw per (cell, emitter);
        ``emitter_grid(tally=...)`` makes tables of it.  The caller zeroes and keeps it.  ``out=False`` with a tally: a
        training-only call, no sums are made and None comes back."""
        samples, first_sample = _sample_range(samples, first_sample)
        surf = surfel_records(points, normals)
        weights, cells = None, None
        if isinstance(pick, tuple):
            if len(pick) not in (2, 3) or pick[0] != "grid":
                raise ValueError('pick: ("grid", grid) or ("grid", grid, tables)')
            cells, rows = grid_records(pick[1])
            weights = pick[2] if len(pick) == 3 else None
        elif isinstance(pick, str):
            if pick not in ("uniform", "power"):
                raise ValueError('pick: "uniform", "power" or a table of weights')
        elif emitters is None:
            raise ValueError("pick: a table of weights goes with a table of emitters")
        else:
            weights = pick
        if tally is not None and cells is None:
            raise ValueError('tally: it goes with pick=("grid", grid[, tables])')
        train_only = out is False
        if train_only and tally is None:
            raise ValueError("out=False: a call without sums needs a tally")
        if train_only:
            out = None
        f = Form(self.query_device, surf, seeds, emitters, out, weights, tally)
        surf, fp = f.input("points / normals", surf, abi.SURFEL)
        n = len(surf)
        table, tp, n_emit = None, None, 0
        if emitters is not None:
            if f.on_device and not is_tensor(emitters):
                emitters = upload(host_in("emitters", emitters, abi.EMITTER)[0], abi.EMITTER, self.query_device)
            table, tp = f.input("emitters", emitters, abi.EMITTER)
            n_emit = len(table)
            if n_emit == 0:   # an empty table of the caller's is not the scene's: a record that is never read stands in
                table, tp = f.input("emitters", device_new(abi.EMITTER, 1, self.query_device) if f.on_device else np.zeros(1, dtype=abi.EMITTER),
                                    abi.EMITTER)
        seeds, sp = f.optional("seeds", seeds, SEEDS, n)
        res, op = (None, None) if train_only else f.output("out", out, abi.RADIANCE, n)
        prm = self._light_params(offset, shorten, mask)
        if isinstance(pick, str) and pick == "uniform":
            self._query(f, "rb_direct_light", tp, n_emit, fp, sp, n, prm.ctypes.data, first_sample, samples, op)
            return res
        cp = None
        if cells is not None:
            if emitters is None:
                n_emit = len(self.scene_emitters())
            if weights is not None:
                if f.on_device and not is_tensor(weights):
                    weights = upload(host_in("pick", weights, CDF)[0].view(np.int32), np.dtype(np.int32), self.query_device)
                weights, cp = f.input("pick", weights, CDF, rows * n_emit)
            if tally is not None:
                kept, kp, back = self._tally_in(f, tally, rows * n_emit)
                if kp is None:   # no record to add to (no emitter, or an empty array): one that is never touched stands in
                    kept = device_new(abi.GRID_TALLY, 1, self.query_device) if f.on_device else np.zeros(1, dtype=abi.GRID_TALLY)
                    kp = kept.data_ptr() if f.on_device else kept.ctypes.data
                self._query(f, "rb_direct_light_grid_tally", tp, cells.ctypes.data, cp, n_emit, fp, sp, n, prm.ctypes.data, first_sample,
                            samples, op, kp)
                if back is not None and back.size:
                    back[...] = download(kept, abi.GRID_TALLY).reshape(back.shape)
                return res
            self._query(f, "rb_direct_light_grid", tp, cells.ctypes.data, cp, n_emit, fp, sp, n, prm.ctypes.data, first_sample, samples, op)
            return res
        if weights is not None:
            if f.on_device and not is_tensor(weights):
                weights = upload(host_in("pick", weights, CDF)[0].view(np.int32), np.dtype(np.int32), self.query_device)
            weights, cp = f.input("pick", weights, CDF, n_emit)
        self._query(f, "rb_direct_light_cdf", tp, cp, n_emit, fp, sp, n, prm.ctypes.data, first_sample, samples, op)
        return res

    # ---- lightmap texels made on the device (rb_abi.h)
    @staticmethod
    def _lightmap_params(width, height, mesh=None, flip=False, offset=0.0, dilate=0):
        for name, v in (("width", width), ("height", height), ("dilate", dilate)):
            if not 0 <= int(v) < 2 ** 32:
                raise ValueError(f"{name}: a 32-bit unsigned number")
        prm = np.zeros(1, dtype=abi.LIGHTMAP_PARAMS)
        prm["width"], prm["height"], prm["dilate"], prm["offset"] = int(width), int(height), int(dilate), offset
        prm["mesh"] = abi.LIGHTMAP_ALL_MESHES if mesh is None else int(mesh)
        prm["flags"] = abi.LIGHTMAP_FLIP if flip else 0
        return prm

    def lightmap_surfels(self, width, height, mesh=None, flip=False, out=None):
        """rb_lightmap_surfels_device: the surfel of every texel of a ``width`` x ``height`` atlas over the uploaded scene's uvs
        -- texel (x, y) at y * width + x, row 0 on top -- and the triangle that owns it (abi.LIGHTMAP_NO_OWNER: none; its surfel
        is all zero, which trace_hemisphere and openness call invalid).  ``mesh``: a mesh index, or None for every mesh;
        ``flip``: the normals negated.  ``out`` = (surfels, owners) torch tensors on the engine's device, (n, 8) float32 and
        (n,) int32 or None: filled and returned, and nothing crosses to the host -- what trace_hemisphere and openness take
        as ``surfels[:, 0:3]``, ``surfels[:, 4:7]``.  Without ``out``: (abi.SURFEL[n], uint32 owners[n]) numpy arrays."""
        prm = self._lightmap_params(width, height, mesh, flip)
        n = int(width) * int(height)
        dev = self.query_device
        surf, own = (device_new(abi.SURFEL, n, dev), device_new(np.int32, n, dev)) if out is None else out
        surf, sp = device_tensor("surfels", surf, abi.SURFEL, dev, n)
        own, op = (None, None) if own is None else device_tensor("owners", own, np.int32, dev, n)
        self._device_call(self._lib.rb_lightmap_surfels_device, prm.ctypes.data, sp, op)
        if out is not None:
            return surf, own
        return download(surf, abi.SURFEL), download(own, np.uint32)

    def bake_lightmap(self, width, height, samples, first_sample=0, mesh=None, flip=False, offset=1e-3, dilate=2, out=None, sums=None):
        """rb_bake_lightmap: the lightmap of the uploaded scene's uvs in one call -- surfels, ``samples`` cosine-weighted rays
        per texel traced as trace_hemisphere traces them (the stream id is the texel index), sum / weight, ``dilate`` fill
        passes round the charts -> float32 (height, width, 4) in sample_texture's layout (row 0 on top); fourth component
        0 = empty, 1 = baked, 2 = filled.  ``sums``: an abi.RADIANCE[height * width] array that receives the raw sums, for
        accumulating over calls with ``first_sample`` and resolving later (lightmap_resolve).  Torch tensors on the engine's
        device for ``out`` ((n, 4) float32) or ``sums`` ((n, 4) float32) select rb_bake_lightmap_device: nothing crosses to the
        host, and ``out`` (or, with sums alone, ``sums``) is returned."""
        samples, first_sample = _sample_range(samples, first_sample)
        prm = self._lightmap_params(width, height, mesh, flip, offset, dilate)
        n = int(width) * int(height)
        f = Form(self.query_device, out, sums)
        if f.on_device:   # rgba rows in abi.RADIANCE's layout, and none where ``out`` is None
            res, op = (None, None) if out is None else f.output("out", out, abi.RADIANCE, n)
        else:
            res, op = host_out("out", out, np.float32, (int(height), int(width), 4), any_shape=True)
        sums, sp = (None, None) if sums is None else f.output("sums", sums, abi.RADIANCE, n, any_shape=True)
        self._query(f, "rb_bake_lightmap", prm.ctypes.data, first_sample, samples, op, sp)
        return res if res is not None else sums

    # ---- irradiance probes made on the device (rb_abi.h)
    def _bake_probes(self, name, out_dtype, pos, samples, first_sample, seeds, out, *params):
        """the two forms of a bake over probes: probe records from the positions, the call -- `params` go between the sample
        range and the result --, the result"""
        samples, first_sample = _sample_range(samples, first_sample)
        f = Form(self.query_device, pos, seeds, out)
        rec, pp = f.input("pos", probe_records(pos), abi.PROBE)
        n = len(rec)
        seeds, sp = f.optional("seeds", seeds, SEEDS, n)
        res, op = f.output("out", out, out_dtype, n)
        self._query(f, name, pp, sp, n, first_sample, samples, *params, op)
        return res

    def bake_probes(self, pos, samples, first_sample=0, seeds=None, out=None):
        """rb_bake_probes: the SH9 sums of the radiance arriving at (n, 3) points in free space from every direction,
        ``samples`` uniform-sphere rays per probe made on the device from the probe's own random stream -> abi.SH9[n] (``sum``
        [j][channel] over the samples, ``weight``: the valid samples; ``probes.radiance_coefficients`` and
        ``probes.irradiance`` read them).  ``seeds``: n uint32 ids or None (the probe's index).  A torch tensor on the engine's
        device for the positions, the seeds or ``out`` ((n, 28) float32) goes to rb_bake_probes_device: an (n, 28) tensor comes
        back and nothing crosses to the host."""
        return self._bake_probes("rb_bake_probes", abi.SH9, pos, samples, first_sample, seeds, out)

    # ---- light points from a baked probe grid (rb_abi.h)
    def probe_coefficients(self, sh, out=None):
        """rb_probe_coefficients_device: abi.SH9 sums (``bake_probes``' result) -> irradiance-over-pi coefficients in the same
        layout, the weight 1 (a valid probe) or 0 (its record all zero) -- what ``light_points`` blends.  A numpy array in
        gives abi.SH9[n] out.  An (n, 28) float32 tensor on the engine's device is read where it lies and an (n, 28) tensor
        comes back: ``out`` if given -- it may be ``sh`` itself, the work is then in place -- or a new one."""
        return _probe_stage(*self._staged(sh, out), "rb_probe_coefficients", abi.SH9, "sh", sh, out)

    def light_points(self, grid, coeffs, points, normals=None, out=None):
        """rb_light_points_device: the lit value of m points from a regular grid of baked probes -- ``grid``: an abi.PROBE_GRID
        scalar (``probes.grid_params``), ``coeffs``: its nx * ny * nz coefficient records, x fastest (``probe_coefficients``)
        -- for the points' normals (any length: the device normalises).  ``points`` and ``normals``: (m, 3) each, or
        ``points`` alone as surfel records (abi.SURFEL[m], or an (m, 8) float32 tensor: pos, 0, normal, 0 -- what
        ``lightmap_surfels`` makes).  numpy in gives abi.LIT[m] out (``value``: the irradiance over pi, albedo x value is a
        lambert surface's radiance; ``weight``: the blend weight, 0 where nothing lit the point).  With a torch tensor on the
        engine's device for the coefficients ((n, 28) float32), the points or ``out`` ((m, 4) float32), every tensor is used
        where it lies, an (m, 4) tensor comes back and nothing crosses to the host."""
        return _light_points(*self._staged(coeffs, points, normals, out), grid, coeffs, points, normals, out)

    # ---- probe visibility: depth moments and the leak-free blend (rb_abi.h)
    def bake_probe_depth(self, pos, samples, max_distance, first_sample=0, seeds=None, out=None):
        """rb_bake_probe_depth: per probe an 8 x 8 octahedral map of the first-hit distances of ``bake_probes``' own rays (same
        ``seeds``, ``first_sample`` and ``samples``: the same rays), clipped at ``max_distance`` -> abi.PROBE_DEPTH[n], texel
        ty * 8 + tx = {sum r, sum r r, samples, back faces among them}; ``probe_moments`` turns the sums into what
        ``light_points_visible`` reads.  A torch tensor on the engine's device for the positions, the seeds or ``out``
        ((n, 256) float32) goes to rb_bake_probe_depth_device: an (n, 256) tensor comes back and nothing crosses to the host."""
        return self._bake_probes("rb_bake_probe_depth", abi.PROBE_DEPTH, pos, samples, first_sample, seeds, out, float(max_distance))

    def probe_moments(self, sums, out=None):
        """rb_probe_moments_device: abi.PROBE_DEPTH sums (``bake_probe_depth``'s result) -> (moments, back-face share per probe):
        a texel with samples becomes {mean r, mean r r, 1, its back-face share}, one without all zero.  A numpy array in gives
        (abi.PROBE_DEPTH[n], float32 (n,)) out.  An (n, 256) float32 tensor on the engine's device is read where it lies and
        tensors come back: ``out`` if given -- it may be ``sums`` itself, the work is then in place -- or a new one."""
        return _probe_stage(*self._staged(sums, out), "rb_probe_moments", abi.PROBE_DEPTH, "sums", sums, out, share=True)

    def light_points_visible(self, grid, coeffs, moments, points, normals=None, normal_bias=0.0, min_visibility=0.0, wrap=True, depth=True,
                             out=None):
        """rb_light_points_visible_device: ``light_points`` with every probe's weight times a wrapped cosine of the point's normal
        towards the probe (``wrap``) and the Chebyshev bound of the point's distance -- the point moved ``normal_bias`` along
        its normal first -- against the probe's depth moments (``depth``; ``moments``: ``probe_moments``' maps, abi.PROBE_DEPTH
        [nx * ny * nz] or an (n, 256) float32 tensor; None with ``depth=False``), never below ``min_visibility``.  Everything
        else, tensors included, as ``light_points``; with both weights off the result is ``light_points``' bit for bit."""
        return _light_points(*self._staged(coeffs, moments, points, normals, out), grid, coeffs, points, normals, out, moments,
                             _visibility(normal_bias, min_visibility, wrap, depth))

    def last_probe_depth_project_ms(self):
        """kernel ms of the projection (k_depth_project) in the most recent bake_probe_depth: its share of last_query_ms()"""
        return self._last_ms(self._lib.rb_last_probe_depth_project_ms)

    def last_probe_project_ms(self):
        """kernel ms of the projection (k_sh_project) in the most recent bake_probes: its share of last_query_ms()"""
        return self._last_ms(self._lib.rb_last_probe_project_ms)

    def last_lightmap_ms(self):
        """(surfels_ms, resolve_ms): kernel ms of the surfel stage and of the resolve in the most recent lightmap_surfels or
        bake_lightmap; both lie inside last_query_ms()"""
        return self._last_ms(self._lib.rb_last_lightmap_ms, 2)

    def last_camera_rays_ms(self):
        """kernel ms of the generator (k_cam_rays, k_hemi_rays, k_probe_rays) in the most recent trace_camera, trace_hemisphere, openness or bake_probes:
        its share of last_query_ms()"""
        return self._last_ms(self._lib.rb_last_camera_rays_ms)

    def render_hits(self, surfaces=False):
        """rb_render_hits: the first hit of every pixel centre as abi.HIT[rows, width] (and abi.SURFACE with ``surfaces``) in
        the orientation of the delivered frame; a sharded engine: its padded local rows, like read_accumulation."""
        w, h = self.size()
        if self.shard_count > 1:   # (a multi-device handle delivers whole frames: its shard_count is 1 here)
            h = self.local_rows()[1]
        hits = np.empty((h, w), dtype=abi.HIT)
        surf = np.empty((h, w), dtype=abi.SURFACE) if surfaces else None
        self._check(self._lib.rb_render_hits(self._h, hits.ctypes.data, None if surf is None else surf.ctypes.data))
        return (hits, surf) if surfaces else hits

    def pick(self, px, py):
        """rb_pick: (abi.HIT, abi.SURFACE) scalars of displayed pixel (px from the left, py from the top)."""
        hit, surf = np.empty(1, dtype=abi.HIT), np.empty(1, dtype=abi.SURFACE)
        self._check(self._lib.rb_pick(self._h, int(px), int(py), hit.ctypes.data, surf.ctypes.data))
        return hit[0], surf[0]

    def last_query_kernel_name(self):
        return (self._lib.rb_last_query_kernel_name(self._h) or b"").decode()

    def last_query_ms(self):
        return self._last_ms(self._lib.rb_last_query_ms)

    # ---- the denoiser (rb_abi.h)
    def denoise(self, params=None, linear=False, out=None):
        """rb_denoise: the edge-avoiding a-trous filter over the committed accumulation, guided by the first hits of the pixel
        centres.  ``params``: an abi.DENOISE_PARAMS scalar (``denoise.params(...)``), by default the library's.  Returns the
        RGBA8 frame, uint8 (h, w, 4) -- with ``linear`` the linear output, float32 (h, w, 4), w = 1.  ``out``: an array of that
        shape to fill instead (a page-locked one is filled by DMA), or a torch tensor on the engine's device (uint8 or float32,
        (h, w, 4), contiguous): rb_denoise_device writes it there and nothing crosses to the host."""
        p = np.ascontiguousarray(denoise_defaults() if params is None else params, dtype=abi.DENOISE_PARAMS).reshape(1)
        w, h = self.size()
        if is_tensor(out):
            import torch
            dtype = torch.float32 if linear else torch.uint8
            if out.device != torch_device(self.query_device) or out.dtype != dtype or not out.is_contiguous() \
                    or tuple(out.shape) != (h, w, 4):
                raise ValueError(f"out: a contiguous {dtype} tensor of shape ({h}, {w}, 4) on cuda:{self.query_device} is needed")
            ptr = out.data_ptr() if out.numel() else None
            self._device_call(self._lib.rb_denoise_device, p.ctypes.data, *((None, ptr) if linear else (ptr, None)))
            return out
        res, _ = host_out("out", out, np.float32 if linear else np.uint8, (h, w, 4))
        ptr = res.ctypes.data
        self._check(self._lib.rb_denoise(self._h, p.ctypes.data, *((None, ptr) if linear else (ptr, None))))
        return res

    def denoise_guides(self):
        """rb_denoise_guides: the guide buffer the engine filters with, abi.GUIDE[h, w] in the orientation of the frame."""
        w, h = self.size()
        g = np.empty((h, w), dtype=abi.GUIDE)
        self._check(self._lib.rb_denoise_guides(self._h, g.ctypes.data))
        return g

    def last_denoise_ms(self):
        """(kernel ms of the most recent denoise, ms of the guide build it had to make -- 0 when it had the guides)"""
        return self._last_ms(self._lib.rb_last_denoise_ms, 2)

    # ---- temporal reprojection (rb_abi.h)
    def reproject(self, prev4, prev_guides, view, cur_guides, cur4=None, params=None, out=None, size=None):
        """rb_reproject_buffers on the engine's device / rb_reproject_device: REPROJECT of section 22.1, and with ``cur4`` MERGE on
        top.  Host arrays: ``prev4`` / ``cur4`` (h, w, 4) float32 frame records, the guides abi.GUIDE[h, w] -> (h, w, 4) float32.
        Torch tensors on the engine's device: (h * w, 4) float32 records and (h * w, 12) float32 guides, ``size`` = (w, h) -> an
        (h * w, 4) tensor (``out`` if given); every tensor is used where it lies and nothing crosses to the host.  ``view``: the
        previous camera's abi.VIEW (``view_from_camera``); ``params``: abi.REPROJECT_PARAMS, by default the library's."""
        p = np.ascontiguousarray(reproject_defaults() if params is None else params, dtype=abi.REPROJECT_PARAMS).reshape(1)
        v = np.ascontiguousarray(view, dtype=abi.VIEW).reshape(1)
        f = Form(self.query_device, prev4, prev_guides, cur_guides, cur4, out)
        if size is None:
            if f.on_device or np.ndim(cur_guides) != 2:
                raise ValueError("size: (w, h) is needed unless cur_guides is an abi.GUIDE[h, w] array")
            size = np.shape(cur_guides)[::-1]
        w, h = int(size[0]), int(size[1])
        n = w * h
        prev4, pp = f.input("prev4", _frame_records(prev4), abi.FRAME_RECORD, n)
        pg, pgp = f.input("prev_guides", prev_guides, abi.GUIDE, n)
        cg, cgp = f.input("cur_guides", cur_guides, abi.GUIDE, n)
        cur4, cp = f.optional("cur4", None if cur4 is None else _frame_records(cur4), abi.FRAME_RECORD, n)
        res, op = f.output("out", None if out is None else _frame_records(out), abi.FRAME_RECORD, n)
        if n and f.on_device:
            self._device_call(self._lib.rb_reproject_device, p.ctypes.data, w, h, v.ctypes.data, pp, pgp, cgp, cp, op)
        elif n:
            _check_global(self._lib.rb_reproject_buffers(self.query_device, p.ctypes.data, w, h, v.ctypes.data, pp, pgp, cgp, cp, op))
        return res if f.on_device else res.view(np.float32).reshape(h, w, 4)

    def denoise_history(self, rparams=None, dparams=None, linear=False, out=None):
        """rb_denoise_history: ``denoise`` on the frame with its history -- the previous call's records carried across the
        camera move of the last update (REPROJECT), the accumulation merged onto them (MERGE), the filter over the result.
        ``rparams``: abi.REPROJECT_PARAMS (``temporal.params(...)``), ``dparams``: abi.DENOISE_PARAMS, by default the library's.
        ``linear`` and ``out`` as ``denoise`` has them.  Call it once per displayed frame, after the frame's passes."""
        rp = np.ascontiguousarray(reproject_defaults() if rparams is None else rparams, dtype=abi.REPROJECT_PARAMS).reshape(1)
        dp = np.ascontiguousarray(denoise_defaults() if dparams is None else dparams, dtype=abi.DENOISE_PARAMS).reshape(1)
        w, h = self.size()
        if is_tensor(out):
            import torch
            dtype = torch.float32 if linear else torch.uint8
            if out.device != torch_device(self.query_device) or out.dtype != dtype or not out.is_contiguous() \
                    or tuple(out.shape) != (h, w, 4):
                raise ValueError(f"out: a contiguous {dtype} tensor of shape ({h}, {w}, 4) on cuda:{self.query_device} is needed")
            ptr = out.data_ptr() if out.numel() else None
            self._device_call(self._lib.rb_denoise_history_device, rp.ctypes.data, dp.ctypes.data, *((None, ptr) if linear else (ptr, None)))
            return out
        res, _ = host_out("out", out, np.float32 if linear else np.uint8, (h, w, 4))
        ptr = res.ctypes.data
        self._check(self._lib.rb_denoise_history(self._h, rp.ctypes.data, dp.ctypes.data, *((None, ptr) if linear else (ptr, None))))
        return res

    def history(self):
        """rb_history_read: the frame records of the most recent ``denoise_history`` -- (h, w, 4) float32, {mean r, g, b,
        count} -- before the filter; RenderError (not initialised) without one."""
        w, h = self.size()
        out = np.empty((h, w, 4), dtype=np.float32)
        self._check(self._lib.rb_history_read(self._h, out.ctypes.data))
        return out

    def history_reset(self):
        """rb_history_reset: the next ``denoise_history`` starts without history"""
        self._check(self._lib.rb_history_reset(self._h))

    def last_reproject_ms(self):
        """kernel ms of REPROJECT (0 when the base was there already) plus MERGE in the most recent denoise_history"""
        return self._last_ms(self._lib.rb_last_reproject_ms)

    def fast_bvh_builder(self):
        """("host-sah" | "device-lbvh" | "", build milliseconds) of the tree RB_FLAG_FAST_BVH walks."""
        return self._builder(self._lib.rb_fast_bvh_builder)

    def sphere_tree_builder(self):
        """("device-median" | "host-median" | "", build milliseconds) of the library's sphere tree (> 64 spheres)."""
        return self._builder(self._lib.rb_sphere_tree_builder)

    def chunk_tree_builder(self):
        """("device" | "host" | "", build milliseconds) of the chunked walk's tree (multi-node meshes, the default walk)."""
        return self._builder(self._lib.rb_chunk_tree_builder)

    def tree(self):
        """(abi.BVH_NODE[], uint32[] indices) of the reference-layout tree the engine walks (rb_engine_tree): the caller's,
        or the engine's own under ``build_tree``."""
        nn, ni = C.c_size_t(0), C.c_size_t(0)
        self._check(self._lib.rb_engine_tree(self._h, None, 0, C.byref(nn), None, 0, C.byref(ni)))
        nodes = np.zeros(nn.value, dtype=abi.BVH_NODE)
        indices = np.zeros(ni.value, dtype=np.uint32)
        self._check(self._lib.rb_engine_tree(self._h, host_ptr(nodes), len(nodes), C.byref(nn), host_ptr(indices), len(indices), C.byref(ni)))
        return nodes, indices

    def tree_builder(self):
        """("device" | "host" | "caller" | "", build milliseconds) of the reference-layout tree the engine walks."""
        return self._builder(self._lib.rb_tree_builder)

    def debug_chunk_tree(self):
        """The tree the engine walks, read back and checked (rb_debug_engine_chunk_tree): dict of its census, or None."""
        out = (C.c_uint64 * 6)()
        self._check(self._lib.rb_debug_engine_chunk_tree(self._h, out))
        if not out[0]:
            return None
        return dict(nodes=out[1], positions=out[2], depth=out[3], chunks=out[4], unbounded=out[5])

    def debug_own_tree(self):
        """The library's own triangle tree as the engine walks it, read back unchecked (rb_debug_engine_own_tree): dict of
        nodes (abi.OWN_NODE[]), slots, slot_meta, root, depth, bmin, bmax -- or None when the engine has no such tree."""
        return own_tree_readback(self._check, self._lib.rb_debug_engine_own_tree, self._h)

    def debug_sphere_tree(self):
        """The sphere tree as the engine walks it, read back unchecked (rb_debug_engine_sphere_tree): dict of nodes
        (abi.SPHERE_NODE[]), leaf (float32[n, 4]), ids, root, depth (stack entries) -- or None when the engine scans."""
        return sphere_tree_readback(self._check, self._lib.rb_debug_engine_sphere_tree, self._h)

    def last_dispatch_ms(self):
        return self._last_ms(self._lib.rb_last_dispatch_ms)


class FrameIterator:
    """``RaytracerFrameIterator`` (lib.rs:127-234)."""

    def __init__(self, engine: Engine):
        self._e = engine

    def has_next(self) -> bool:
        return bool(self._e._lib.rb_iter_has_next(self._e._h))

    def next(self) -> Frame:
        w, h = self._e._frame_shape()
        if self._e.comm_rank not in (None, 0):
            self._e._check(self._e._lib.rb_iter_next(self._e._h, None))
            return None
        out = np.empty((h, w, 4), dtype=np.uint8)
        self._e._check(self._e._lib.rb_iter_next(self._e._h, out.ctypes.data))
        return Frame(w, h, out)

    def destroy(self):
        self._e._lib.rb_iter_destroy(self._e._h)

    def __iter__(self):
        while self.has_next():
            yield self.next()


class PinnedFrame:
    """A page-locked RGBA8 frame buffer (rb_host_alloc) as a numpy array: read-backs into it are DMA copies."""

    def __init__(self, width, height):
        self._lib = load()
        self._p = self._lib.rb_host_alloc(width * height * 4)
        if not self._p:
            raise MemoryError("rb_host_alloc failed")
        self.array = np.ctypeslib.as_array((C.c_uint8 * (width * height * 4)).from_address(self._p)).reshape(height, width, 4)

    def free(self):
        if getattr(self, "_p", None):
            self.array = None
            self._lib.rb_host_free(self._p)
            self._p = None

    def __del__(self):
        try:
            self.free()
        except Exception:
            pass


def device_name(device=-1):
    buf = C.create_string_buffer(256)
    rc = load().rb_device_name(device, buf, 256)
    return buf.value.decode() if rc == 0 else "unknown"


def _generated(items, samples):
    """(abi.RAY[items * samples], uint32 seeds[items * samples]) for a generator to fill: of 0 items where it refuses the
    samples (a refused call writes nothing)"""
    if not 0 <= samples < 2 ** 32:
        raise ValueError("samples: a 32-bit unsigned number")
    n = items * samples if samples <= 65536 else 0
    return np.zeros(n, dtype=abi.RAY), np.zeros(n, dtype=np.uint32)


def camera_rays_device(cam, samples, first_sample=0, region=None, device=-1):
    """rb_camera_rays: the generator alone, no engine -- (abi.RAY[n * samples], uint32 seeds[n * samples]) of the pixels of
    ``region`` ((first_pixel, n_pixels); by default the whole image), item (pixel - first_pixel) * samples + k: the origin, the
    normalised direction (0 0 0: an invalid ray) and the seed trace_ray starts with.  ``camera.rays`` is its numpy model."""
    _, call = _engineless(device)
    c, first, n = _camera_region(cam, region)
    samples = int(samples)
    if not 0 <= samples < 2 ** 32:
        raise ValueError("samples: a 32-bit unsigned number")
    rays, seeds = np.zeros(n * samples, dtype=abi.RAY), np.zeros(n * samples, dtype=np.uint32)
    call("rb_camera_rays", c.ctypes.data, first, n, int(first_sample), samples, host_ptr(rays), host_ptr(seeds))
    return rays, seeds


def hemisphere_rays_device(points, normals, samples, first_sample=0, seeds=None, offset=1e-3, device=-1):
    """rb_hemisphere_rays: the generator alone, no engine -- (abi.RAY[m * samples], uint32 seeds[m * samples]) of (m, 3)
    points and normals, item i * samples + k: the origin, the normalised direction (0 0 0: an invalid item) and the seed
    trace_ray starts with.  ``hemisphere.rays`` is its numpy model."""
    f, call = _engineless(device)
    surf, fp = f.input("points", surfel_records(np.asarray(points, np.float32), np.asarray(normals, np.float32)), abi.SURFEL)
    rays, seeds_out = _generated(len(surf), int(samples))
    seeds, sp = f.optional("seeds", seeds, SEEDS, len(surf))
    prm = Engine._hemi_params(offset)
    call("rb_hemisphere_rays", fp, sp, len(surf), prm.ctypes.data, int(first_sample), int(samples), rays.ctypes.data, seeds_out.ctypes.data)
    return rays, seeds_out


def emitter_cdf(emitters, device=-1):
    """rb_emitter_cdf: the pick weights by power of an abi.EMITTER table, no engine -> uint32[n], inclusive (DESIGN.md section
    23).  ``direct.emitter_cdf`` is its numpy model."""
    f, call = _engineless(device)
    table, tp = f.input("emitters", emitters, abi.EMITTER)
    cdf = np.zeros(len(table), dtype=CDF)
    call("rb_emitter_cdf", tp, len(table), host_ptr(cdf))
    return cdf


def emitter_grid_cdf(emitters, grid, device=-1):
    """rb_emitter_grid_cdf: the pick tables per grid cell of an abi.EMITTER table and an abi.PROBE_GRID whose counts count cells, no
    engine -> uint32[rows * n], row r at [r n, (r + 1) n).  ``direct.emitter_grid_cdf`` is its numpy model."""
    f, call = _engineless(device)
    table, tp = f.input("emitters", emitters, abi.EMITTER)
    g, rows = grid_records(grid)
    if rows * max(len(table), 1) > abi.MAX_GRID_ENTRIES:
        raise ValueError("grid: at most 2^26 entries (cells times emitters) are taken")
    tables = np.zeros(rows * len(table), dtype=CDF)
    call("rb_emitter_grid_cdf", tp, len(table), g.ctypes.data, host_ptr(tables))
    return tables


def emitter_grid_learned(emitters, grid, tally, prior=1.0, device=-1):
    """rb_emitter_grid_learned: ``emitter_grid_cdf`` with the weight times the seen share of an abi.GRID_TALLY[rows * n] and a
    ``prior`` in (0, 16777216].  ``direct.emitter_grid_cdf(tally=...)`` is its numpy model."""
    f, call = _engineless(device)
    table, tp = f.input("emitters", emitters, abi.EMITTER)
    g, rows = grid_records(grid)
    if rows * max(len(table), 1) > abi.MAX_GRID_ENTRIES:
        raise ValueError("grid: at most 2^26 entries (cells times emitters) are taken")
    kept, kp = f.input("tally", tally, abi.GRID_TALLY, rows * len(table))
    tables = np.zeros(rows * len(table), dtype=CDF)
    call("rb_emitter_grid_learned", tp, len(table), g.ctypes.data, kp, float(prior), host_ptr(tables))
    return tables


def light_rays(emitters, points, normals, samples, first_sample=0, seeds=None, offset=1e-3, shorten=1e-3, device=-1, cdf=None, grid=None,
               tables=None):
    """rb_light_rays: the generator of direct_light alone, no engine -- (abi.RAY[m * samples], float32 bounds[m * samples],
    float32 contributions (m * samples, 4)) of an abi.EMITTER table and (m, 3) points and normals, item i * samples + k: the
    shadow ray's origin and direction (0 0 0: an invalid item), the bound rb_occluded walks it to (0: a dark item) and the
    unoccluded contribution with 1 for a valid item behind it.  ``direct.rays`` is its numpy model.  ``cdf``: None for the
    uniform pick, or rb_light_rays_cdf's weighted one: "power", or uint32 inclusive weights, one per
    emitter.  ``grid``: rb_light_rays_grid's pick per grid cell by ``tables`` (uint32[rows * n]; None: made
    for this call)."""
    f, call = _engineless(device)
    table, tp = f.input("emitters", emitters, abi.EMITTER)
    surf, fp = f.input("points", surfel_records(np.asarray(points, np.float32), np.asarray(normals, np.float32)), abi.SURFEL)
    rays, _ = _generated(len(surf), int(samples))
    tmax, contrib = np.zeros(len(rays), dtype=np.float32), np.zeros((len(rays), 4), dtype=np.float32)
    seeds, sp = f.optional("seeds", seeds, SEEDS, len(surf))
    prm = Engine._light_params(offset, shorten)
    if grid is not None:
        if cdf is not None:
            raise ValueError("cdf and grid: one pick at a time")
        g, rows = grid_records(grid)
        tables, cp = f.optional("tables", tables, CDF, rows * len(table))
        call("rb_light_rays_grid", tp, g.ctypes.data, cp, len(table), fp, sp, len(surf), prm.ctypes.data, int(first_sample), int(samples),
             host_ptr(rays), host_ptr(tmax), host_ptr(contrib))
        return rays, tmax, contrib
    if cdf is None:
        call("rb_light_rays", tp, len(table), fp, sp, len(surf), prm.ctypes.data, int(first_sample), int(samples), host_ptr(rays),
             host_ptr(tmax), host_ptr(contrib))
        return rays, tmax, contrib
    if isinstance(cdf, str):
        if cdf != "power":
            raise ValueError('cdf: None, "power" or a table of weights')
        cp = None
    else:
        cdf, cp = f.input("cdf", cdf, CDF, len(table))
    call("rb_light_rays_cdf", tp, cp, len(table), fp, sp, len(surf), prm.ctypes.data, int(first_sample), int(samples), host_ptr(rays),
         host_ptr(tmax), host_ptr(contrib))
    return rays, tmax, contrib


def probe_rays_device(pos, samples, first_sample=0, seeds=None, device=-1):
    """rb_probe_rays: the generator alone, no engine -- (abi.RAY[n * samples], uint32 seeds[n * samples]) of (n, 3) probe
    positions, item i * samples + k: the position, the normalised direction (0 0 0: an invalid item) and the seed trace_ray
    starts with.  ``probes.rays`` is its numpy model."""
    f, call = _engineless(device)
    rec, pp = f.input("pos", probe_records(np.asarray(pos, np.float32)), abi.PROBE)
    rays, seeds_out = _generated(len(rec), int(samples))
    seeds, sp = f.optional("seeds", seeds, SEEDS, len(rec))
    call("rb_probe_rays", pp, sp, len(rec), int(first_sample), int(samples), rays.ctypes.data, seeds_out.ctypes.data)
    return rays, seeds_out


def probe_coefficients(sh, device=-1):
    """rb_probe_coefficients: stage 1 alone, no engine -- abi.SH9[n] sums -> abi.SH9[n] coefficients.  ``probes.coefficients``
    is its numpy model."""
    return _probe_stage(*_engineless(device), "rb_probe_coefficients", abi.SH9, "sh", sh)


def light_points(grid, coeffs, points, normals=None, device=-1):
    """rb_light_points: stage 2, no engine -- abi.LIT[m] of m points from an abi.PROBE_GRID scalar and its nx * ny * nz
    coefficient records; ``points`` and ``normals`` (m, 3) each, or ``points`` alone as abi.SURFEL[m].  ``probes.light`` is its
    numpy model."""
    return _light_points(*_engineless(device), grid, coeffs, points, normals)


def probe_moments(sums, device=-1):
    """rb_probe_moments, no engine -- abi.PROBE_DEPTH[n] sums -> (abi.PROBE_DEPTH[n] moments, float32 (n,) back-face shares).
    ``probes.moments`` is its numpy model."""
    return _probe_stage(*_engineless(device), "rb_probe_moments", abi.PROBE_DEPTH, "sums", sums, share=True)


def light_points_visible(grid, coeffs, moments, points, normals=None, normal_bias=0.0, min_visibility=0.0, wrap=True, depth=True, device=-1):
    """rb_light_points_visible, no engine -- abi.LIT[m] as ``light_points`` with the visibility weights of
    ``Engine.light_points_visible``.  ``probes.light_visible`` is its numpy model."""
    return _light_points(*_engineless(device), grid, coeffs, points, normals, None, moments,
                         _visibility(normal_bias, min_visibility, wrap, depth))


def lightmap_surfels_device(tris, uvs, width, height, mesh=None, flip=False, device=-1):
    """rb_lightmap_surfels: the generator alone, no engine -- (abi.SURFEL[height * width], uint32 owners[height * width]) of
    abi.GPU_TRIANGLE triangles and their uv floats; every triangle counts as valid.  ``lightmap.surfels`` is its numpy model."""
    f, call = _engineless(device)
    tris, tp = f.input("tris", tris, abi.GPU_TRIANGLE)
    uvs, up = f.input("uvs", uvs, np.float32)
    prm = Engine._lightmap_params(width, height, mesh, flip)
    n = int(width) * int(height) if (0 < int(width) <= abi.LIGHTMAP_MAX_SIDE and 0 < int(height) <= abi.LIGHTMAP_MAX_SIDE) else 0
    surf, own = np.zeros(n, dtype=abi.SURFEL), np.zeros(n, dtype=np.uint32)   # (a refused call writes nothing)
    call("rb_lightmap_surfels", tp, len(tris), up, len(uvs), prm.ctypes.data, surf.ctypes.data, own.ctypes.data)
    return surf, own


def lightmap_resolve(sums, width, height, dilate=2, device=-1):
    """rb_lightmap_resolve: the resolve alone, no engine -- abi.RADIANCE[height * width] sums -> float32 (height, width, 4):
    sum / weight and ``dilate`` fill passes.  ``lightmap.resolve`` is its numpy model."""
    f, call = _engineless(device)
    width, height, dilate = int(width), int(height), int(dilate)
    for v in (width, height, dilate):
        if not 0 <= v < 2 ** 32:
            raise ValueError("width, height and dilate are 32-bit unsigned numbers")
    sums, _ = f.input("sums", sums, abi.RADIANCE, width * height)
    out = np.zeros((height, width, 4), dtype=np.float32)
    call("rb_lightmap_resolve", width, height, sums.ctypes.data, dilate, out.ctypes.data)
    return out


def denoise_defaults():
    """rb_denoise_default_params as an abi.DENOISE_PARAMS scalar."""
    p = np.zeros(1, dtype=abi.DENOISE_PARAMS)
    rc = load().rb_denoise_default_params(p.ctypes.data)
    if rc != abi.RB_OK:
        raise RenderError(rc, "rb_denoise_default_params")
    return p[0]


def view_from_camera(uniforms_or_camera, w=None, h=None):
    """rb_view_from_camera: the abi.VIEW scalar of a render camera (abi.CAMERA with ``w`` and ``h``, or abi.UNIFORMS, which
    brings its own size); host only.  ``temporal.view_from_camera`` is its numpy model."""
    a = np.asarray(uniforms_or_camera)
    if a.dtype == abi.UNIFORMS:
        u = a.reshape(-1)[0]
        a, w, h = u["camera"], (u["width"] if w is None else w), (u["height"] if h is None else h)
    cam = np.ascontiguousarray(a, dtype=abi.CAMERA).reshape(1)
    v = np.zeros(1, dtype=abi.VIEW)
    _check_global(load().rb_view_from_camera(cam.ctypes.data, int(w), int(h), v.ctypes.data))
    return v[0]


def reproject_defaults():
    """rb_reproject_default_params as an abi.REPROJECT_PARAMS scalar."""
    p = np.zeros(1, dtype=abi.REPROJECT_PARAMS)
    rc = load().rb_reproject_default_params(p.ctypes.data)
    if rc != abi.RB_OK:
        raise RenderError(rc, "rb_reproject_default_params")
    return p[0]


def _frame_records(x):
    """(h, w, 4) or (n, 4) float32 frame records as abi.FRAME_RECORD[n]; a tensor as it stands"""
    if is_tensor(x):
        return x
    a = np.asarray(x)
    if a.dtype == abi.FRAME_RECORD:
        return a
    if a.ndim < 1 or a.shape[-1] != 4:
        raise ValueError(f"frame records: (..., 4) float32 is needed, not {a.shape}")
    if not (isinstance(x, np.ndarray) and a.dtype == np.float32 and a.flags.c_contiguous):
        a = np.ascontiguousarray(a, dtype=np.float32)
    return a.reshape(-1, 4).view(abi.FRAME_RECORD).reshape(-1)


def reproject_buffers(prev4, prev_guides, view, cur_guides, cur4=None, params=None, device=-1):
    """rb_reproject_buffers: REPROJECT of section 22.1 -- with ``cur4`` MERGE on top -- on its own: (h, w, 4) float32 frame
    records and abi.GUIDE[h, w] in, (h, w, 4) float32 out; host arrays, the work on the GPU, no engine.
    ``temporal.reproject`` and ``temporal.merge`` are its numpy model."""
    cg = np.ascontiguousarray(cur_guides, dtype=abi.GUIDE)
    pg = np.ascontiguousarray(prev_guides, dtype=abi.GUIDE)
    if cg.ndim != 2 or pg.shape != cg.shape:
        raise ValueError(f"previous guides {pg.shape} and current guides {cg.shape} differ")
    h, w = cg.shape
    f, call = _engineless(device)
    p4, pp = f.input("prev4", _frame_records(prev4), abi.FRAME_RECORD, w * h)
    c4, cp = f.optional("cur4", None if cur4 is None else _frame_records(cur4), abi.FRAME_RECORD, w * h)
    p = np.ascontiguousarray(reproject_defaults() if params is None else params, dtype=abi.REPROJECT_PARAMS).reshape(1)
    v = np.ascontiguousarray(view, dtype=abi.VIEW).reshape(1)
    out = np.zeros((h, w, 4), dtype=np.float32)   # (a refused call writes nothing)
    call("rb_reproject_buffers", p.ctypes.data, w, h, v.ctypes.data, pp or p4.ctypes.data, pg.ctypes.data, cg.ctypes.data, cp, out.ctypes.data)
    return out


def denoise_buffers(color, guides, params=None, device=-1):
    """rb_denoise_buffers: the filter on its own -- (h, w, 3 or 4) float32 mean radiance and abi.GUIDE[h, w] in, the linear
    output (h, w, 4) float32 and the RGBA8 frame (h, w, 4) uint8 out; host arrays, the work on the GPU, no engine."""
    g = np.ascontiguousarray(guides, dtype=abi.GUIDE)
    c = np.asarray(color, dtype=np.float32)
    if c.ndim != 3 or c.shape[:2] != g.shape or c.shape[2] not in (3, 4):
        raise ValueError(f"colour {c.shape} and guides {g.shape} differ")
    h, w = g.shape
    c4 = np.zeros((h, w, 4), dtype=np.float32)
    c4[..., :c.shape[2]] = c
    p = np.ascontiguousarray(denoise_defaults() if params is None else params, dtype=abi.DENOISE_PARAMS).reshape(1)
    lin, img = np.empty((h, w, 4), dtype=np.float32), np.empty((h, w, 4), dtype=np.uint8)
    _, call = _engineless(device)
    call("rb_denoise_buffers", p.ctypes.data, w, h, c4.ctypes.data, g.ctypes.data, lin.ctypes.data, img.ctypes.data)
    return lin, img
