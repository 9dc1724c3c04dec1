"""The one marshalling path between numpy arrays / torch tensors and the pointers of the C ABI (include/rb_abi.h).

A query takes arrays of records.  Its host form takes numpy arrays of the record's dtype; its device form takes torch tensors
on the engine's device, one row of ``row`` elements per record (``RECORDS``), or one element per item for a scalar.  ``Form``
decides which of the two a call is and resolves every array argument of it to (array, pointer); the helpers below it build
the records the families share.  Nothing here loads the library, and torch is imported only once a tensor is about.
"""
import numpy as np

from . import abi

# what each record is as a tensor: numpy dtype -> (element dtype, elements per row)
RECORDS = {rec: (np.dtype(elem), rec.itemsize // np.dtype(elem).itemsize) for rec, elem in (
    (abi.RAY, np.float32), (abi.SURFEL, np.float32), (abi.PROBE, np.float32), (abi.HIT, np.float32), (abi.SURFACE, np.float32),
    (abi.RADIANCE, np.float32), (abi.LIT, np.float32), (abi.OPENNESS, np.int32), (abi.SH9, np.float32), (abi.PROBE_DEPTH, np.float32))}
# ... and a table a call reads whole, beside its per-item arrays: the emitters of direct_light, (n, 16) float32
# ... and the per-pixel planes of ``Engine.reproject``: guide records, (n, 12) float32, and frame records, (n, 4)
TABLES = {rec: (np.dtype(np.float32), rec.itemsize // 4) for rec in (abi.EMITTER, abi.GUIDE, abi.FRAME_RECORD)}
# ... and the tally a grid call of direct_light adds to, one record per (cell, emitter): (n, 2) int32, only the bits count
TABLES[abi.GRID_TALLY] = (np.dtype(np.int32), 2)
# the ids of random streams: uint32 on the host; as a tensor int32 or uint32, only the bits count
SEEDS = np.dtype(np.uint32)
# the pick weights of direct_light, one inclusive entry per emitter: the same words under the same rule
CDF = SEEDS


def layout(dtype):
    """(element dtype, elements per row) of `dtype` as a tensor; the row of a scalar (uint8, float32, the seeds) is None"""
    dtype = np.dtype(dtype)
    return RECORDS.get(dtype) or TABLES.get(dtype, (dtype, None))


def is_tensor(x):
    """a torch tensor?  (without importing torch for callers that never pass one)"""
    return type(x).__module__.split(".")[0] == "torch" and hasattr(x, "data_ptr")


def host_ptr(a):
    """the address of a numpy array; None for no array and for an empty one"""
    return a.ctypes.data if (a is not None and a.size) else None


def same_length(name, got, n):
    """the one length check: `name` has `got` items where the call has n"""
    if got != n:
        raise ValueError(f"{name}: {n} items are needed, not {got}")


def host_in(name, value, dtype, n=None, flat=True):
    """(array, pointer) of an input of a host form: contiguous `dtype` items -- `value` itself when it is that already --, one
    dimension (``flat``), n of them where n is given"""
    a = np.ascontiguousarray(value, dtype=dtype)
    if flat and a.ndim != 1:
        a = a.reshape(-1)
    if n is not None:
        same_length(name, len(a), n)
    return a, host_ptr(a)


def host_out(name, out, dtype, shape, any_shape=False):
    """(array, pointer) of the result of a host form: ``out``, which must be a C-contiguous `dtype` ndarray of `shape` (an int
    n: (n,); ``any_shape``: of as many elements), or a new one"""
    shape = tuple(shape) if isinstance(shape, (tuple, list)) else (int(shape),)
    res = np.empty(shape, dtype=dtype) if out is None else out
    if not isinstance(res, np.ndarray) or res.dtype != dtype or not res.flags.c_contiguous \
            or (res.size != int(np.prod(shape, dtype=np.uint64)) if any_shape else res.shape != shape):
        raise ValueError(f"{name}: a contiguous {np.dtype(dtype).name} array of shape {shape} is needed")
    return res, host_ptr(res)


def torch_device(device):
    """the torch.device of a HIP ordinal (a torch.device stands for itself)"""
    import torch
    return device if isinstance(device, torch.device) else torch.device("cuda", device)


def device_tensor(name, t, dtype, device, n=None):
    """(tensor, data_ptr()) of a tensor a device form may read or write: on cuda:`device`, contiguous, of `dtype`'s element type,
    shape (rows, row) or (rows,) (``layout``), n rows where n is given; anything else is a ValueError.  An empty one: None."""
    import torch
    elem, row = layout(dtype)
    if elem == SEEDS and is_tensor(t) and t.dtype == getattr(torch, "uint32", None):
        want_dtype = torch.uint32
    else:
        want_dtype = torch.int32 if elem == SEEDS else getattr(torch, elem.name)
    want = torch_device(device)
    if not is_tensor(t) or t.device != want:
        raise ValueError(f"{name}: a torch tensor on {want} is needed (the engine's device)")
    if t.dtype != want_dtype or not t.is_contiguous():
        raise ValueError(f"{name}: a contiguous {want_dtype} tensor is needed")
    if row is None:
        if t.dim() != 1:
            raise ValueError(f"{name}: one element per item is needed")
    elif t.dim() != 2 or t.shape[1] != row:
        raise ValueError(f"{name}: shape (n, {row}) is needed")
    if n is not None:
        same_length(name, t.shape[0], n)
    return t, (t.data_ptr() if t.numel() else None)


def device_new(dtype, n, device):
    """a new tensor of n `dtype` items on cuda:`device`"""
    import torch
    elem, row = layout(dtype)
    return torch.empty((n,) if row is None else (n, row), dtype=getattr(torch, elem.name), device=torch_device(device))


def upload(a, dtype, device):
    """a numpy array of `dtype` items as a tensor on cuda:`device`"""
    import torch
    elem, row = layout(dtype)
    return torch.from_numpy(a.view(elem).reshape((-1,) if row is None else (-1, row))).to(torch_device(device))


def download(t, dtype):
    """the numpy array of `dtype` items of a tensor (``upload``'s inverse)"""
    return t.cpu().numpy().view(dtype).reshape(-1)


class Form:
    """Which form one call takes -- the device form when any of `arrays` is a tensor, as is every ``staged`` call: a call that
    has a device form only, whose numpy arrays are uploaded and whose results come back as numpy unless a tensor went in --
    and every array argument of it as (array, pointer).  The first input gives the number of items, every later argument is
    held to it through `n`; the pointers of a call of 0 items are None.  A pointer is good for as long as its array is kept:
    the array may be a converted copy, or an uploaded one, that nothing else holds."""

    def __init__(self, device, *arrays, staged=False):
        self.device = device
        self.tensors = any(is_tensor(a) for a in arrays)
        self.staged = staged
        self.on_device = self.tensors or staged

    def input(self, name, value, dtype, n=None, flat=True):
        if not self.on_device:
            return host_in(name, value, dtype, n, flat)
        if self.staged and not is_tensor(value):
            value = upload(host_in(name, value, dtype)[0], dtype, self.device)
        return device_tensor(name, value, dtype, self.device, n)

    def optional(self, name, value, dtype, n):
        """an input that may be None: (None, None) then"""
        return (None, None) if value is None else self.input(name, value, dtype, n)

    def output(self, name, out, dtype, n, any_shape=False):
        """``out`` if given, or a new array or tensor of n items (``any_shape``: as ``host_out`` has it; a tensor has its one shape)"""
        if not self.on_device:
            return host_out(name, out, dtype, n, any_shape)
        return device_tensor(name, device_new(dtype, n, self.device) if out is None else out, dtype, self.device, n)

    def result(self, t, dtype):
        """what the call returns for its result `t`: a staged call that no tensor went into, `t` as a numpy array"""
        return download(t, dtype) if (self.staged and not self.tensors) else t


def ray_records(origins, dirs):
    """abi.RAY[n] -- abi.SURFEL's layout too -- from (n, 3) numpy origins and directions (points and normals), or an (n, row)
    float32 tensor from (n, 3) torch tensors"""
    if is_tensor(origins) or is_tensor(dirs):
        import torch
        if not (is_tensor(origins) and is_tensor(dirs)) or origins.dtype != torch.float32 or dirs.dtype != torch.float32 \
                or origins.device != dirs.device:
            raise ValueError("origins and dirs must both be float32 tensors on one device")
        o, d = origins.reshape(-1, 3), dirs.reshape(-1, 3)
        same_length("dirs", len(d), len(o))
        rays = torch.zeros((len(o), layout(abi.RAY)[1]), dtype=torch.float32, device=o.device)
        rays[:, 0:3], rays[:, 4:7] = o, d
        return rays
    o = np.asarray(origins, dtype=np.float32).reshape(-1, 3)
    d = np.asarray(dirs, dtype=np.float32).reshape(-1, 3)
    same_length("dirs", len(d), len(o))
    rays = np.zeros(len(o), dtype=abi.RAY)
    rays["origin"], rays["dir"] = o, d
    return rays


def surfel_records(points, normals=None):
    """the surfels of a call: ``ray_records`` of (m, 3) points and normals, or `points` alone as ready records -- abi.SURFEL[m],
    or a tensor as it stands"""
    if normals is not None:
        rec = ray_records(points, normals)
        return rec if is_tensor(rec) else rec.view(abi.SURFEL)
    return points if is_tensor(points) else host_in("points", points, abi.SURFEL)[0]


def probe_records(pos):
    """abi.PROBE[n] from (n, 3) numpy positions, or an (n, row) float32 tensor from a float32 tensor of them"""
    if is_tensor(pos):
        import torch
        if pos.dtype != torch.float32:
            raise ValueError("pos: a float32 tensor is needed")
        p3 = pos.reshape(-1, 3)
        rec = torch.zeros((len(p3), layout(abi.PROBE)[1]), dtype=torch.float32, device=p3.device)
        rec[:, 0:3] = p3
        return rec
    p3 = np.asarray(pos, dtype=np.float32).reshape(-1, 3)
    rec = np.zeros(len(p3), dtype=abi.PROBE)
    rec["pos"] = p3
    return rec


def grid_records(grid):
    """(abi.PROBE_GRID[1], nx * ny * nz: the records its arrays need) of a probe grid"""
    g = np.ascontiguousarray(grid, dtype=abi.PROBE_GRID).reshape(1)
    return g, int(np.prod(g["counts"][0].astype(np.uint64)))
