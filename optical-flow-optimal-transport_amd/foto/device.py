"""Device buffers: GPU-resident frames in, GPU-resident flow out (include/foto.h, *_dev).

``DeviceArray``   owned device memory over foto_dev_malloc / free / memcpy, with
                  ``__cuda_array_interface__`` (v3), so it needs no other GPU library and any
                  consumer of that interface (torch.as_tensor, cupy.asarray) can wrap it.
``as_image``      anything exposing ``__cuda_array_interface__`` (a torch ROCm tensor, a
                  DeviceArray, a strided view of either) -> the C ABI's foto_image.
``bb_flow`` / ``gn_flow``  the two solvers on device frames, through the context / plan caches.
``prepare_pair``  grey, resize and pair normalisation of two device frames ahead of a solve.

This module never imports torch.  One HIP runtime per process: torch bundles its own
libamdhip64, and device pointers of one runtime mean nothing to another -- import torch before
the first foto call, so that libfoto binds to torch's copy (``runtime_check``).
"""
import ctypes
import os
import sys

import numpy as np

from . import _lib
from ._lib import FotoError, check, lib

_DTYPES = {"|u1": (_lib.FOTO_U8, np.uint8), "<f4": (_lib.FOTO_F32, np.float32), "<f8": (_lib.FOTO_F64, np.float64)}
_OUT_DTYPES = {"float32": _lib.FOTO_F32, "float64": _lib.FOTO_F64}
_LAYOUTS = {"planar": 0, "interleaved": 1}
H2D, D2H, D2D = 0, 1, 2


def mapped_hip_runtimes():
    """The distinct libamdhip64 files mapped into this process (/proc/self/maps)."""
    found = []
    try:
        with open("/proc/self/maps") as f:
            for line in f:
                path = line.rstrip("\n").split(None, 5)[-1] if line.count(" ") >= 5 else ""
                if os.path.basename(path).startswith("libamdhip64"):
                    real = os.path.realpath(path)
                    if real not in found:
                        found.append(real)
    except OSError:
        pass
    return found


def runtime_check():
    """Raise FotoError when more than one HIP runtime is mapped: device pointers handed from one
    (torch's) to the other (libfoto's) would be meaningless.  Returns the mapped runtime files."""
    found = mapped_hip_runtimes()
    if len(found) > 1:
        raise FotoError("two HIP runtimes are mapped into this process: " + " and ".join(found) +
                        "; device pointers cannot cross them.  Rule: import torch before the first foto call "
                        "(libfoto then binds to torch's libamdhip64)")
    return found


_INDEX_DTYPES = ("<i4", "<u8")   # foto.match's indices, distances and descriptor words: no frame, no flow


def _typestr(dtype):
    dt = np.dtype(dtype)
    ts = dt.str if dt.itemsize > 1 else "|" + dt.str[1:]
    if ts not in _DTYPES and ts not in _INDEX_DTYPES:
        raise ValueError(f"dtype {dt}: device arrays hold uint8, float32 or float64 (and int32 / uint64 tables)")
    return ts


def packed_strides(shape, item):
    """The byte strides of a C-contiguous array of ``shape``."""
    st, acc = [], item
    for s in reversed(tuple(shape)):
        st.append(acc)
        acc *= max(s, 1)
    return tuple(reversed(st))


def c_contiguous(shape, strides, item):
    """Whether byte ``strides`` (None: packed) lay ``shape`` out C-contiguously: the one such test
    of the package (DeviceArray.contiguous and every device argument that must be packed)."""
    if strides is None:
        return True
    acc = item
    for s, st in zip(reversed(tuple(shape)), reversed(tuple(strides))):
        if s > 1 and st != acc:
            return False
        acc *= s
    return True


class _Owner:
    """One foto_dev_malloc allocation, freed with its last DeviceArray view."""

    def __init__(self, nbytes):
        self.nbytes = int(nbytes)
        p = ctypes.c_void_p()
        check(lib().foto_dev_malloc(self.nbytes, ctypes.byref(p)))
        self.ptr = p.value

    def free(self):
        if self.ptr:
            lib().foto_dev_free(ctypes.c_void_p(self.ptr))
            self.ptr = None

    def __del__(self):
        if sys.is_finalizing():   # the HIP runtime may already be torn down
            return
        try:
            self.free()
        except Exception:
            pass


class DeviceArray:
    """A (possibly strided) array in device memory.  ``DeviceArray(shape, dtype)`` allocates;
    basic slicing, ``.T`` and integer indexing give views that share the allocation."""

    def __init__(self, shape, dtype=np.float64, *, _owner=None, _offset=0, _strides=None):
        self.shape = tuple(int(s) for s in (shape if isinstance(shape, (tuple, list)) else (shape,)))
        self.dtype = np.dtype(dtype)
        self.typestr = _typestr(self.dtype)
        size = int(np.prod(self.shape, dtype=np.int64)) if self.shape else 1
        self._owner = _owner if _owner is not None else _Owner(max(size * self.dtype.itemsize, 1))
        self._offset = int(_offset)
        if _strides is None:
            _strides = packed_strides(self.shape, self.dtype.itemsize)
        self.strides = tuple(int(s) for s in _strides)

    # ---------------------------------------------------------------- interface
    @property
    def ptr(self):
        return self._owner.ptr + self._offset

    @property
    def size(self):
        return int(np.prod(self.shape, dtype=np.int64)) if self.shape else 1

    @property
    def ndim(self):
        return len(self.shape)

    @property
    def contiguous(self):
        return c_contiguous(self.shape, self.strides, self.dtype.itemsize)

    @property
    def __cuda_array_interface__(self):
        return {"shape": self.shape, "typestr": self.typestr, "data": (self.ptr, False), "version": 3,
                "strides": None if self.contiguous else self.strides}

    def _host_view(self, host):
        """This array's shape / strides over `host`, a uint8 host copy of the whole allocation."""
        n = (host.size - self._offset) // self.dtype.itemsize * self.dtype.itemsize
        base = host[self._offset:self._offset + n].view(self.dtype)
        return np.lib.stride_tricks.as_strided(base, shape=self.shape, strides=self.strides, writeable=False)

    # ---------------------------------------------------------------- host <-> device
    @classmethod
    def from_numpy(cls, a):
        a = np.ascontiguousarray(a)
        d = cls(a.shape, a.dtype)
        if a.nbytes:
            check(lib().foto_dev_memcpy(ctypes.c_void_p(d.ptr), a.ctypes.data_as(ctypes.c_void_p), a.nbytes, H2D))
        return d

    def to_numpy(self):
        host = np.empty(self._owner.nbytes, dtype=np.uint8)
        check(lib().foto_dev_memcpy(host.ctypes.data_as(ctypes.c_void_p), ctypes.c_void_p(self._owner.ptr),
                                    host.nbytes, D2H))
        return np.array(self._host_view(host))   # a contiguous, owned copy

    def copy_from(self, other):
        """Device-to-device copy of a same-shape contiguous array into this contiguous one."""
        if not (self.contiguous and other.contiguous) or self.shape != other.shape or self.dtype != other.dtype:
            raise ValueError("copy_from: same shape and dtype, both contiguous")
        check(lib().foto_dev_memcpy(ctypes.c_void_p(self.ptr), ctypes.c_void_p(other.ptr),
                                    self.size * self.dtype.itemsize, D2D))
        return self

    # ---------------------------------------------------------------- views
    def _view(self, fn):
        # numpy works out shape / strides / offset of the view on an array that is never read
        probe = np.lib.stride_tricks.as_strided(np.empty(1, self.dtype), shape=self.shape, strides=self.strides,
                                                writeable=False)
        v = fn(probe)
        off = v.__array_interface__["data"][0] - probe.__array_interface__["data"][0]
        return DeviceArray(v.shape, self.dtype, _owner=self._owner, _offset=self._offset + off, _strides=v.strides)

    def __getitem__(self, key):
        keys = key if isinstance(key, tuple) else (key,)
        if not all(isinstance(k, (slice, type(Ellipsis))) or (isinstance(k, (int, np.integer))) for k in keys):
            raise TypeError("DeviceArray: basic indexing only (integers, slices, Ellipsis)")
        # (an integer index becomes a length-1 slice and is squeezed: numpy would return a scalar)
        norm = tuple(slice(k, k + 1 if k != -1 else None) if isinstance(k, (int, np.integer)) else k for k in keys)
        drop = [i for i, k in enumerate(self._expand(keys)) if isinstance(k, (int, np.integer))]
        v = self._view(lambda p: p[norm])
        if drop:
            shape = tuple(s for i, s in enumerate(v.shape) if i not in drop)
            strides = tuple(s for i, s in enumerate(v.strides) if i not in drop)
            v = DeviceArray(shape, self.dtype, _owner=self._owner, _offset=v._offset, _strides=strides)
        return v

    def _expand(self, keys):
        """keys with an Ellipsis spelled out, one entry per axis"""
        n_e = sum(1 for k in keys if k is Ellipsis)
        if n_e > 1:
            raise IndexError("an index can only have a single ellipsis")
        out = []
        for k in keys:
            if k is Ellipsis:
                out.extend([slice(None)] * (self.ndim - (len(keys) - 1)))
            else:
                out.append(k)
        if len(out) > self.ndim:
            raise IndexError("too many indices for DeviceArray")
        return out + [slice(None)] * (self.ndim - len(out))

    @property
    def T(self):
        return self._view(lambda p: p.T)

    def reshape(self, *shape):
        if not self.contiguous:
            raise ValueError("reshape: contiguous arrays only")
        shape = shape[0] if len(shape) == 1 and isinstance(shape[0], (tuple, list)) else shape
        probe = np.lib.stride_tricks.as_strided(np.empty(1, self.dtype), shape=self.shape, strides=self.strides,
                                                writeable=False)
        v = probe.reshape(shape)
        return DeviceArray(v.shape, self.dtype, _owner=self._owner, _offset=self._offset, _strides=v.strides)

    def __repr__(self):
        return f"DeviceArray(shape={self.shape}, dtype={self.dtype}, strides={self.strides}, ptr=0x{self.ptr:x})"


# -------------------------------------------------------------------- descriptors

def _interface(obj):
    """(ptr, typestr, shape, byte strides or None, stream entry or None) of obj."""
    if isinstance(obj, dict):
        d = obj
    else:
        d = getattr(obj, "__cuda_array_interface__", None)
        if d is None:
            raise TypeError(f"{type(obj).__name__} does not expose __cuda_array_interface__ (a device array, e.g. a "
                            "torch ROCm tensor or a foto.device.DeviceArray, is required)")
    if "ptr" in d:   # the explicit (ptr, typestr, shape, strides) mapping
        ptr = d["ptr"]
    else:
        ptr = d["data"][0]
    return int(ptr or 0), str(d["typestr"]), tuple(int(s) for s in d["shape"]), d.get("strides"), d.get("stream")


def device_interface(obj):
    """_interface of a device argument.  A foreign object's pointers come from whichever HIP
    runtime its library uses, so runtime_check first; a DeviceArray's are libfoto's own."""
    if not isinstance(obj, DeviceArray):
        runtime_check()
    return _interface(obj)


def make_image(ptr, code, stride_y, stride_x, divisor, shape, keep):
    """The _lib.Image of a frame: element strides, ``divisor`` None = 255 for uint8 and 1 otherwise;
    carries ``.shape`` = (h, w) and keeps ``keep`` alive."""
    im = _lib.Image()
    im.data, im.dtype = ptr, code
    im.stride_y, im.stride_x = stride_y, stride_x
    im.divisor = float(divisor) if divisor is not None else (255.0 if code == _lib.FOTO_U8 else 1.0)
    im.shape = (int(shape[0]), int(shape[1]))
    im._keep = keep
    return im


def stream_handle(stream=None, *objs):
    """The hipStream_t (as an integer; 0 = the legacy null stream) for a call: an explicit
    ``stream`` (an integer handle, or an object with ``.cuda_stream`` such as torch.cuda.Stream),
    else the "stream" entry of the first object's interface that has one (1 = legacy default,
    2 = per-thread default), else null."""
    if stream is None:
        for o in objs:
            try:
                s = _interface(o)[4]
            except (TypeError, KeyError):
                s = None
            if s is not None:
                stream = s
                if stream == 0:
                    raise ValueError("__cuda_array_interface__: stream 0 is not allowed (1 is the legacy default stream)")
                return 0 if stream == 1 else int(stream)
        return 0
    if hasattr(stream, "cuda_stream"):
        stream = stream.cuda_stream
    return int(stream)


def as_image(obj, divisor=None):
    """The foto_image of a 2-D uint8 / float32 / float64 device array (rows = y, columns = x).
    ``divisor`` defaults to 255 for uint8 and 1 otherwise: value = float64(pixel) / divisor.
    The returned ``_lib.Image`` carries ``.shape`` = (h, w) and keeps ``obj`` alive."""
    if isinstance(obj, _lib.Image):
        return obj
    ptr, typestr, shape, strides, _ = device_interface(obj)
    if typestr not in _DTYPES:
        raise TypeError(f"typestr {typestr!r}: frames are uint8 ('|u1'), float32 ('<f4') or float64 ('<f8')")
    if len(shape) != 2:
        raise ValueError(f"shape {shape}: a frame is a 2-D (height, width) array; take one channel of a colour image")
    code, npdt = _DTYPES[typestr]
    item = np.dtype(npdt).itemsize
    h, w = shape
    if strides is None:
        strides = (w * item, item)
    sy, sx = (int(s) for s in strides)
    if sy % item or sx % item:
        raise ValueError(f"byte strides {(sy, sx)} are not multiples of the {item}-byte item size")
    return make_image(ptr, code, sy // item, sx // item, divisor, (h, w), obj)


def _pair(f0, f1, divisor=None):
    a, b = as_image(f0, divisor), as_image(f1, divisor)
    if a.shape != b.shape:
        raise ValueError(f"frames differ in shape: {a.shape} and {b.shape}")
    return a, b


def export_target(out, dtype, layout, h, w):
    """(DeviceArray or the caller's object, pointer, dtype code, layout code) of a flow export."""
    dtype = _dtype_name(dtype, _OUT_DTYPES, None)   # (a wrong dtype is reported before a wrong layout)
    if layout not in _LAYOUTS:
        raise ValueError(f"layout {layout!r}: 'planar' ([3][h][w] = u, v, m) or 'interleaved' ([h][w][2] = (u, v))")
    shape = (3, h, w) if layout == "planar" else (h, w, 2)
    out, ptr, code = _shaped_target(out, dtype, _OUT_DTYPES, shape, None)
    return out, ptr, code, _LAYOUTS[layout]


_FRAME_DTYPES = {"uint8": _lib.FOTO_U8, "float32": _lib.FOTO_F32, "float64": _lib.FOTO_F64}


def _dtype_name(dtype, codes, what):
    """The key of ``codes`` that ``dtype`` (a name, or anything np.dtype takes) stands for; the
    ValueError names ``what`` the values are (None: a flow export's own wording)."""
    if dtype not in codes:
        dtype = np.dtype(dtype).name
    if dtype not in codes:
        raise ValueError(f"dtype {dtype!r}: " + (f"{what} are " if what else "") + " or ".join(repr(k) for k in codes))
    return dtype


def _shaped_target(out, dtype, codes, shape, what):
    """(DeviceArray or the caller's object, pointer, dtype code): a new DeviceArray of ``shape``
    or the caller's ``out``, which must be C-contiguous device memory of that dtype and shape.
    ValueError before the library is touched."""
    dtype = _dtype_name(dtype, codes, what)
    if out is None:
        out = DeviceArray(shape, dtype)
        return out, out.ptr, codes[dtype]
    ptr, typestr, oshape, strides, _ = device_interface(out)
    if typestr != _typestr(dtype) or tuple(oshape) != tuple(shape):
        raise ValueError(f"out: expected {dtype} of shape {tuple(shape)}, got {typestr} of shape {tuple(oshape)}")
    if not c_contiguous(shape, strides, np.dtype(dtype).itemsize):
        raise ValueError("out must be C-contiguous")
    return out, ptr, codes[dtype]


def frame_positions(s, Nt):
    """The plane positions of a frames export as a float64 vector: an int K means
    np.linspace(0, Nt - 1, K), a sequence is taken as it is (one dimension)."""
    if isinstance(s, (int, np.integer)) and not isinstance(s, (bool, np.bool_)):
        if s < 1:
            raise ValueError(f"frames: K = {s} must be >= 1")
        return np.linspace(0.0, float(Nt - 1), int(s))
    a = np.asarray(s, dtype=np.float64)
    if a.ndim != 1:
        raise ValueError(f"frames: s of shape {a.shape}; an int K or a 1-D sequence of plane positions")
    return np.ascontiguousarray(a)


def frames_target(out, dtype, count, h, w):
    """(out, pointer, dtype code) of a frames export: [count][h][w] of uint8 | float32 | float64."""
    return _shaped_target(out, dtype, _FRAME_DTYPES, (int(count), h, w), "frames")


def path_target(out, dtype, layout, Nt, h, w):
    """(out, pointer, dtype code, layout code) of a flow-path export: Nt - 1 records of
    export_target's shape, [Nt-1][3][h][w] planar or [Nt-1][h][w][2] interleaved."""
    if layout not in _LAYOUTS:
        raise ValueError(f"layout {layout!r}: 'planar' ([Nt-1][3][h][w] = u, v, m) or 'interleaved' "
                         "([Nt-1][h][w][2] = (u, v))")
    shape = (Nt - 1, 3, h, w) if layout == "planar" else (Nt - 1, h, w, 2)
    out, ptr, code = _shaped_target(out, dtype, _OUT_DTYPES, shape, "flow records")
    return out, ptr, code, _LAYOUTS[layout]


def track_points(points):
    """Host start points as a C-contiguous float64 (M, 2) array: anything np.asarray turns into
    (M, 2); a single (2,) point is promoted to M = 1.  ValueError otherwise."""
    a = np.asarray(points, dtype=np.float64)
    if a.shape == (2,):
        a = a.reshape(1, 2)
    if a.ndim != 2 or a.shape[1] != 2:
        raise ValueError(f"points of shape {a.shape}: an (M, 2) array of (x, y) start points, or one (2,) point")
    return np.ascontiguousarray(a)


def track_source(points):
    """(pointer, dtype code, M) of device start points: a C-contiguous (M, 2) float32 | float64
    device array.  ValueError before the library is touched."""
    ptr, typestr, shape, strides, _ = device_interface(points)
    if typestr not in ("<f4", "<f8"):
        raise ValueError(f"points: typestr {typestr!r}; device start points are float32 or float64")
    if len(shape) != 2 or shape[1] != 2:
        raise ValueError(f"points of shape {shape}: a device (M, 2) array of (x, y) start points")
    if not c_contiguous(shape, strides, np.dtype(typestr).itemsize):
        raise ValueError("points must be C-contiguous")
    return ptr, _DTYPES[typestr][0], int(shape[0])


def track_target(out, dtype, R, M):
    """(out, pointer, dtype code) of a point-tracking export: [R][M][2] of float32 | float64."""
    return _shaped_target(out, dtype, _OUT_DTYPES, (int(R), int(M), 2), "track records")


def maps_target(out, dtype, count, h, w):
    """(out, pointer, dtype code) of a maps export: [count][4][h][w] of float32 | float64."""
    return _shaped_target(out, dtype, _OUT_DTYPES, (int(count), 4, h, w), "maps")


def interp_frames(frame0, frame1, channels_last=True, divisor=None):
    """The two frames of an in-between as (image 0, image 1, channels, stride_c0, stride_c1,
    has_channel_axis, dtype name): device arrays (h, w), (h, w, C) or (C, h, w) of the same shape
    (foto.render.source_arg's rules; dtypes and strides may differ).  ValueError before the library
    is touched."""
    from .render import source_arg
    a, C, sc0, has_c = source_arg(frame0, channels_last, divisor)
    b, C1, sc1, has_c1 = source_arg(frame1, channels_last, divisor)
    if a.shape != b.shape or C != C1 or has_c != has_c1:
        raise ValueError(f"frames differ in shape: {a.shape} x {C} and {b.shape} x {C1} (h x w x channels)")
    name = {v[0]: np.dtype(v[1]).name for v in _DTYPES.values()}[a.dtype]
    return a, b, C, sc0, sc1, has_c, name


def interp_target(out, dtype, count, h, w, C, has_c):
    """(out, pointer, dtype code) of an in-between export: [count][h][w][C] (no channel axis for
    2-D frames) of uint8 | float32 | float64."""
    return _shaped_target(out, dtype, _FRAME_DTYPES, (int(count), h, w) + ((C,) if has_c else ()), "in-betweens")


def report_target(out, Nt):
    """(out, pointer) of a transport-report export: a new DeviceArray or the caller's ``out``,
    C-contiguous float64 of shape (Nt, 8).  ValueError before the library is touched."""
    from .report import REPORT_COLS
    out, ptr, _ = _shaped_target(out, "float64", {"float64": _lib.FOTO_F64}, (int(Nt), REPORT_COLS), "report tables")
    return out, ptr


# -------------------------------------------------------------------- convenience

def prepare_pair(c0, c1, size=None, filter="lanczos", normalize=True, *, channels_last=True, stream=None):
    """Two grey or colour device frames made ready for bb_flow / gn_flow / tvl1_flow / bb_sequence
    without leaving the device (foto.prep): colour frames ((h, w, 3 | 4), or (3 | 4, h, w) with
    ``channels_last=False``) go through PIL's convert('L'); ``size`` ((ow, oh), "WxH" or a scale
    factor; None: as they are) through PIL's Image.resize with ``filter``; ``normalize`` through
    bin/normalize_image.py's mass equalisation, written as uint8 like the tool's PNGs.  The stages
    run.sh:18-70 applies before main.py.  Returns the two device images."""
    from . import prep
    frames = []
    for f in (c0, c1):
        if len(_interface(f)[2]) == 3:
            f = prep.gray(f, channels_last=channels_last, stream=stream)
        if size is not None:
            f = prep.resize(f, size, filter, stream=stream)
        frames.append(f)
    a, b = frames
    if as_image(a).shape != as_image(b).shape:
        raise ValueError(f"frames differ in shape: {as_image(a).shape} and {as_image(b).shape}")
    if normalize:
        a, b, _ = prep.normalize_pair(a, b, dtype="uint8", stream=stream)
    return a, b


def _bb_solved(f0, f1, Nt, r, convergence_tol, reg_epsilon, max_it, normalize, stream, opts, run, *more):
    """The frame of bb_flow, bb_path and bb_track: the pair solved with the reference's stop rules
    on the cached context (foto.bb.cached_solver's, reset to this pair) or, the cache off, on a
    fresh one, then ``run(solver, stream handle)``; ``more``: further arguments that may name the
    stream."""
    from . import bb
    a, b = _pair(f0, f1)
    st = stream_handle(stream, f0, f1, *more)

    def go(s):
        s.iterate(max_it, convergence_tol=convergence_tol, stop_rules=True)
        return run(s, st)

    return bb.on_context(
        opts, lambda: bb.cached_solver_device(a, b, Nt, r, reg_epsilon, normalize=normalize, stream=st, **opts),
        lambda: bb.BBSolver.from_device(a, b, Nt, r=r, reg_epsilon=reg_epsilon, normalize=normalize, stream=st, **opts),
        go)


def bb_flow(f0, f1, Nt, r=1.0, convergence_tol=0.3, reg_epsilon=1e-3, max_it=100, *, normalize=False,
            dtype="float32", layout="planar", out=None, stream=None, **opts):
    """benamou_brenier.solve on device frames, the flow left on the device: a context from the
    cache (foto.bb.cached_solver's, reset to this pair), the reference's stop rules, one export.
    Returns the DeviceArray (or ``out``)."""
    return _bb_solved(f0, f1, Nt, r, convergence_tol, reg_epsilon, max_it, normalize, stream, opts,
                      lambda s, st: s.flow_device(out=out, dtype=dtype, layout=layout, stream=st))


def bb_sequence(frames, Nt, r=1.0, convergence_tol=0.3, reg_epsilon=1e-3, max_it=100, *, normalize=False,
                dtype="float32", layout="planar", out=None, stream=None, **opts):
    """bb_flow for every consecutive pair of ``frames`` -- a sequence of K + 1 device frames (or one
    (K + 1, h, w) device array) -- into one flow buffer of K records, [K][3][h][w] planar or
    [K][h][w][2] interleaved: record k is bb_flow(frames[k], frames[k + 1]), exported into its view
    of the buffer by the one cached context, reset per pair.  Returns the DeviceArray (or ``out``):
    what ``foto.chain.compose`` takes as it is."""
    n = int(frames.shape[0]) if hasattr(frames, "shape") else len(frames)
    if n < 2:
        raise ValueError(f"bb_sequence: {n} frames; a sequence has at least 2")
    frs = [frames[k] for k in range(n)]
    h, w = as_image(frs[0]).shape
    out, _, _, _ = path_target(out, dtype, layout, n, h, w)   # (K = n - 1 records)
    for k in range(n - 1):
        bb_flow(frs[k], frs[k + 1], Nt, r, convergence_tol, reg_epsilon, max_it, normalize=normalize, dtype=dtype,
                layout=layout, out=out[k], stream=stream, **opts)
    return out


def bb_path(f0, f1, Nt, r=1.0, convergence_tol=0.3, reg_epsilon=1e-3, max_it=100, *, frames=None, normalize=False,
            frame_dtype="float32", dtype="float32", layout="planar", frames_out=None, out=None, stream=None,
            **opts):
    """bb_flow with the transport path instead of its end point: the same solve on the cached
    context, then ``frames`` in-between density frames (an int K: np.linspace(0, Nt-1, K), or a
    sequence of plane positions; default Nt: every plane) and the Nt - 1 partial flows, both left
    on the device.  With ``normalize`` the frames are scaled by the frame-0 sum, back to the
    intensity range of ``f0``.  Returns (frames [K][h][w], flow path [Nt-1][3][h][w] or
    [Nt-1][h][w][2]); the last flow record is bb_flow's result."""
    pos = Nt if frames is None else frames

    def run(s, st):
        fr = s.frames_device(pos, scale=s.sums[0] if normalize else 1.0, out=frames_out, dtype=frame_dtype, stream=st)
        return fr, s.flow_path_device(out=out, dtype=dtype, layout=layout, stream=st)

    return _bb_solved(f0, f1, Nt, r, convergence_tol, reg_epsilon, max_it, normalize, stream, opts, run)


def bb_track(f0, f1, Nt, points, r=1.0, convergence_tol=0.3, reg_epsilon=1e-3, max_it=100, *, normalize=False,
             all_steps=True, dtype="float32", out=None, stream=None, **opts):
    """bb_flow for a caller's own points instead of the pixel grid: the same solve on the cached
    context, then the trajectories of the device start points ``points`` ((M, 2) float32 |
    float64, (x, y) in pixel-index coordinates) left on the device.  Returns [Nt-1][M][2]
    displacements (``all_steps``) or [1][M][2], the last record: where bb_flow moves each point."""
    return _bb_solved(f0, f1, Nt, r, convergence_tol, reg_epsilon, max_it, normalize, stream, opts,
                      lambda s, st: s.track_device(points, out=out, dtype=dtype, all_steps=all_steps, stream=st),
                      points)


def bb_interpolate(f0, f1, Nt, times, r=1.0, convergence_tol=0.3, reg_epsilon=1e-3, max_it=100, *, normalize=False,
                   inv_iters=_lib.FOTO_INV_ITERS_DEFAULT, dtype=None, out=None, stream=None, channels_last=True,
                   colour0=None, colour1=None, **opts):
    """bb_flow's solve on the cached context, then motion-compensated in-betweens of the caller's own
    frames at plane positions ``times`` (an int K: np.linspace(0, Nt-1, K), or a sequence in
    [0, Nt-1]), left on the device: BBSolver.interpolate.  The solve runs on the grey-scale pair
    ``f0``, ``f1``; ``colour0`` / ``colour1`` (device (h, w, C) or (C, h, w) arrays, e.g. the RGB
    frames the grey pair came from) are what is interpolated instead, when given.  Returns
    [K][h][w] or [K][h][w][C] (``dtype`` None: the frames' own); times 0 and Nt-1 give the two
    frames back bit for bit."""
    g0 = f0 if colour0 is None else colour0
    g1 = f1 if colour1 is None else colour1
    return _bb_solved(f0, f1, Nt, r, convergence_tol, reg_epsilon, max_it, normalize, stream, opts,
                      lambda s, st: s.interpolate(g0, g1, times, inv_iters=inv_iters, dtype=dtype, out=out, stream=st,
                                                  channels_last=channels_last), g0, g1)


def bb_report(f0, f1, Nt, r=1.0, convergence_tol=0.3, reg_epsilon=1e-3, max_it=100, *, normalize=False, stream=None,
              **opts):
    """bb_flow's solve on the cached context, then the transport report of its last outer
    iteration instead of the flow: a foto.report.TransportReport (BBSolver.report())."""
    return _bb_solved(f0, f1, Nt, r, convergence_tol, reg_epsilon, max_it, normalize, stream, opts,
                      lambda s, st: s.report())


def gn_flow(f0, f1, alpha, lam, *, dtype="float32", layout="planar", out=None, stream=None, levels=1, warps=1):
    """classical.GLLOpticalFlow.process on device frames (the plan from foto.gn's cache); returns
    the DeviceArray (or ``out``) holding u, v, m.  levels / warps other than (1, 1): the
    coarse-to-fine scheme for displacements beyond a pixel (foto.gn.Pyramid, cached likewise)."""
    from . import gn
    a, b = _pair(f0, f1)
    h, w = a.shape
    if (int(levels), int(warps)) != (1, 1):
        p = gn.cached_pyramid(w, h, alpha, lam, levels=levels, warps=warps)
        return p.solve_device(a, b, out=out, dtype=dtype, layout=layout, stream=stream_handle(stream, f0, f1))[0]
    p = gn.cached_plan(w, h, alpha, lam)
    return p.solve_device(a, b, out=out, dtype=dtype, layout=layout, stream=stream_handle(stream, f0, f1))[0]


def tvl1_flow(f0, f1, *, dtype="float32", layout="planar", out=None, stream=None, **opts):
    """Duality-based TV-L1 flow with an illumination channel on device frames (the solver from
    foto.tvl1's cache; ``opts`` are foto.tvl1.DEFAULTS' keys); returns the DeviceArray (or ``out``)
    holding u, v, m: a flow buffer foto.chain, foto.filter, foto.render and foto.evaluate take as
    it is."""
    from . import tvl1
    a, b = _pair(f0, f1)
    h, w = a.shape
    p = tvl1.cached_tvl1(w, h, **opts)
    return p.solve_device(a, b, out=out, dtype=dtype, layout=layout, stream=stream_handle(stream, f0, f1))[0]


def sinkhorn_flow(f0, f1, *, eps=2.0, radius=16, iters=100, dtype="float32", layout="planar", out=None, stream=None):
    """Entropic optimal transport between two device frames as a flow (the solver from
    foto.sinkhorn's cache): ``iters`` Sinkhorn iterations with the Gaussian kernel of variance
    ``eps`` px^2 in a window of ``radius``, then the plan's barycentric projection, frame 0 -> frame
    1; returns the DeviceArray (or ``out``) holding u, v, m (m = 0): a flow buffer foto.chain,
    foto.filter, foto.render, foto.evaluate and foto.motion.fit_flow take as it is.  The masses are
    the caller's (``prepare_pair`` equalises them)."""
    from . import sinkhorn
    a, b = _pair(f0, f1)
    h, w = a.shape
    p = sinkhorn.cached_sinkhorn(w, h, eps, radius)
    return p.solve_device(a, b, iters, out=out, dtype=dtype, layout=layout, stream=stream_handle(stream, f0, f1))


def lk_track(f0, f1, points_or_count, *, check=False, fb_tol=0.5, dtype="float32", stream=None, corner_opts=None,
             **opts):
    """Pyramidal Lucas-Kanade on device frames (the tracker from foto.sparse's cache; ``opts`` are
    foto.sparse.LK_DEFAULTS' keys): the classical sparse baseline of bb_track, on the same points.
    ``points_or_count``: device start points ((M, 2) float32 | float64), or an int K -- then the K
    strongest Shi-Tomasi corners of ``f0`` (``corner_opts``: foto.sparse.CORNER_DEFAULTS' keys), M
    = their count.  Returns (points (M, 2), disp (M, 2), status (M,), err (M,)) and, with
    ``check``, fb (M,) after them: foto.sparse.LK.track's results, everything left on the device."""
    from . import sparse
    a, b = _pair(f0, f1)
    h, w = a.shape
    st = stream_handle(stream, f0, f1)
    pts = points_or_count
    if isinstance(pts, (int, np.integer)) and not isinstance(pts, (bool, np.bool_)):
        pts, count = sparse.corners(a, int(pts), dtype=dtype, stream=st, **(corner_opts or {}))
        if count < 1:
            raise FotoError("lk_track: the frame has no corner to track")
        pts = pts[:count]
    p = sparse.cached_lk(w, h, **opts).set_frames(a, b, stream=st)
    return (pts,) + tuple(p.track(pts, check=check, fb_tol=fb_tol, dtype=dtype, stream=st))


def global_motion(f0, f1, model="affine", max_corners=1024, *, threshold=1.0, rounds=3, samples=None, min_inliers=0,
                  fb_tol=0.5, dtype="float32", stream=None, corner_opts=None, **opts):
    """The global motion between two device frames: the ``max_corners`` strongest Shi-Tomasi
    corners of ``f0`` (``corner_opts``: foto.sparse.CORNER_DEFAULTS' keys), tracked forward and
    backward by the cached Lucas-Kanade tracker (``opts``: foto.sparse.LK_DEFAULTS' keys), and
    ``foto.motion.fit`` with LK's status bytes, all on one stream and with nothing downloaded (the
    corner count stays on the device: rows beyond it are NaN, which the tracker marks and the fit
    leaves out).  Returns (fit, points, disp, status): a foto.motion.Fit and the device arrays it
    was fitted to.  ``foto.render.reconstruct(f1, foto.motion.field(fit, w, h))`` stabilises."""
    from . import motion, sparse
    a, b = _pair(f0, f1)
    h, w = a.shape
    st = stream_handle(stream, f0, f1)
    pts, _ = sparse.corners(a, int(max_corners), dtype=dtype, stream=st, wait=False, **(corner_opts or {}))
    p = sparse.cached_lk(w, h, **opts).set_frames(a, b, stream=st)
    disp, status, _, _ = p.track(pts, check=True, fb_tol=fb_tol, dtype=dtype, stream=st)
    fit = motion.fit(pts, disp, w, h, model, status=status, threshold=threshold, rounds=rounds, samples=samples,
                     min_inliers=min_inliers, stream=st)
    return fit, pts, disp, status


_DESCRIBE_KEYS, _MATCH_KEYS = ("blur", "patch", "orientations", "seed", "table"), ("max_disp", "max_dist", "ratio")


def match_frames(f0, f1, max_corners=1024, *, check=True, corner_opts=None, dtype="float32", stream=None, **opts):
    """Wide-baseline correspondences between two device frames (foto.match): the ``max_corners``
    strongest Shi-Tomasi corners of each frame (``corner_opts``: foto.sparse.CORNER_DEFAULTS' keys,
    the margin raised to at least the patch radius), their binary descriptors, the nearest frame-1
    corner of every frame-0 corner under the Hamming distance and, with ``check``, the mutual
    check.  ``opts``: foto.match.describe's blur, patch, orientations, seed, table and
    foto.match.match's max_disp, max_dist, ratio.  All on one stream and with nothing downloaded
    (the corner counts stay on the device: rows beyond them are NaN, which ``describe`` marks and the
    matcher leaves out).  Returns (points (M, 2), disp (M, 2), status (M,), idx (M,), dist (M, 2)):
    what lk_track's callers and foto.motion.fit take as they are."""
    from . import match as MT
    from . import sparse
    a, b = _pair(f0, f1)
    st = stream_handle(stream, f0, f1)
    unknown = set(opts) - set(_DESCRIBE_KEYS) - set(_MATCH_KEYS)
    if unknown:
        raise TypeError(f"matching options are {sorted(_DESCRIBE_KEYS + _MATCH_KEYS)}; got {sorted(unknown)}")
    d_opts = {k: opts[k] for k in _DESCRIBE_KEYS if k in opts}
    m_opts = {k: opts[k] for k in _MATCH_KEYS if k in opts}
    co = dict(sparse.CORNER_DEFAULTS, **(corner_opts or {}))
    co["margin"] = max(int(co["margin"]), int(d_opts.get("patch", MT.DESCRIBE_DEFAULTS["patch"])))
    p0, _ = sparse.corners(a, int(max_corners), dtype=dtype, stream=st, wait=False, **co)
    p1, _ = sparse.corners(b, int(max_corners), dtype=dtype, stream=st, wait=False, **co)
    d0, s0 = MT.describe(a, p0, stream=st, **d_opts)
    d1, s1 = MT.describe(b, p1, stream=st, **d_opts)
    idx, dist, status, disp = MT.match(d0, s0, p0, d1, s1, p1, dtype=dtype, stream=st, **m_opts)
    if check:
        idx10 = MT.match(d1, s1, p1, d0, s0, p0, dtype=dtype, stream=st, **m_opts)[0]
        MT.cross(idx, idx10, status, stream=st)
    return p0, disp, status, idx, dist


def match_motion(f0, f1, model="affine", max_corners=1024, *, threshold=1.0, rounds=3, samples=None, min_inliers=0,
                 check=True, dtype="float32", stream=None, corner_opts=None, **opts):
    """global_motion with ``match_frames`` in the tracker's place: the global motion between two
    device frames that may be a large pan or a roll apart.  Returns (fit, points, disp, status)."""
    from . import motion
    a, b = _pair(f0, f1)
    h, w = a.shape
    st = stream_handle(stream, f0, f1)
    pts, disp, status, _, _ = match_frames(a, b, max_corners, check=check, corner_opts=corner_opts, dtype=dtype,
                                           stream=st, **opts)
    fit = motion.fit(pts, disp, w, h, model, status=status, threshold=threshold, rounds=rounds, samples=samples,
                     min_inliers=min_inliers, stream=st)
    return fit, pts, disp, status
