"""The plumbing between a wrapper and a library call, each piece written once.  torch is imported inside the functions, so
host-only use does not import it."""
import ctypes
import math

import numpy as np

from . import _lib

SLOT = 256
_MAP_KINDS = {"uint8": "a uint8", "int32": "an int32"}
# host_image_ptrs: (a tensor that is no contiguous uint8 CPU tensor, a tensor that is not [h,w,3], an array that is not)
_IMAGE_ERRORS = {"crop": ("crop %d: expected a contiguous uint8 [h,w,3] CPU tensor",) * 2 + ("crop %d: expected uint8 [h,w,3]",),
                 "window": ("window %d: expected a contiguous uint8 CPU tensor",) + ("window %d: expected uint8 [H,W,3], every window of one size",) * 2}


def bound(entries):
    """_lib.load() with a module's own table {name: (restype, argtypes)} bound; AttributeError where the library does not export
    an entry (there is no fallback)"""
    lib = _lib.load()
    for name, (res, args) in entries.items():
        fn = getattr(lib, name)
        if fn.argtypes != args:
            fn.restype, fn.argtypes = res, args
    return lib


def stream_ptr(device):
    """torch's current stream on `device`, as the hipStream_t argument of a library call"""
    import torch
    return ctypes.c_void_p(torch.cuda.current_stream(device).cuda_stream)


def planned_bytes(fn, *ints):
    """fn(*ints, &bytes) of a gs_*_plan entry -> bytes; GlomsegError where the plan refuses the sizes.  Host-only."""
    need = ctypes.c_size_t(0)
    _lib.check(fn(*[int(v) for v in ints], ctypes.byref(need)))
    return need.value


def device_map(m, dtype, what, upload=False):
    """m as a contiguous 2-D GPU tensor of `dtype` ("uint8" / "int32"), or ValueError("<what> must be ...").  upload: anything that
    is no tensor is taken as a class map in host memory and copied to the current device."""
    import torch
    if upload and not isinstance(m, torch.Tensor):
        m = torch.from_numpy(np.array(m, dtype=dtype)).cuda()      # (a copy: the array may be read-only)
    if not isinstance(m, torch.Tensor) or m.dtype != getattr(torch, dtype) or m.dim() != 2 or not m.is_cuda:
        raise ValueError("%s must be %s [h,w] map on the GPU" % (what, _MAP_KINDS[dtype]))
    return m.contiguous()


def mean_std_arrays(mean_stds, members):
    """[(mean, std), ...] of an ensemble's members -> (means, stds), float arrays of three values for each of `members`"""
    k = ctypes.c_float * (3 * members)
    return k(*[float(v) for ms in mean_stds for v in ms[0]]), k(*[float(v) for ms in mean_stds for v in ms[1]])


def host_image_ptrs(images, what):
    """images: uint8 [h,w,3] numpy arrays or CPU tensors (`what`: "crop" / "window", for the error text) ->
    (pointer array, [(h, w), ...], keep): the address of every image's data, its size, and the objects that own the memory --
    an array that is not contiguous uint8 is converted, and its copy is what `keep` holds for the duration of the call."""
    import torch
    bad_tensor, bad_tensor_shape, bad_shape = _IMAGE_ERRORS[what]
    ptrs, shapes, keep = (ctypes.c_void_p * len(images))(), [], []
    for i, im in enumerate(images):
        if isinstance(im, torch.Tensor):
            if im.is_cuda or im.dtype != torch.uint8 or not im.is_contiguous():
                raise ValueError(bad_tensor % i)
            ptrs[i], bad_shape_i = im.data_ptr(), bad_tensor_shape
        else:
            im = np.ascontiguousarray(im, dtype=np.uint8)
            ptrs[i], bad_shape_i = im.ctypes.data, bad_shape
        if im.ndim != 3 or im.shape[2] != 3:
            raise ValueError(bad_shape_i % i)
        shapes.append((int(im.shape[0]), int(im.shape[1])))
        keep.append(im)
    return ptrs, shapes, keep


def packed_pinned(byte_sizes, pin=True):
    """One pinned uint8 buffer with a slot per size -> (buffer, offsets int64 [n + 1], pointer array [n]).  The slots are
    256 bytes apart or a multiple of it, the alignment of the library's packed device buffer: a batch's maps then sit exactly as
    they do on the device and leave it as one DMA instead of one per crop (gs_espnet_segment_crops_host).  pin=False: pageable
    memory (no device needed)."""
    import torch
    offsets = np.zeros(len(byte_sizes) + 1, dtype=np.int64)
    np.cumsum([(int(s) + SLOT - 1) // SLOT * SLOT for s in byte_sizes], out=offsets[1:])
    buf = torch.empty(int(offsets[-1]), dtype=torch.uint8, pin_memory=pin)
    base = buf.data_ptr()
    return buf, offsets, (ctypes.c_void_p * len(byte_sizes))(*[base + int(o) for o in offsets[:-1]])


def packed_views(buffer, offsets, shapes):
    """the slots of packed_pinned's buffer as numpy views: slot i as uint8 of shapes[i]"""
    flat = buffer.numpy()
    return [flat[int(o):int(o) + math.prod(s)].reshape(s) for o, s in zip(offsets, shapes)]
