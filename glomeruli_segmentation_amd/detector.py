"""The assembled detector behind the reference's ``detect_box`` tensor contract
(module/faster-rcnn/detect_glomus_test.py:349-352, tensors :443-450), running on the GPU through
``gs_detector_*`` (csrc/detector.hip).

The reference's network is an external TensorFlow-1.12 frozen graph (:419-427) whose architecture and weights are
not in the reference, so this is a detector of the same SHAPE with caller-supplied weights; ``synthetic_weights``
makes seeded ones (there is no network to download trained ones from).  Parity with the reference's graph is
unpinned; the graph itself is checked against oracle/detector_oracle.py.

    det = FrcnnDetector(synthetic_weights(seed=0))
    boxes, scores, classes, num = det(window_rgb_u8[None])        # the sess.run of :350-352
"""
import ctypes
from functools import lru_cache

import numpy as np
import torch

from . import _call, _lib
from .engine import pack_state_dict


@lru_cache(maxsize=None)
def layers():
    """name -> (kernel, cin, cout) of the graph's convolutions, in launch order, read from the library's own table
    (gs_detector_layer_info; csrc/detect_plan.h); weights are [k,k,cin,cout] (TF layout), biases [cout].  Loads the library on
    first use (no device needed), not on import."""
    lib = _lib.load()
    name, v = ctypes.c_char_p(), [ctypes.c_int() for _ in range(6)]
    rows = {}
    while lib.gs_detector_layer_info(len(rows), ctypes.byref(name), *[ctypes.byref(x) for x in v]):
        rows[name.value.decode()] = (v[0].value, v[1].value, v[2].value)
    return rows


def plan(n, h, w):
    """gs_detector_plan: what a forward of n windows of h x w runs (feature size, workspace bytes, per-layer shapes and kernels)"""
    p = _lib.DetectorPlan()
    _lib.check(_lib.load().gs_detector_plan(n, h, w, ctypes.byref(p)))
    return p


def synthetic_weights(seed=0):
    """Seeded random weights of the right shapes: He-normal for the ReLU layers, small heads (as detection heads are
    initialised), so activations stay O(1) through the stack and box deltas stay moderate."""
    rng = np.random.default_rng(seed)
    sd = {}
    for name, (k, cin, cout) in layers().items():
        head = name in ("rpn.head", "head.fc")
        std = 0.05 if head else float(np.sqrt(2.0 / (k * k * cin)))
        w = rng.standard_normal((k, k, cin, cout)).astype(np.float32) * np.float32(std)
        if name == "backbone.c1":
            w[:, :, 12:, :] = 0.0          # the four padding channels of the space-to-depth input carry no weight
        sd[name + ".weight"] = w
        sd[name + ".bias"] = (rng.standard_normal(cout) * (0.5 if head else 0.05)).astype(np.float32)
    return sd


# ---- include/glomseg_detector_steps.h: one kernel of the forward on the caller's buffers.  These exist for the tests
# (tests/test_detector_steps.py); nothing in the product calls them.
def step_names():
    """the steps gs_detector_step accepts (gs_detector_step_name), in the header's order"""
    lib, names = _lib.load(), []
    while lib.gs_detector_step_name(len(names)) is not None:
        names.append(lib.gs_detector_step_name(len(names)).decode())
    return names


def step(name, inputs, outputs, handle=None, stream=None, **sizes):
    """gs_detector_step: `inputs` / `outputs` are device addresses (up to three each) in the order of the header's table, `sizes`
    the fields of gs_detector_step_args the step reads (n, h, w, c, k, stride, pad, layer, count, crop, win_h, win_w)"""
    a = _lib.DetectorStepArgs()
    for i, p in enumerate(inputs):
        a.inp[i] = p
    for i, p in enumerate(outputs):
        a.out[i] = p
    for key, v in sizes.items():
        if key not in ("n", "h", "w", "c", "k", "stride", "pad", "layer", "count", "crop", "win_h", "win_w"):
            raise TypeError("gs_detector_step_args has no field %r" % key)
        setattr(a, key, v)
    _lib.check(_lib.load().gs_detector_step(handle, name.encode(), ctypes.byref(a), stream))


def pack4(weight):
    """gs_conv2d_nhwc_pack4 (host): float32 [kh,kw,cin,cout] -> the packed layout, as a flat float32 array"""
    weight = np.ascontiguousarray(weight, dtype=np.float32)
    kh, kw, cin, cout = weight.shape
    out = np.empty(weight.size, dtype=np.float32)
    _lib.check(_lib.load().gs_conv2d_nhwc_pack4(weight.ctypes.data_as(ctypes.c_void_p), kh, kw, cin, cout, out.ctypes.data_as(ctypes.c_void_p)))
    return out


def conv2d_nhwc_packed(inp, n, h, w, cin, packed_weight, kh, kw, cout, bias, stride, pad, relu, out, stream=None):
    """gs_conv2d_nhwc_packed: device addresses in, sizes as gs_conv2d_nhwc takes them; `bias` may be None"""
    _lib.check(_lib.load().gs_conv2d_nhwc_packed(inp, n, h, w, cin, packed_weight, kh, kw, cout, bias, stride, pad, int(relu), out, stream))


class FrcnnDetector:
    """One detector on one GPU.  Callable with the ``detect_box`` contract: uint8 RGB [N,H,W,3] (numpy or a GPU tensor)
    -> (boxes [N,D,4] normalised [ymin,xmin,ymax,xmax], scores [N,D] descending, classes [N,D], num [N]) as numpy."""

    def __init__(self, weights, device=None, rpn_nms_iou=0.7, det_nms_iou=0.6, score_threshold=0.0):
        if not torch.cuda.is_available():
            raise RuntimeError("FrcnnDetector needs a HIP device; there is no CPU path in this build")
        self.lib = _lib.load()
        self.device = torch.device("cuda", torch.cuda.current_device() if device is None else torch.device(device).index or 0)
        blob, table = pack_state_dict(weights)
        h = ctypes.c_void_p()
        with torch.cuda.device(self.device):
            _lib.check(self.lib.gs_detector_create(blob.ctypes.data_as(ctypes.c_void_p), table, len(table), ctypes.byref(h)))
            self.handle = h
            _lib.check(self.lib.gs_detector_set_thresholds(h, rpn_nms_iou, det_nms_iou, score_threshold))
        self.max_det = self.lib.gs_detector_max_detections()

    def close(self):
        if getattr(self, "handle", None):
            with torch.cuda.device(self.device):
                self.lib.gs_detector_destroy(self.handle)
            self.handle = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def forward_device(self, images, taps=False):
        """images: uint8 [N,H,W,3] GPU tensor -> dict of GPU tensors (boxes, scores, classes, num [+ debug taps])."""
        if images.dtype != torch.uint8 or images.dim() != 4 or images.shape[3] != 3 or not images.is_cuda:
            raise ValueError("expected a uint8 [N,H,W,3] tensor on the GPU")
        images = images.contiguous()
        n, h, w, _ = images.shape
        dev = images.device
        d = self.max_det
        out = {"boxes": torch.empty((n, d, 4), dtype=torch.float32, device=dev), "scores": torch.empty((n, d), dtype=torch.float32, device=dev),
               "classes": torch.empty((n, d), dtype=torch.float32, device=dev), "num": torch.empty((n,), dtype=torch.float32, device=dev)}
        dbg = [None, None, None, None]
        if taps:
            p, rows, props = plan(n, h, w), layers(), self.lib.gs_detector_num_proposals()
            out["features"] = torch.empty((n, p.hf, p.wf, rows["backbone.c6"][2]), dtype=torch.float32, device=dev)
            out["rpn"] = torch.empty((n, p.hf, p.wf, rows["rpn.head"][2]), dtype=torch.float32, device=dev)
            out["proposals"] = torch.empty((n, props, 4), dtype=torch.float32, device=dev)
            out["head"] = torch.empty((n * props, rows["head.fc"][2]), dtype=torch.float32, device=dev)
            dbg = [out[k].data_ptr() for k in ("features", "rpn", "proposals", "head")]
        with torch.cuda.device(dev):
            _lib.check(self.lib.gs_detector_forward(
                self.handle, images.data_ptr(), n, h, w, out["boxes"].data_ptr(), out["scores"].data_ptr(), out["classes"].data_ptr(),
                out["num"].data_ptr(), dbg[0], dbg[1], dbg[2], dbg[3], _call.stream_ptr(dev)))
        return out

    def step(self, name, inputs, outputs, **sizes):
        """one step of the forward on the caller's device buffers, with this handle's weights (module-level `step`; tests)"""
        with torch.cuda.device(self.device):
            step(name, inputs, outputs, handle=self.handle,
                 stream=_call.stream_ptr(self.device), **sizes)

    def detect_host(self, windows, batch=16):
        """gs_detector_detect_host: a list of equal-size uint8 RGB [H,W,3] windows in host memory (numpy; pinned CPU tensors are
        DMA'd in place) -> (boxes [n,D,4], scores [n,D], classes [n,D], num [n]) numpy.  Uploads run one batch ahead of the
        forward on a stream of their own; pageable windows are staged into pinned memory by a few threads."""
        n = len(windows)
        ptrs, shapes, keep = _call.host_image_ptrs(windows, "window")      # keep: the converted windows, alive until the call returns
        h, w = shapes[0] if shapes else (None, None)
        for i, shape in enumerate(shapes):
            if shape != (h, w):
                raise ValueError("window %d: expected uint8 [H,W,3], every window of one size" % i)
        d = self.max_det
        boxes = np.empty((n, d, 4), dtype=np.float32)
        scores = np.empty((n, d), dtype=np.float32)
        classes = np.empty((n, d), dtype=np.float32)
        num = np.empty((n,), dtype=np.float32)
        torch.cuda.current_stream(self.device).synchronize()     # the pipeline runs on streams of its own
        with torch.cuda.device(self.device):
            _lib.check(self.lib.gs_detector_detect_host(self.handle, ptrs, n, h, w, int(batch), boxes.ctypes.data_as(ctypes.c_void_p),
                                                        scores.ctypes.data_as(ctypes.c_void_p), classes.ctypes.data_as(ctypes.c_void_p),
                                                        num.ctypes.data_as(ctypes.c_void_p)))
        return boxes, scores, classes, num

    def __call__(self, images):
        if not isinstance(images, torch.Tensor):
            images = torch.from_numpy(np.ascontiguousarray(images, dtype=np.uint8))
        out = self.forward_device(images.to(self.device))
        return (out["boxes"].cpu().numpy(), out["scores"].cpu().numpy(), out["classes"].cpu().numpy(), out["num"].cpu().numpy())
