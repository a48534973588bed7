"""The detector's kernels one step at a time, each against a float64 restatement of its definition, on inputs the test chooses.

tests/test_detector_forms.py holds the UNPACKED convolution instances, gs_roialign, gs_nms and the selection stages; the assembled
forward only ever feeds a glue kernel what the stage before produced (a max-pool that sees ReLU outputs cannot show a zero
padding, a decode that sees trained-size deltas never clamps).  Here, through include/glomseg_detector_steps.h -- the step entry
runs the launchers gs_detector_forward itself calls --:

* the packed-weight convolution instances (conv2d_nhwc_tiled_kernel<true>, conv2d_nhwc_wide_kernel<4,true>): every tiled / wide
  case of CONV_CASES through gs_conv2d_nhwc_pack4 + gs_conv2d_nhwc_packed, and the detector's own 11 rows through the `conv`
  step with a handle's weights: the former at the family bound CONV_TAU * max(1, max|ref64|), the latter (K up to 2304) at
  STEP_CONV_TAU, measured the same way on their shapes;
* preprocess, maxpool, objectness, rpn_decode, gather_proposals, crop_pool, avgpool, head_decode: exact where the definition is
  exact, otherwise inside a bound that is derived (preprocess, avgpool, the proposals' quotient) or measured as 4 x the error
  of the float32 restatement against float64 on the same inputs (OBJ_BOUND, DECODE_BOUND; margin 4 as CONV_TAU has it);
* CPU tests showing, for every bound, that the float32 restatement stays inside it and that the named wrong variants do not.

Every GPU output is pre-filled with NaN (ints: -99) with 64 sentinel elements beyond its end, which must survive.
References: tests/helpers/detector_steps_ref.py (imports nothing from the package); oracle/detector_oracle.py only as a second
witness of crop_pool.  NOT reference parity: the reference's detector is an external frozen graph.
"""
import ctypes
import os
from functools import lru_cache

import numpy as np
import pytest

from helpers import detector_steps_ref as ref
from oracle import detector_oracle as do
from test_detector_forms import (CONV_BY_NAME, CONV_CASES, CONV_TAU, DET_LAYER_ROWS, ConvCase, conv_bound, conv_data, conv_form,
                                 conv_ref64, conv_reference, roi_case)

F32 = np.float32
REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SENTINELS = 64
SENTINEL_F, SENTINEL_I, UNWRITTEN_I = 12345.0, -7, -99


@pytest.fixture(scope="module")
def torch_mod():
    import torch
    assert torch.cuda.is_available(), "the gpu-marked tests need a HIP device"
    return torch


class DevOut:
    """an output buffer of `shape` on the device: NaN (ints: -99) where the kernel must write, 64 sentinels beyond"""

    def __init__(self, torch, shape, integer=False):
        self.torch, self.shape, self.size, self.integer = torch, tuple(shape), int(np.prod(shape)), integer
        host = np.full(self.size + SENTINELS, UNWRITTEN_I if integer else np.nan, dtype=np.int32 if integer else F32)
        host[self.size:] = SENTINEL_I if integer else SENTINEL_F
        self.t = torch.from_numpy(host).cuda()
        self.ptr = self.t.data_ptr()

    def read(self, allow_nan=False):
        self.torch.cuda.synchronize()
        a = self.t.cpu().numpy()
        assert (a[self.size:] == (SENTINEL_I if self.integer else SENTINEL_F)).all(), "written beyond the output"
        a = a[:self.size].reshape(self.shape)
        if self.integer:
            assert not (a == UNWRITTEN_I).any(), "output elements left unwritten"
        elif not allow_nan:
            assert not np.isnan(a).any(), "output elements left unwritten (or NaN produced)"
        return a


def dev(torch, a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def run_step(name, inputs, outputs, handle=None, **sizes):
    from glomeruli_segmentation_amd import detector
    if handle is not None:
        handle.step(name, [t.data_ptr() for t in inputs], [o.ptr for o in outputs], **sizes)
    else:
        detector.step(name, [t.data_ptr() for t in inputs], [o.ptr for o in outputs], **sizes)


# ================================================================================================ the header and the entry
STEP_NAMES = ["preprocess", "maxpool", "conv", "objectness", "rpn_decode", "gather_proposals", "crop_pool", "avgpool", "head_decode"]


def test_the_header_and_the_binding():
    from helpers.header_binding import assert_declared_exported_prototyped
    from glomeruli_segmentation_amd import _lib, detector
    text = assert_declared_exported_prototyped("glomseg_detector_steps.h", _lib.DETECTOR_STEPS_PROTOTYPES,
                                               {"gs_conv2d_nhwc_pack4", "gs_conv2d_nhwc_packed", "gs_detector_step_name", "gs_detector_step"})
    assert detector.step_names() == STEP_NAMES
    for name in STEP_NAMES:
        assert '"%s"' % name in text, name
    # the struct of the binding is the header's, field for field
    import re
    body = re.search(r"typedef struct gs_detector_step_args \{(.*?)\} gs_detector_step_args;", re.sub(r"/\*.*?\*/", "", text, flags=re.S), flags=re.S).group(1)
    fields = [f for decl in body.split(";") for f in re.findall(r"(\w+)(?:\[\d+\])?\s*(?:,|$)", decl.strip())]
    assert fields == [{"inp": "in"}.get(n, n) for n, _ in _lib.DetectorStepArgs._fields_], fields
    assert ctypes.sizeof(_lib.DetectorStepArgs) == 6 * 8 + 8 + 9 * 4 + 2 * 4 + 4        # (padded to the pointers' alignment)


def test_every_step_has_a_gpu_test():
    """every step name the header's entry accepts has a gpu-marked test_step_<name>... in this file"""
    from glomeruli_segmentation_amd import detector
    names = detector.step_names()
    assert names == STEP_NAMES
    gpu_tests = [k for k, v in globals().items() if k.startswith("test_step_") and callable(v) and
                 any(m.name == "gpu" for m in getattr(v, "pytestmark", []))]
    for name in names:
        assert any(t.startswith("test_step_" + name) for t in gpu_tests), "step %r has no GPU test" % name


def test_step_entry_refuses_on_the_host():
    """bad arguments are GS_ERR_INVALID with a message, before anything is launched (no device here)"""
    from glomeruli_segmentation_amd import _lib, detector
    p = 4096            # (never dereferenced: every call below is refused)
    bad = [
        ("nosuchstep", dict(inputs=[p], outputs=[p], n=1, h=2, w=2), "no step named"),
        ("preprocess", dict(inputs=[], outputs=[p], n=1, h=2, w=2), "null pointer"),
        ("preprocess", dict(inputs=[p], outputs=[p], n=0, h=2, w=2), "must be positive"),
        ("maxpool", dict(inputs=[p], outputs=[p], n=1, h=4, w=4, c=6, k=3, stride=2, pad=1), "multiple of 4"),
        ("maxpool", dict(inputs=[p], outputs=[p], n=1, h=4, w=4, c=8, k=3, stride=2, pad=3), "pad < k"),
        ("maxpool", dict(inputs=[p], outputs=[p], n=1, h=1, w=4, c=8, k=3, stride=2, pad=0), "empty output"),
        ("maxpool", dict(inputs=[p], outputs=[p], n=1, h=4, w=4, c=8, k=3, stride=0, pad=1), "stride > 0"),
        ("conv", dict(inputs=[p], outputs=[p], n=1, h=4, w=4, layer=0), "null handle"),
        ("objectness", dict(inputs=[p], outputs=[], n=1, h=2, w=2), "null pointer"),
        ("rpn_decode", dict(inputs=[p, p], outputs=[p], n=1, h=2, w=2, count=0, win_h=32, win_w=32), "must be positive"),
        ("rpn_decode", dict(inputs=[p, p], outputs=[p], n=1, h=2, w=2, count=4, win_h=0, win_w=32), "must be positive"),
        ("rpn_decode", dict(inputs=[p], outputs=[p], n=1, h=2, w=2, count=4, win_h=32, win_w=32), "null pointer"),
        ("gather_proposals", dict(inputs=[p, p], outputs=[p, p], n=1, count=4, win_h=32, win_w=32), "null pointer"),
        ("crop_pool", dict(inputs=[p, p, p], outputs=[p], n=1, h=2, w=2, c=6, count=3, crop=14), "multiple of 4"),
        ("crop_pool", dict(inputs=[p, p, p], outputs=[p], n=1, h=2, w=2, c=8, count=3, crop=7), "crop must be even"),
        ("crop_pool", dict(inputs=[p, p, p], outputs=[p], n=1, h=2, w=2, c=8, count=0, crop=14), "count must be positive"),
        ("avgpool", dict(inputs=[p], outputs=[p], n=1, h=0, w=2, c=8), "must be positive"),
        ("head_decode", dict(inputs=[p, p, p], outputs=[p, p], count=0, win_h=32, win_w=32), "must be positive"),
        ("head_decode", dict(inputs=[p, p], outputs=[p, p], count=5, win_h=32, win_w=32), "null pointer"),
    ]
    for name, kw, message in bad:
        with pytest.raises(_lib.GlomsegError, match=message) as e:
            detector.step(name, **kw)
        assert e.value.status == 1, (name, kw)
    with pytest.raises(TypeError):
        detector.step("avgpool", [p], [p], n=1, hw=3)
    # the packed convolution shares gs_conv2d_nhwc's argument checks and the packed kernels' refusal
    with pytest.raises(_lib.GlomsegError, match="gs_conv2d_nhwc_packed: null pointer") as e:
        detector.conv2d_nhwc_packed(None, 1, 4, 4, 8, p, 3, 3, 8, None, 1, 1, 1, p)
    assert e.value.status == 1
    with pytest.raises(_lib.GlomsegError, match="conv2d_nhwc_packed4: shape not supported by the packed-weight kernel") as e:
        detector.conv2d_nhwc_packed(p, 1, 4, 4, 12, p, 3, 3, 8, None, 1, 1, 1, p)
    assert e.value.status == 4


def test_conv_form_32bit_limit_leaves_room_for_the_no_data_offset():
    """the 64 x 64 kernels read "no data" at byte offset 0x7ffffff0, so a tensor they take has at most that many bytes:
    233 x 1103 x 2089 x 1 floats are 2^31 - 4 bytes -- generic; one row less still runs the small-cin kernel"""
    assert 233 * 1103 * 2089 == 2 ** 29 - 1
    assert conv_form(233, 1103, 2089, 1, 3, 3, 8, 1, 1) == "generic"
    assert conv_form(233, 1102, 2089, 1, 3, 3, 8, 1, 1) == "smallcin"
    # (with cin % 8 == 0 a tensor's bytes are a multiple of 32 and never fall between the two limits: only the small-cin kernel
    # could meet the case, and the refusals and known answers of test_detector_forms are what they were)


# ================================================================================================ packed convolutions
PACKED_CASES = [c.name for c in CONV_CASES if c.form in ("tiled", "wide")]


def pack4_ref(w):
    K, cout = w.shape[0] * w.shape[1] * w.shape[2], w.shape[3]
    return np.ascontiguousarray(w.reshape(K // 4, 4, cout).transpose(0, 2, 1))


def test_pack4_is_the_documented_layout():
    from glomeruli_segmentation_amd import _lib, detector
    assert PACKED_CASES == ["T%d" % i for i in range(1, 8)] + ["W%d" % i for i in range(1, 8)]
    rng = np.random.default_rng(3)
    for shape in ((1, 1, 8, 6), (3, 3, 64, 72), (2, 3, 24, 33)):
        w = rng.standard_normal(shape).astype(F32)
        got = detector.pack4(w)
        assert got.dtype == F32 and np.array_equal(got, pack4_ref(w).reshape(-1)), shape
    for cin in (4, 12, 7):
        with pytest.raises(_lib.GlomsegError, match="not supported by the packed-weight kernel") as e:
            detector.pack4(np.zeros((3, 3, cin, 8), F32))
        assert e.value.status == 4          # GS_ERR_UNSUPPORTED


def test_packed_comparison_rejects_a_transposed_packer():
    """a packer with the roles of k / 4 and k & 3 swapped (k = r * (K/4) + q instead of 4 q + r), read back the right way and
    convolved in float64, misses the bound on every packed case"""
    import torch
    for name in PACKED_CASES:
        c = CONV_BY_NAME[name]
        x, w, b = conv_data(name)
        K = c.kh * c.kw * c.cin
        wrong = np.ascontiguousarray(w.reshape(4, K // 4, c.cout).transpose(1, 2, 0))        # [K/4][cout][4], wrongly filled
        seen = np.ascontiguousarray(wrong.transpose(0, 2, 1)).reshape(w.shape)               # what the kernel's walk reads
        assert np.array_equal(np.ascontiguousarray(pack4_ref(w).transpose(0, 2, 1)).reshape(w.shape), w)
        bad = conv_reference(c, x, seen, b, torch.float64)
        assert np.abs(bad - conv_ref64(name)).max() > conv_bound(conv_ref64(name)), name


@pytest.mark.gpu
@pytest.mark.parametrize("name", PACKED_CASES)
def test_packed_conv_against_float64(torch_mod, name):
    torch = torch_mod
    from glomeruli_segmentation_amd import detector
    c = CONV_BY_NAME[name]
    assert conv_form(c.n, c.h, c.w, c.cin, c.kh, c.kw, c.cout, c.stride, c.pad, packed=True) == c.form
    x, w, b = conv_data(name)
    want = conv_ref64(name)
    xd, wd, bd = dev(torch, x), dev(torch, detector.pack4(w)), dev(torch, b)
    out = DevOut(torch, want.shape)
    detector.conv2d_nhwc_packed(xd.data_ptr(), c.n, c.h, c.w, c.cin, wd.data_ptr(), c.kh, c.kw, c.cout, bd.data_ptr() if c.bias else None,
                                c.stride, c.pad, c.relu, out.ptr)
    got = out.read().astype(np.float64)
    err, bound = float(np.abs(got - want).max()), conv_bound(want)
    print("packed conv %s (%s): error / bound = %.3f (error %.3g relative to max(1, max|ref|))" % (
        name, c.form, err / bound, err / max(1.0, float(np.abs(want).max()))))
    assert err <= bound, (name, c.form, err, bound)


# ---- the detector's own rows through the `conv` step: (row, images, h, w, the packed form the shape must plan)
# The bound.  CONV_TAU (3.52e-6, relative to max(1, max|ref64|)) is four times the worst error of torch's fp32 CPU convolution over
# CONV_CASES, whose longest K is 864.  The detector's rows reach K = 2304, and on these shapes and this data that yardstick is not
# a quarter of CONV_TAU (8.8e-7): torch's fp32 CPU convolution errs by up to 2.01e-6 (backbone.c6 on 2x3x3; 1.7e-6 on rpn.conv,
# 1.3e-6 on c6 10x12), and even with oneDNN switched off (5.9e-7) a float32 accumulator that walks K in order, two products a
# step as the matrix instruction does, errs by 1.42e-6 on that shape.  So these cases take their own bound, made the way
# CONV_TAU was: 4 x the measured worst, 2.01e-6 written up to 2.1e-6.  test_step_conv_bound_holds_for_the_reference re-measures
# it; the GPU test prints its error against both bounds.
STEP_CONV_TAU = 4 * 2.1e-6


def step_conv_bound(ref64):
    return STEP_CONV_TAU * max(1.0, float(np.abs(ref64).max()))


STEP_CONV_CASES = [
    (0, 2, 17, 24, "tiled"), (1, 2, 9, 12, "wide"), (1, 1, 7, 9, "tiled"), (2, 2, 9, 12, "tiled"), (2, 1, 17, 16, "wide"),
    (3, 2, 5, 6, "tiled"), (3, 1, 8, 8, "wide"), (4, 2, 5, 6, "tiled"), (4, 1, 17, 16, "wide"), (5, 2, 3, 3, "tiled"),
    (5, 1, 10, 12, "wide"), (6, 1, 10, 12, "wide"), (6, 1, 9, 7, "tiled"), (7, 1, 10, 12, "wide"), (7, 2, 3, 3, "tiled"),
    (8, 5, 7, 7, "tiled"), (9, 5, 7, 7, "tiled"), (10, 37, 1, 1, "tiled"),
]
STEP_CONV_IDS = ["%s-%dx%dx%d" % (DET_LAYER_ROWS[i][0], n, h, w) for i, n, h, w, _ in STEP_CONV_CASES]


@lru_cache(maxsize=None)
def step_conv_weights():
    """the handle's tensors: row i seeded 2000 + i, weights standard_normal * 0.2 then biases standard_normal (conv_data's recipe)"""
    sd = {}
    for i, (name, k, cin, cout, stride, pad, relu) in enumerate(DET_LAYER_ROWS):
        rng = np.random.default_rng(2000 + i)
        sd[name + ".weight"] = (rng.standard_normal((k, k, cin, cout)) * 0.2).astype(F32)
        sd[name + ".bias"] = rng.standard_normal(cout).astype(F32)
    return sd


@lru_cache(maxsize=None)
def step_conv_case(ci):
    """(ConvCase, x, w, b, ref64) of STEP_CONV_CASES[ci]; the input is standard_normal, seeded by the row and the shape"""
    import torch
    i, n, h, w_, form = STEP_CONV_CASES[ci]
    name, k, cin, cout, stride, pad, relu = DET_LAYER_ROWS[i]
    c = ConvCase(name, form, n, h, w_, cin, k, k, cout, stride, pad, True, bool(relu), frozenset())
    x = np.random.default_rng([2000 + i, n, h, w_]).standard_normal((n, h, w_, cin)).astype(F32)
    sd = step_conv_weights()
    w, b = sd[name + ".weight"], sd[name + ".bias"]
    return c, x, w, b, conv_reference(c, x, w, b, torch.float64)


def test_step_conv_cases_plan_their_forms():
    assert [r[0] for r in DET_LAYER_ROWS] == ["backbone.c%d" % i for i in range(1, 7)] + ["rpn.conv", "rpn.head", "head.h1", "head.h2", "head.fc"]
    assert {i for i, *_ in STEP_CONV_CASES} == set(range(11))
    for (i, n, h, w, form) in STEP_CONV_CASES:
        name, k, cin, cout, stride, pad, relu = DET_LAYER_ROWS[i]
        assert conv_form(n, h, w, cin, k, k, cout, stride, pad, packed=True) == form, (name, n, h, w)
        ho, wo = (h + 2 * pad - k) // stride + 1, (w + 2 * pad - k) // stride + 1
        assert (ho * wo >= 64) == (form == "wide") or cin % 32, (name, n, h, w)
        assert n * h * w * cin * 4 <= 400000 and n * ho * wo * cout * 4 <= 400000
    assert STEP_CONV_CASES[12][1:4] == (1, 9, 7)            # rpn.conv on 63 pixels: the tiled side of the threshold at cin 256


def test_step_conv_bound_holds_for_the_reference():
    """torch's fp32 CPU convolution against float64 on every shape of STEP_CONV_CASES, relative to max(1, max|ref64|): at most a
    quarter of STEP_CONV_TAU -- the margin the family bound CONV_TAU was given where it was measured (test_detector_forms); it
    is NOT within a quarter of CONV_TAU (comment at STEP_CONV_TAU), which is why these cases have a bound of their own"""
    import torch
    worst = {}
    for ci, cid in enumerate(STEP_CONV_IDS):
        c, x, w, b, want = step_conv_case(ci)
        err = float(np.abs(conv_reference(c, x, w, b, torch.float32).astype(np.float64) - want).max())
        worst[cid] = err / max(1.0, float(np.abs(want).max()))
        print("conv step %s: torch fp32 CPU vs float64 %.3g relative (%.3f of STEP_CONV_TAU, %.3f of CONV_TAU)" % (
            cid, worst[cid], worst[cid] / STEP_CONV_TAU, worst[cid] / CONV_TAU))
        # ... and the bound sees one dropped 8-channel chunk of the last tap
        w_bad = w.copy()
        w_bad[-1, -1, -8:] = 0
        assert np.abs(conv_reference(c, x, w_bad, b, torch.float64) - want).max() > step_conv_bound(want), cid
    top = max(worst, key=worst.get)
    print("conv step: worst %.3g on %s; x4 = %.3g; STEP_CONV_TAU = %.3g; CONV_TAU / 4 = %.3g" % (
        worst[top], top, 4 * worst[top], STEP_CONV_TAU, CONV_TAU / 4))
    assert worst[top] <= STEP_CONV_TAU / 4, (top, worst[top])
    assert STEP_CONV_TAU <= 2e-4          # 24 times tighter than what check_detector_stages holds the same kernels to, and per layer


@pytest.fixture(scope="module")
def step_detector(torch_mod):
    from glomeruli_segmentation_amd.detector import FrcnnDetector
    det = FrcnnDetector(step_conv_weights())
    yield det
    det.close()


@pytest.mark.gpu
@pytest.mark.parametrize("ci", range(len(STEP_CONV_CASES)), ids=STEP_CONV_IDS)
def test_step_conv_against_float64(torch_mod, step_detector, ci):
    torch = torch_mod
    c, x, w, b, want = step_conv_case(ci)
    assert conv_form(c.n, c.h, c.w, c.cin, c.kh, c.kw, c.cout, c.stride, c.pad, packed=True) == c.form
    xd = dev(torch, x)
    out = DevOut(torch, want.shape)
    run_step("conv", [xd], [out], handle=step_detector, layer=STEP_CONV_CASES[ci][0], n=c.n, h=c.h, w=c.w)
    got = out.read().astype(np.float64)
    err, bound = float(np.abs(got - want).max()), step_conv_bound(want)
    print("conv step %s (%s): error / bound = %.3f (error %.3g relative to max(1, max|ref|) = %.3f of CONV_TAU)" % (
        STEP_CONV_IDS[ci], c.form, err / bound, err / max(1.0, float(np.abs(want).max())), err / conv_bound(want)))
    assert err <= bound, (STEP_CONV_IDS[ci], err, bound)


# ================================================================================================ preprocess
PRE_SIZES = [(1, 1, 1), (2, 3, 5), (2, 33, 47), (1, 32, 32), (3, 50, 37)]
# |fp32 - float64| of 2 x / 255 - 1: the constant's rounding (half an ulp of 2/255 = 2^-31) times x <= 255 is < 2^-23, the
# product (<= 2) rounds by <= 2^-24, the difference (in [-1,1]) by <= 2^-25; fused, the last two are one rounding
PRE_BOUND = 2.0 ** -22


@lru_cache(maxsize=None)
def pre_image(n, H, W):
    """bytes: a seeded permutation of 0..255 repeated to the size (all 256 values wherever the image has room for them)"""
    size = n * H * W * 3
    rng = np.random.default_rng(300 + size)
    vals = np.concatenate([rng.permutation(256) for _ in range(size // 256 + 1)])[:size]
    img = vals.astype(np.uint8).reshape(n, H, W, 3)
    assert size < 256 or len(np.unique(img)) == 256
    return img


def check_preprocess(got, img):
    """the exact part: which pixel every channel holds (2 x / 255 - 1 is injective on bytes), and the zeros, bit for bit"""
    n, H, W, _ = img.shape
    h2, w2 = (H + 1) // 2, (W + 1) // 2
    assert got.shape == (n, h2, w2, 16) and got.dtype == F32
    bits = got.view(np.uint32)
    assert not bits[..., 12:].any(), "channels 12..15 are not +0.0"
    for dy in range(2):
        for dx in range(2):
            q = (dy * 2 + dx) * 3
            src = img[:, dy::2, dx::2]
            hy, wx = src.shape[1], src.shape[2]
            back = np.rint((got[:, :hy, :wx, q:q + 3].astype(np.float64) + 1.0) * 127.5)
            assert np.array_equal(back, src), (dy, dx)
            assert not bits[:, hy:, :, q:q + 3].any() and not bits[:, :, wx:, q:q + 3].any(), "beyond an odd edge is not +0.0"


def test_preprocess_bound_holds_and_discriminates():
    for (n, H, W) in PRE_SIZES:
        img = pre_image(n, H, W)
        want = ref.preprocess(img)
        for fused in (False, True):
            got = ref.preprocess(img, F32, fused=fused)
            check_preprocess(got, img)
            assert np.abs(got.astype(np.float64) - want).max() <= PRE_BOUND
        if H * W > 1:
            assert np.abs(ref.preprocess(img, bgr=True) - want).max() > PRE_BOUND
            with pytest.raises(AssertionError):
                check_preprocess(ref.preprocess(img, F32, bgr=True), img)
        if H % 2 or W % 2:
            bad = ref.preprocess(img, F32, edge=-1.0)
            assert np.abs(bad.astype(np.float64) - want).max() > PRE_BOUND
            with pytest.raises(AssertionError, match="odd edge"):
                check_preprocess(bad, img)
    # all 256 byte values, both roundings: the worst error, for the record
    x = np.arange(256, dtype=np.uint8).reshape(1, 16, 16, 1).repeat(3, axis=3)
    worst = max(np.abs(ref.preprocess(x, F32, fused=f).astype(np.float64) - ref.preprocess(x)).max() for f in (False, True))
    print("preprocess: worst fp32 error %.3g = %.3f of 2^-22" % (worst, worst / PRE_BOUND))


@pytest.mark.gpu
@pytest.mark.parametrize("size", PRE_SIZES, ids=lambda s: "%dx%dx%d" % s)
def test_step_preprocess(torch_mod, size):
    torch = torch_mod
    n, H, W = size
    img = pre_image(n, H, W)
    want = ref.preprocess(img)
    out = DevOut(torch, want.shape)
    run_step("preprocess", [dev(torch, img)], [out], n=n, h=H, w=W)
    got = out.read()
    check_preprocess(got, img)
    err = float(np.abs(got.astype(np.float64) - want).max())
    print("preprocess %dx%dx%d: error / bound = %.3f" % (n, H, W, err / PRE_BOUND))
    assert err <= PRE_BOUND


# ================================================================================================ maxpool
#            n   h   w    c  k  s pad  input
POOL_CASES = [(2, 17, 24, 64, 3, 2, 1, "normal"), (1, 16, 16, 64, 3, 2, 1, "negative"), (3, 25, 19, 64, 3, 2, 1, "with_inf"),
              (1, 1, 1, 64, 3, 2, 1, "negative"), (1, 2, 3, 4, 3, 2, 1, "normal"), (1, 9, 7, 128, 2, 2, 0, "normal")]


@lru_cache(maxsize=None)
def pool_input(ci):
    n, h, w, c, k, s, pad, kind = POOL_CASES[ci]
    rng = np.random.default_rng(400 + ci)
    x = rng.standard_normal((n, h, w, c)).astype(F32)
    if kind == "negative":
        x = -(np.abs(x) + F32(0.5))
    if kind == "with_inf":
        x[rng.random(x.shape) < 0.1] = -np.inf
        x[0, 4:9, 6:11] = -np.inf            # whole windows of -inf: the maximum is -inf
        x[1, :3, :3, ::2] = np.inf
    return x


def pool_threads(ci):
    n, h, w, c, k, s, pad, kind = POOL_CASES[ci]
    return n * ((h + 2 * pad - k) // s + 1) * ((w + 2 * pad - k) // s + 1) * (c // 4)


def test_maxpool_cases_and_zero_padding_variant():
    totals = [pool_threads(ci) for ci in range(len(POOL_CASES))]
    assert any(t < 256 for t in totals) and any(t > 256 and t % 256 for t in totals), totals
    for ci, (n, h, w, c, k, s, pad, kind) in enumerate(POOL_CASES):
        x = pool_input(ci)
        want = ref.maxpool(x, k, s, pad)
        assert not np.isnan(want).any() and x.nbytes <= 400000
        if kind == "negative":               # a zero padding wins on the border, and only there
            zero = ref.maxpool(x, k, s, pad, pad_value=0.0)
            assert (x < 0).all() and (zero != want).any() and (zero[:, 0] == 0).all()
        if kind == "with_inf":
            assert np.isneginf(want).any() and np.isposinf(want).any() and np.isfinite(want).any()


@pytest.mark.gpu
@pytest.mark.parametrize("ci", range(len(POOL_CASES)), ids=["%dx%dx%dx%d-k%ds%dp%d-%s" % c for c in POOL_CASES])
def test_step_maxpool(torch_mod, ci):
    torch = torch_mod
    n, h, w, c, k, s, pad, kind = POOL_CASES[ci]
    x = pool_input(ci)
    want = ref.maxpool(x, k, s, pad)
    out = DevOut(torch, want.shape)
    run_step("maxpool", [dev(torch, x)], [out], n=n, h=h, w=w, c=c, k=k, stride=s, pad=pad)
    got = out.read()
    assert np.array_equal(got.astype(np.float64), want), np.argwhere(got.astype(np.float64) != want)[:5]


# ================================================================================================ objectness
# |score - float64|, absolute (scores are compared with absolute thresholds downstream): 4 x the worst error of the fp32 numpy
# restatement on objectness_case()'s inputs, measured 8.22e-08 (test_objectness_bound_holds_and_discriminates prints it)
OBJ_BOUND = 4 * 8.22e-08
OBJ_N, OBJ_HF, OBJ_WF = 2, 3, 5


@lru_cache(maxsize=None)
def objectness_case():
    """rpn [2,15,72] and, per anchor, what its logit difference is: 0 'half', +-200 'zero' / 'one', else within [-30, 30]"""
    rng = np.random.default_rng(500)
    n_anchor = OBJ_N * OBJ_HF * OBJ_WF * ref.A
    rpn = rng.standard_normal((OBJ_N, OBJ_HF * OBJ_WF, 6 * ref.A)).astype(F32)
    d = rng.uniform(-30, 30, n_anchor)
    mid = rng.uniform(-5, 5, n_anchor)
    bg, fg = (mid + d / 2).astype(F32), (mid - d / 2).astype(F32)
    kind = np.array(["rest"] * n_anchor, dtype=object)
    for j, what in ((0, "half"), (1, "zero"), (2, "one")):
        sel = np.arange(j, n_anchor, 9)
        kind[sel] = what
        bg[sel], fg[sel] = {"half": (mid[sel].astype(F32), mid[sel].astype(F32)), "zero": (100.0, -100.0), "one": (-100.0, 100.0)}[what]
    rpn[..., :2 * ref.A] = np.stack([bg, fg], axis=1).reshape(OBJ_N, OBJ_HF * OBJ_WF, 2 * ref.A)     # anchor-major (bg, fg) pairs
    assert np.abs(bg[kind == "rest"] - fg[kind == "rest"]).max() <= 30.001
    return rpn, kind


def check_scores(got, want64, kind, label):
    """exact where the definition is exact; the rest inside OBJ_BOUND -> error / bound"""
    assert (got[kind == "half"] == F32(0.5)).all() and (got[kind == "zero"] == 0).all() and (got[kind == "one"] == 1).all(), label
    rest = kind == "rest"
    assert (got[rest] > 2.0 ** -126).all()              # nothing in the subnormal range (nor below)
    return float(np.abs(got[rest].astype(np.float64) - want64[rest]).max()) / OBJ_BOUND


def test_objectness_bound_holds_and_discriminates():
    rpn, kind = objectness_case()
    assert rpn.shape[0] * rpn.shape[1] * ref.A == 360 and 360 % 256
    want = ref.objectness(rpn).reshape(-1)
    got = ref.objectness(rpn, F32).reshape(-1)
    ratio = check_scores(got, want, kind, "fp32 restatement")
    print("objectness: fp32 restatement worst error %.3g; x4 = %.3g; OBJ_BOUND = %.3g" % (ratio * OBJ_BOUND, 4 * ratio * OBJ_BOUND, OBJ_BOUND))
    assert ratio <= 0.25 + 1e-3                          # the constant is 4 x this measurement
    swapped = ref.objectness(rpn, F32, swap=True).reshape(-1)
    assert float(np.abs(swapped[kind == "rest"].astype(np.float64) - want[kind == "rest"]).max()) > OBJ_BOUND
    with pytest.raises(AssertionError):
        check_scores(swapped, want, kind, "swapped")


@pytest.mark.gpu
def test_step_objectness(torch_mod):
    torch = torch_mod
    rpn, kind = objectness_case()
    want = ref.objectness(rpn).reshape(-1)
    out = DevOut(torch, want.shape)
    run_step("objectness", [dev(torch, rpn)], [out], n=OBJ_N, h=OBJ_HF, w=OBJ_WF)
    ratio = check_scores(out.read(), want, kind, "gpu")
    print("objectness: error / bound = %.3f" % ratio)
    assert ratio <= 1.0


# ================================================================================================ rpn_decode
# |corner - float64| in pixels: 4 x the worst error of the fp32 numpy restatement over rpn_decode_case()'s and head_case()'s
# comparable rows, measured 3.02e-05 on the former and 2.05e-05 on the latter (test_decode_bound_holds_and_discriminates prints both)
DECODE_BOUND = 4 * 3.02e-05
DEC_H, DEC_W, DEC_HF, DEC_WF, DEC_N, DEC_K = 160, 192, 10, 12, 2, 64
DELTA_KINDS = ["zero", "size_clamped", "zero_size", "far_down", "far_up", "far_right", "far_left", "nan", "random", "random", "random", "random"]


def make_deltas(rng, kind, j):
    d = (rng.standard_normal(4) * 2).astype(F32)
    if kind == "zero":
        d[:] = 0
    elif kind == "size_clamped":             # above LIM / 0.2 = 20.7
        d[2], d[3] = 25.0, 1000.0
    elif kind == "zero_size":                # exp(-200) = 0 in fp32
        d[2] = -1000.0
    elif kind.startswith("far_"):
        d[{"far_down": 0, "far_up": 0, "far_right": 1, "far_left": 1}[kind]] = 1e4 if kind in ("far_down", "far_right") else -1e4
    elif kind == "nan":
        d[[[0], [2], [0, 1, 2, 3]][j % 3]] = np.nan
    return d


@lru_cache(maxsize=None)
def rpn_decode_case():
    """(rpn [2,120,72], sel int32 [2,64], kinds [2,64]): per image four -1 entries (two of them the tail), anchor 0, the last
    anchor of the last cell, the 12 anchors of interior cell (5, 6), distinct random anchors; deltas by kind, round robin"""
    rng = np.random.default_rng(600)
    cells = DEC_HF * DEC_WF
    rpn = rng.standard_normal((DEC_N, cells, 6 * ref.A)).astype(F32)
    sel = np.zeros((DEC_N, DEC_K), dtype=np.int32)
    kinds = np.empty((DEC_N, DEC_K), dtype=object)
    for i in range(DEC_N):
        fixed = [0, cells * ref.A - 1] + [(5 * DEC_WF + 6) * ref.A + a for a in range(ref.A)]
        others = rng.permutation(np.setdiff1d(np.arange(cells * ref.A), fixed))[:DEC_K - 4 - len(fixed)]
        body = rng.permutation(np.concatenate([fixed, others, [-1, -1]]))
        sel[i] = np.concatenate([body, [-1, -1]])
        deltas = rpn[i][:, 2 * ref.A:].reshape(-1, 4)     # (a copy) by anchor index
        for j, ai in enumerate(sel[i]):
            kinds[i, j] = "none" if ai < 0 else DELTA_KINDS[(j + 5 * i) % len(DELTA_KINDS)]
            if ai >= 0:
                deltas[ai] = make_deltas(rng, kinds[i, j], j)
        rpn[i][:, 2 * ref.A:] = deltas.reshape(cells, 4 * ref.A)
    assert len(set(sel[0][sel[0] >= 0])) == DEC_K - 4 and set(DELTA_KINDS) <= set(kinds[0]) | set(kinds[1])
    return rpn, sel, kinds


def check_boxes(got, want64, kinds, H, W, label):
    """exact: everything finite, inside [0,H] x [0,W], corners ordered; 'none' rows zero; a zero-size box has equal corners on
    its axis; NaN deltas give finite boxes (their values are not compared) -> worst error / DECODE_BOUND of the other rows"""
    got = got.reshape(-1, 4)
    want64 = want64.reshape(-1, 4)
    kinds = kinds.reshape(-1)
    assert np.isfinite(got).all(), label
    assert (got >= 0).all() and (got[:, [0, 2]] <= H).all() and (got[:, [1, 3]] <= W).all(), label
    assert (got[:, 0] <= got[:, 2]).all() and (got[:, 1] <= got[:, 3]).all(), label
    assert not got[kinds == "none"].any(), label
    assert (got[kinds == "zero_size"][:, 0] == got[kinds == "zero_size"][:, 2]).all(), label
    compared = (kinds != "nan") & (kinds != "none")
    return float(np.abs(got[compared].astype(np.float64) - want64[compared]).max()) / DECODE_BOUND


def test_decode_bound_holds_and_discriminates():
    rpn, sel, kinds = rpn_decode_case()
    want = ref.rpn_decode(rpn, sel, DEC_HF, DEC_WF, DEC_H, DEC_W)
    r1 = check_boxes(ref.rpn_decode(rpn, sel, DEC_HF, DEC_WF, DEC_H, DEC_W, F32), want, kinds, DEC_H, DEC_W, "fp32 restatement")
    # the inputs reach what they are for: clipped on every side, clamped sizes fill the window, interior boxes exist
    flat, k = want.reshape(-1, 4), kinds.reshape(-1)
    assert (flat[k == "far_down"][:, 0] == DEC_H).all() and (flat[k == "far_up"][:, 2] == 0).all()
    assert (flat[k == "far_right"][:, 1] == DEC_W).all() and (flat[k == "far_left"][:, 3] == 0).all()
    inner = (flat > 0).all(1) & (flat[:, [0, 2]] < DEC_H).all(1) & (flat[:, [1, 3]] < DEC_W).all(1)
    assert inner.sum() >= 5, inner.sum()
    head, prop, keep, hk, bk = head_case(600)
    r2 = check_boxes(ref.head_decode(head, prop, keep, DEC_H, DEC_W, F32)[1], ref.head_decode(head, prop, keep, DEC_H, DEC_W)[1], bk, DEC_H, DEC_W,
                     "fp32 restatement, head")
    print("decode: fp32 restatement worst error %.3g px (rpn_decode inputs), %.3g px (head_decode inputs); x4 of the larger = %.3g; "
          "DECODE_BOUND = %.3g" % (r1 * DECODE_BOUND, r2 * DECODE_BOUND, 4 * max(r1, r2) * DECODE_BOUND, DECODE_BOUND))
    assert max(r1, r2) <= 0.25 + 1e-3                   # the constant is 4 x this measurement
    for label, wrong in (("cell % hf", dict(cell_mod=DEC_HF)), ("scales swapped", dict(centre_scale=0.2, size_scale=0.1)),
                         ("clip to H-1", dict(clip_to=(DEC_H - 1, DEC_W - 1)))):
        bad = ref.rpn_decode(rpn, sel, DEC_HF, DEC_WF, DEC_H, DEC_W, F32, **wrong).reshape(-1, 4)
        cmp = (k != "nan") & (k != "none")
        assert np.abs(bad[cmp].astype(np.float64) - flat[cmp]).max() > DECODE_BOUND, label


@pytest.mark.gpu
def test_step_rpn_decode(torch_mod):
    torch = torch_mod
    rpn, sel, kinds = rpn_decode_case()
    want = ref.rpn_decode(rpn, sel, DEC_HF, DEC_WF, DEC_H, DEC_W)
    out = DevOut(torch, want.shape)
    run_step("rpn_decode", [dev(torch, rpn), dev(torch, sel)], [out], n=DEC_N, h=DEC_HF, w=DEC_WF, count=DEC_K, win_h=DEC_H, win_w=DEC_W)
    ratio = check_boxes(out.read(), want, kinds, DEC_H, DEC_W, "gpu")
    print("rpn_decode: error / bound = %.3f" % ratio)
    assert ratio <= 1.0


# ================================================================================================ gather_proposals
@lru_cache(maxsize=None)
def gather_case():
    rng = np.random.default_rng(700)
    n, K, P = 2, 64, ref.PROPOSALS
    tl = rng.uniform(0, 0.6, (n, K, 2)) * [DEC_H, DEC_W]
    boxes = np.concatenate([tl, tl + rng.uniform(1, 0.4 * DEC_H, (n, K, 2))], axis=2).astype(F32)
    keep = np.full((n, P), -1, dtype=np.int32)
    keep[0, :40] = rng.permutation(K)[:40]               # out of order, a long -1 tail
    keep[1, :K] = np.arange(K)[::-1]                     # every box, descending
    keep[1, K:K + 5] = [3, 3, 0, 63, 3]                  # and repeats
    return boxes, keep


@pytest.mark.gpu
def test_step_gather_proposals(torch_mod):
    torch = torch_mod
    boxes, keep = gather_case()
    n, K, P = boxes.shape[0], boxes.shape[1], keep.shape[1]
    assert (n * P) % 256 and (np.diff(keep[0, :40]) < 0).any() and (keep[:, -200:] == -1).all()
    prop, norm, image = ref.gather_proposals(boxes, keep, DEC_H, DEC_W)
    o_prop, o_norm, o_img = DevOut(torch, prop.shape), DevOut(torch, norm.shape), DevOut(torch, image.shape, integer=True)
    run_step("gather_proposals", [dev(torch, boxes), dev(torch, keep)], [o_prop, o_norm, o_img], n=n, count=K, win_h=DEC_H, win_w=DEC_W)
    g_prop, g_norm, g_img = o_prop.read(), o_norm.read(), o_img.read()
    assert np.array_equal(g_prop.view(np.uint32), prop.view(np.uint32))
    assert np.array_equal(g_img, image)
    pad = keep < 0
    assert not g_prop[pad].view(np.uint32).any() and not g_norm[pad].view(np.uint32).any()
    # the quotient: within two ulps of float64's (which division instruction sequence the device uses is not pinned)
    err = np.abs(g_norm.astype(np.float64) - norm)
    assert (err <= 4 * 2.0 ** -24 * np.abs(norm)).all(), float((err / np.maximum(np.abs(norm), 1e-30)).max())
    assert (g_norm[~pad] > 0).all()


# ================================================================================================ crop_pool
CROP_MAPS = [(11, 13), (2, 2), (1, 13), (11, 1)]
CROP_CHANNELS = [4, 256]
CROP = 14


@lru_cache(maxsize=None)
def crop_case(mi, c):
    h, w = CROP_MAPS[mi]
    n, _, _, _, crop, _, boxes, bimg = roi_case(3, 3)     # the boxes do not depend on the map: on, at, beyond the border, flipped, empty
    assert crop == CROP and bimg[-3] == -1 and bimg[-2] == n and n == 2
    feat = np.random.default_rng(800 + 10 * mi + c).standard_normal((n, h, w, c)).astype(F32)
    return n, h, w, feat, boxes, bimg


@pytest.mark.gpu
@pytest.mark.parametrize("c", CROP_CHANNELS)
@pytest.mark.parametrize("mi", range(len(CROP_MAPS)), ids=["%dx%d" % m for m in CROP_MAPS])
def test_step_crop_pool(torch_mod, mi, c):
    torch = torch_mod
    from glomeruli_segmentation_amd import _lib
    n, h, w, feat, boxes, bimg = crop_case(mi, c)
    nb, half = len(boxes), CROP // 2
    assert (nb * half * half * (c // 4)) % 256
    fd, bd, idd = dev(torch, feat), dev(torch, boxes), dev(torch, bimg)
    out = DevOut(torch, (nb, half, half, c))
    run_step("crop_pool", [fd, bd, idd], [out], n=n, h=h, w=w, c=c, count=nb, crop=CROP)
    got = out.read()
    # bit for bit the 2 x 2 max of gs_roialign's crops: one sampling function under fp contract(off)
    crops = DevOut(torch, (nb, CROP, CROP, c))
    _lib.check(_lib.load().gs_roialign(fd.data_ptr(), n, h, w, c, bd.data_ptr(), idd.data_ptr(), nb, CROP, crops.ptr, None))
    assert np.array_equal(got.view(np.uint32), ref.pool2x2(crops.read()).view(np.uint32))
    # independently: the oracle's crop_and_resize, then the max, at the roialign test's tolerance
    want = ref.pool2x2(do.crop_and_resize(feat, boxes, CROP, box_image=bimg))
    err = float(np.abs(got - want).max())
    print("crop_pool %dx%d c %d: max error %.3g" % (h, w, c, err))
    assert err <= 1e-6 * max(1.0, float(np.abs(feat).max()))
    assert not got[-3:-1].any() and got[0].any()         # image -1 and image n: zeros


# ================================================================================================ avgpool
#            n  h  w   c   input
AVG_CASES = [(37, 4, 4, 128, "normal"), (3, 1, 1, 128, "normal"), (2, 7, 7, 8, "cancelling")]


@lru_cache(maxsize=None)
def avg_input(ci):
    n, h, w, c, kind = AVG_CASES[ci]
    rng = np.random.default_rng(900 + ci)
    x = rng.standard_normal((n, h * w, c)).astype(F32)
    if kind == "cancelling":                 # +-1e4 pairs around O(1) noise (the first element is noise alone)
        sign = np.where(np.arange(h * w - 1) % 2 == 0, 1e4, -1e4).astype(F32)
        x[:, 1:] += sign[None, :, None]
    return x


def test_avgpool_bound_holds_and_discriminates():
    for ci, (n, h, w, c, kind) in enumerate(AVG_CASES):
        x = avg_input(ci)
        hw = h * w
        want, bound = ref.avgpool(x), ref.avgpool_bound(x)
        err = np.abs(ref.avgpool(x, F32).astype(np.float64) - want)
        print("avgpool %dx%dx%d %s: fp32 sequential worst error / bound = %.3f" % (n, hw, c, kind, (err / bound).max()))
        assert (err <= bound).all()
        if kind == "cancelling":
            assert np.abs(want).max() < 2 and np.abs(x).max() > 9e3
        if hw > 1:
            dropped = np.abs(ref.avgpool(x, F32, drop_last=True).astype(np.float64) - want)
            assert (dropped > bound).any(), (ci, "drop_last")
            if kind == "normal":             # (under cancellation the honest bound is wider than mean / (hw - 1))
                assert (np.abs(ref.avgpool(x, F32, divisor=hw - 1).astype(np.float64) - want) > bound).any(), (ci, "hw - 1")


@pytest.mark.gpu
@pytest.mark.parametrize("ci", range(len(AVG_CASES)), ids=["%dx%dx%dx%d-%s" % c for c in AVG_CASES])
def test_step_avgpool(torch_mod, ci):
    torch = torch_mod
    n, h, w, c, kind = AVG_CASES[ci]
    x = avg_input(ci)
    want, bound = ref.avgpool(x), ref.avgpool_bound(x)
    out = DevOut(torch, want.shape)
    run_step("avgpool", [dev(torch, x)], [out], n=n, h=h, w=w, c=c)
    err = np.abs(out.read().astype(np.float64) - want)
    print("avgpool %dx%dx%d %s: worst error / bound = %.3f" % (n, h * w, c, kind, (err / bound).max()))
    assert (err <= bound).all()


# ================================================================================================ head_decode
@lru_cache(maxsize=None)
def head_case(total):
    """(head [total,6], prop [total,4], keep int32 [total], score kinds, box kinds): padded proposals (keep < 0, box zero) every
    seventh row; logits equal / +-200 apart / uniform; deltas by DELTA_KINDS"""
    rng = np.random.default_rng(1000 + total)
    head = np.zeros((total, 6), dtype=F32)
    tl = rng.uniform(0, 0.7, (total, 2)) * [DEC_H, DEC_W]
    prop = np.concatenate([tl, tl + rng.uniform(2, 0.5 * DEC_H, (total, 2))], axis=1).astype(F32)
    prop[:, [0, 2]] = np.minimum(prop[:, [0, 2]], DEC_H)
    prop[:, [1, 3]] = np.minimum(prop[:, [1, 3]], DEC_W)
    keep = np.arange(total, dtype=np.int32)
    score_kinds = np.empty(total, dtype=object)
    box_kinds = np.empty(total, dtype=object)
    for i in range(total):
        what = ["half", "zero", "one", "rest", "rest"][i % 5]
        mid = rng.uniform(-5, 5)
        d = rng.uniform(-30, 30)
        head[i, :2] = {"half": (mid, mid), "zero": (100, -100), "one": (-100, 100), "rest": (mid + d / 2, mid - d / 2)}[what]
        box_kinds[i] = DELTA_KINDS[(i // 2) % len(DELTA_KINDS)]
        head[i, 2:] = make_deltas(rng, box_kinds[i], i)
        if i % 7 == 3:
            keep[i], prop[i], what = -1 - (i % 2), 0, "padded"
        score_kinds[i] = what
    return head, prop, keep, score_kinds, box_kinds


@pytest.mark.gpu
@pytest.mark.parametrize("total", [600, 7])
def test_step_head_decode(torch_mod, total):
    torch = torch_mod
    head, prop, keep, sk, bk = head_case(total)
    assert {"half", "zero", "one", "rest", "padded"} <= set(sk) and total % 256
    want_s, want_b = ref.head_decode(head, prop, keep, DEC_H, DEC_W)
    o_s, o_b = DevOut(torch, (total,)), DevOut(torch, (total, 4))
    run_step("head_decode", [dev(torch, head), dev(torch, prop), dev(torch, keep)], [o_s, o_b], count=total, win_h=DEC_H, win_w=DEC_W)
    got_s, got_b = o_s.read(), o_b.read()
    assert (got_s[sk == "padded"] == F32(-1.0)).all()
    r_s = check_scores(got_s, want_s, sk, "gpu")
    kinds = bk.copy()
    kinds[(sk == "padded") & (bk != "nan")] = "none"     # a zero proposal decodes to a zero box, whatever its deltas
    r_b = check_boxes(got_b, want_b, kinds, DEC_H, DEC_W, "gpu")
    print("head_decode %d: score error / bound = %.3f, box error / bound = %.3f" % (total, r_s, r_b))
    assert r_s <= 1.0 and r_b <= 1.0


def test_head_case_reference_is_inside_its_bounds():
    for total in (600, 7):
        head, prop, keep, sk, bk = head_case(total)
        want_s, want_b = ref.head_decode(head, prop, keep, DEC_H, DEC_W)
        got_s, got_b = ref.head_decode(head, prop, keep, DEC_H, DEC_W, F32)
        assert (got_s[sk == "padded"] == -1).all() and (want_s[sk == "padded"] == -1).all()
        kinds = bk.copy()
        kinds[(sk == "padded") & (bk != "nan")] = "none"
        assert check_scores(got_s, want_s, sk, "fp32 restatement") <= 1.0 and check_boxes(got_b, want_b, kinds, DEC_H, DEC_W, "fp32") <= 1.0
