"""The detector's kernels (csrc/detect_ops.hip, csrc/detector.hip) at the shapes and inputs where they can go wrong.

1. the four convolution kernels behind launch_conv2d_nhwc, in the instances the public gs_conv2d_nhwc launches (weights NOT
   packed: conv2d_nhwc_tiled_kernel<false>, conv2d_nhwc_wide_kernel<4,false>; the packed-weight instances every layer of the
   detector runs, and the detector's glue kernels one step at a time, are in tests/test_detector_steps.py): CONV_CASES holds
   hand-written known answers for its choice, which a CPU test asks of the product itself (gs_conv2d_nhwc_form: conv_nhwc_form
   of csrc/detect_plan.h, the function the launcher switches over), one float64 reference, one bound for the family, and a CPU
   test showing that the bound rejects a dropped K-tail, a zeroed tap column and a one-pixel shift; likewise known answers for
   the detector's host plan (gs_detector_plan, gs_detector_layer_info): size chain, workspace bytes, batch limits, per-layer
   kernels;
2. gs_roialign against the float32 oracle, on the border, beyond it, at crop 1 and on degenerate maps;
3. gs_nms against a float32 restatement, exactly, on inputs whose arithmetic is exact;
4. the selection stages of the assembled detector (top-k, NMS, decode, gather, output) stage by stage against
   oracle/detector_oracle.py, with weights and thresholds chosen to produce ties, short lists, truncation and empty outputs;
5. gs_detector_detect_host bit for bit against forward_device across batch and window-size changes on one handle.

NOT reference parity: the reference's detector is an external frozen graph; every reference here is torch /
numpy or oracle/detector_oracle.py.
"""
import ctypes
import os
from collections import namedtuple
from functools import lru_cache

import numpy as np
import pytest

from oracle import detector_oracle as do

F32 = np.float32
REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def torch_mod():
    import torch
    assert torch.cuda.is_available(), "the gpu-marked tests need a HIP device"
    return torch


# ---------------------------------------------------------------------------------------------- 1. convolution forms
def conv_out_hw(h, w, kh, kw, stride, pad):
    return (h + 2 * pad - kh) // stride + 1, (w + 2 * pad - kw) // stride + 1


def conv_form(n, h, w, cin, kh, kw, cout, stride, pad, packed=False):
    """the library's answer (gs_conv2d_nhwc_form; no device): the kernel launch_conv2d_nhwc runs for the shape; packed=False is
    the public entry, whose weights are not packed"""
    from glomeruli_segmentation_amd import _lib
    name = ctypes.c_char_p()
    _lib.check(_lib.load().gs_conv2d_nhwc_form(n, h, w, cin, kh, kw, cout, stride, pad, int(packed), ctypes.byref(name)))
    return name.value.decode()


ConvCase = namedtuple("ConvCase", "name form n h w cin kh kw cout stride pad bias relu edges")
CONV_FORMS = ("generic", "smallcin", "tiled", "wide")
# the edges every form must be seen at ...
COMMON_EDGES = ("ragged_pix", "image_boundary", "cout_lt32", "cout_33_63", "cout_gt64_ragged", "rect", "stride1", "stride2",
                "stride3", "pad0", "pad_big", "nobias", "norelu")
# ... and the ones of its own K walk / its side of a dispatch boundary
FORM_EDGES = {"smallcin": ("odd_K", "K512"), "generic": ("cin_lt8_bigK", "cin9", "cin12"), "tiled": ("hw63_cin32",),
              "wide": ("hw64_cin32", "total1", "total_odd", "total_even")}


def conv_has_edge(c, edge):
    """whether the SHAPE of case c has the edge (a claim in c.edges is checked against this)"""
    ho, wo = conv_out_hw(c.h, c.w, c.kh, c.kw, c.stride, c.pad)
    K = c.kh * c.kw * c.cin
    ptile, ctile = (32, 32) if c.form == "generic" else (64, 64)      # pixels / channels of a wave's tile
    total = K // 32                                                    # the wide kernel's 32-channel blocks
    return {
        "ragged_pix": (c.n * ho * wo) % ptile != 0,
        "image_boundary": c.n > 1 and (ho * wo) % 64 != 0,
        "cout_lt32": c.cout < 32,
        "cout_33_63": 32 < c.cout < 64,
        "cout_gt64_ragged": c.cout > 64 and c.cout % ctile != 0,
        "rect": c.kh != c.kw and c.h != c.w,
        "stride1": c.stride == 1, "stride2": c.stride == 2, "stride3": c.stride == 3,
        "pad0": c.pad == 0,
        "pad_big": 2 * c.pad > max(c.kh, c.kw) - 1,
        "nobias": not c.bias, "norelu": not c.relu,
        "odd_K": K % 2 == 1, "K512": K == 512,
        "cin_lt8_bigK": c.cin < 8 and K > 512, "cin9": c.cin == 9, "cin12": c.cin == 12,
        "hw63_cin32": ho * wo == 63 and c.cin == 32, "hw64_cin32": ho * wo == 64 and c.cin == 32,
        "total1": total == 1, "total_odd": total > 1 and total % 2 == 1, "total_even": total % 2 == 0,
    }[edge]


def _cc(name, form, n, h, w, cin, kh, kw, cout, stride, pad, bias, relu, *edges):
    return ConvCase(name, form, n, h, w, cin, kh, kw, cout, stride, pad, bias, relu, frozenset(edges))


CONV_CASES = [
    #    name  form         n   h   w cin kh  kw cout s  p  bias   relu
    _cc("S1", "smallcin", 2, 19, 23, 3, 3, 3, 37, 2, 1, True, True, "ragged_pix", "image_boundary", "cout_33_63", "stride2", "odd_K"),
    _cc("S2", "smallcin", 1, 12, 20, 4, 8, 16, 20, 1, 0, False, True, "K512", "rect", "cout_lt32", "pad0", "stride1", "nobias"),
    _cc("S3", "smallcin", 1, 20, 17, 5, 3, 2, 70, 3, 2, True, False, "pad_big", "stride3", "cout_gt64_ragged", "norelu"),
    _cc("S4", "smallcin", 1, 16, 15, 7, 7, 7, 64, 2, 3, True, True, "odd_K"),
    _cc("S5", "smallcin", 2, 9, 11, 1, 3, 3, 5, 1, 1, True, True, "odd_K", "cout_lt32"),
    _cc("G1", "generic", 1, 14, 13, 7, 9, 9, 33, 1, 4, True, True, "cin_lt8_bigK", "cout_33_63", "stride1", "ragged_pix"),
    _cc("G2", "generic", 2, 10, 11, 9, 3, 3, 20, 2, 0, False, True, "cin9", "image_boundary", "cout_lt32", "stride2", "pad0", "nobias"),
    _cc("G3", "generic", 1, 13, 17, 12, 2, 3, 70, 3, 2, True, False, "cin12", "pad_big", "stride3", "cout_gt64_ragged", "rect", "norelu"),
    _cc("G4", "generic", 1, 12, 13, 12, 3, 3, 20, 1, 1, True, True, "cin12"),
    _cc("T1", "tiled", 2, 21, 37, 16, 3, 3, 70, 1, 1, True, True, "ragged_pix", "image_boundary", "cout_gt64_ragged", "stride1"),
    _cc("T2", "tiled", 3, 30, 19, 24, 3, 2, 40, 2, 0, False, False, "rect", "cout_33_63", "stride2", "pad0", "nobias", "norelu"),
    _cc("T3", "tiled", 1, 9, 7, 32, 3, 3, 64, 1, 1, True, True, "hw63_cin32"),
    _cc("T4", "tiled", 1, 17, 14, 8, 1, 3, 6, 3, 2, True, True, "pad_big", "stride3", "cout_lt32"),
    _cc("T5", "tiled", 1, 12, 12, 8, 8, 8, 32, 1, 0, True, True, "pad0"),                 # K = 512 at cin 8 is not smallcin
    _cc("T6", "tiled", 1, 20, 20, 40, 3, 3, 33, 1, 1, True, True, "cout_33_63"),           # many pixels, cin % 32 != 0
    _cc("T7", "tiled", 1, 5, 5, 8, 1, 1, 6, 1, 0, True, True, "cout_lt32", "pad0"),        # one chunk in all
    _cc("W1", "wide", 1, 8, 8, 32, 1, 1, 64, 1, 0, True, True, "total1", "hw64_cin32", "pad0", "stride1"),
    _cc("W2", "wide", 2, 21, 37, 32, 3, 3, 70, 1, 1, True, True, "total_odd", "ragged_pix", "image_boundary", "cout_gt64_ragged"),
    _cc("W3", "wide", 1, 30, 19, 64, 3, 3, 40, 2, 1, False, False, "total_even", "stride2", "cout_33_63", "nobias", "norelu"),
    _cc("W4", "wide", 3, 11, 13, 96, 3, 3, 20, 1, 1, True, True, "total_odd", "cout_lt32", "image_boundary"),
    _cc("W5", "wide", 1, 29, 31, 32, 2, 3, 65, 3, 2, True, True, "pad_big", "stride3", "rect", "total_even", "cout_gt64_ragged"),
    _cc("W6", "wide", 2, 13, 17, 64, 1, 1, 72, 1, 0, True, True, "total_even", "pad0", "cout_gt64_ragged"),
    _cc("W7", "wide", 1, 16, 8, 32, 1, 1, 7, 1, 0, True, False, "total1", "cout_lt32"),    # two whole pixel tiles, one block
]
CONV_BY_NAME = {c.name: c for c in CONV_CASES}

# max|got - ref64| <= CONV_TAU * max(1, max|ref64|), one bound for the family: four times the worst error of torch's fp32
# CPU convolution against the float64 reference over CONV_CASES (measured 8.8e-7 on W4, K = 3x3x96, x 4;
# test_conv_bounds_discriminate prints it).  55 times tighter than the 2e-4 * max(1, max|ref|) that
# test_detector_primitives_self_consistency's absolute 2e-4 amounts to.
CONV_TAU = 3.52e-6


@lru_cache(maxsize=None)
def conv_data(name):
    """(x [n,h,w,cin], w [kh,kw,cin,cout], bias [cout]) float32 numpy, seeded by the case"""
    c = CONV_BY_NAME[name]
    rng = np.random.default_rng(1000 + CONV_CASES.index(c))
    x = rng.standard_normal((c.n, c.h, c.w, c.cin)).astype(F32)
    w = (rng.standard_normal((c.kh, c.kw, c.cin, c.cout)) * 0.2).astype(F32)
    b = rng.standard_normal(c.cout).astype(F32)
    return x, w, b


def conv_reference(c, x, w, b, dtype):
    """torch's CPU convolution, bias and ReLU in `dtype` -> [n,ho,wo,cout] numpy of that dtype"""
    import torch
    import torch.nn.functional as Fn
    xt = torch.from_numpy(x).to(dtype).permute(0, 3, 1, 2)
    wt = torch.from_numpy(w).to(dtype).permute(3, 2, 0, 1)
    y = Fn.conv2d(xt, wt, torch.from_numpy(b).to(dtype) if c.bias else None, stride=c.stride, padding=c.pad)
    if c.relu:
        y = torch.relu(y)
    return y.permute(0, 2, 3, 1).contiguous().numpy()


@lru_cache(maxsize=None)
def conv_ref64(name):
    import torch
    c = CONV_BY_NAME[name]
    return conv_reference(c, *conv_data(name), torch.float64)


def conv_bound(ref64):
    return CONV_TAU * max(1.0, float(np.abs(ref64).max()))


def test_conv_cases_cover_every_form_and_edge():
    assert 20 <= len(CONV_CASES) <= 25 and len(CONV_BY_NAME) == len(CONV_CASES)
    for c in CONV_CASES:
        assert conv_form(c.n, c.h, c.w, c.cin, c.kh, c.kw, c.cout, c.stride, c.pad) == c.form, c.name
        ho, wo = conv_out_hw(c.h, c.w, c.kh, c.kw, c.stride, c.pad)
        assert c.n * ho * wo * c.cout <= 300000, c.name
        for e in c.edges:                       # a claim holds for the shape ...
            assert e in COMMON_EDGES + FORM_EDGES.get(c.form, ()), (c.name, e)
            assert conv_has_edge(c, e), (c.name, e)
    for form in CONV_FORMS:                     # ... and every edge is claimed, per form
        claimed = set().union(*[c.edges for c in CONV_CASES if c.form == form])
        missing = [e for e in COMMON_EDGES + FORM_EDGES.get(form, ()) if e not in claimed]
        assert not missing, (form, missing)
    # the dispatch boundaries, from both sides
    assert conv_form(1, 12, 20, 4, 8, 16, 20, 1, 0) == "smallcin" and conv_form(1, 12, 20, 4, 8, 17, 20, 1, 0) == "generic"
    assert conv_form(1, 9, 7, 32, 3, 3, 64, 1, 1) == "tiled" and conv_form(1, 8, 8, 32, 3, 3, 64, 1, 1) == "wide"
    assert [conv_form(1, 12, 13, ci, 3, 3, 20, 1, 1) for ci in (7, 8, 9)] == ["smallcin", "tiled", "generic"]


def test_conv_bounds_discriminate():
    """torch's fp32 CPU convolution passes the bound on every case; the float64 reference with the last flattened-K element's
    weights zeroed, with the last tap column zeroed, or shifted by one pixel along w does not"""
    import torch
    worst = {}
    for c in CONV_CASES:
        x, w, b = conv_data(c.name)
        ref = conv_ref64(c.name)
        bound = conv_bound(ref)
        err = float(np.abs(conv_reference(c, x, w, b, torch.float32).astype(np.float64) - ref).max())
        worst[c.name] = err / max(1.0, float(np.abs(ref).max()))
        assert err <= bound, (c.name, err, bound)
        w_tail = w.copy()
        w_tail[c.kh - 1, c.kw - 1, c.cin - 1, :] = 0
        w_col = w.copy()
        w_col[:, c.kw - 1] = 0
        planted = {"K-tail": conv_reference(c, x, w_tail, b, torch.float64), "tap column": conv_reference(c, x, w_col, b, torch.float64),
                   "shift": np.roll(ref, 1, axis=2)}
        for what, bad in planted.items():
            assert np.abs(bad - ref).max() > bound, (c.name, what)
    top = max(worst, key=worst.get)
    print("conv: torch fp32 CPU vs float64, worst error / max(1, max|ref|) = %.3g (case %s); x4 = %.3g; CONV_TAU = %.3g; "
          "worst error / bound = %.3f" % (worst[top], top, 4 * worst[top], CONV_TAU, worst[top] / CONV_TAU))
    # no looser than the 2e-4 * max(1, max|ref|) the detector's convolutions were held to before
    assert CONV_TAU <= 2e-4


def test_conv_form_refusals():
    """an empty output is GS_ERR_INVALID; packed weights with a shape the tiled / wide kernels cannot take (or an empty output)
    is GS_ERR_UNSUPPORTED, both with the launcher's messages; packed is a flag beside the form, not a form"""
    from glomeruli_segmentation_amd import _lib
    with pytest.raises(_lib.GlomsegError, match="gs_conv2d_nhwc: empty output") as e:
        conv_form(1, 2, 2, 8, 3, 3, 8, 1, 0)
    assert e.value.status == 1
    for shape in ((1, 12, 13, 7, 3, 3, 20, 1, 1), (1, 12, 13, 12, 3, 3, 20, 1, 1), (1, 2, 2, 8, 3, 3, 8, 1, 0)):
        with pytest.raises(_lib.GlomsegError, match="conv2d_nhwc_packed4: shape not supported by the packed-weight kernel") as e:
            conv_form(*shape, packed=True)
        assert e.value.status == 4
    assert conv_form(1, 9, 7, 32, 3, 3, 64, 1, 1, packed=True) == "tiled" and conv_form(1, 8, 8, 32, 3, 3, 64, 1, 1, packed=True) == "wide"


# ---- the detector's host plan (csrc/detect_plan.h through gs_detector_layer_info / gs_detector_plan; no device)
# the rows synthetic_weights was written against: name -> (k, cin, cout), in launch order
DET_LAYER_ROWS = [("backbone.c1", 3, 16, 64, 1, 1, 1), ("backbone.c2", 3, 64, 64, 1, 1, 1), ("backbone.c3", 3, 64, 128, 2, 1, 1),
                  ("backbone.c4", 3, 128, 128, 1, 1, 1), ("backbone.c5", 3, 128, 256, 2, 1, 1), ("backbone.c6", 3, 256, 256, 1, 1, 1),
                  ("rpn.conv", 3, 256, 256, 1, 1, 1), ("rpn.head", 1, 256, 72, 1, 0, 0), ("head.h1", 1, 256, 128, 1, 0, 1),
                  ("head.h2", 3, 128, 128, 2, 1, 1), ("head.fc", 1, 128, 6, 1, 0, 0)]
# (n, H, W) -> h2 x w2, h4 x w4, h8 x w8, hf x wf, workspace bytes: worked out from the forward's arithmetic before the plan existed
DET_PLAN_KNOWN = {
    (16, 1000, 1000): ((500, 500), (250, 250), (125, 125), (63, 63), 1730729728),
    (1, 32, 32): ((16, 16), (8, 8), (4, 4), (2, 2), 22861568),
    (2, 33, 47): ((17, 24), (9, 12), (5, 6), (3, 3), 45836288),
    (3, 50, 37): ((25, 19), (13, 10), (7, 5), (4, 3), 68834048),
}
# per-layer kernels with packed weights.  1000 x 1000: c1 (cin 16), head.h1 (49 pixels), head.h2 (16 pixels) and head.fc (1 pixel)
# are tiled, the other seven wide; 32 x 32: only c2 (8 x 8 = 64 pixels) is wide
DET_PLAN_FORMS = {
    (16, 1000, 1000): ["tiled", "wide", "wide", "wide", "wide", "wide", "wide", "wide", "tiled", "tiled", "tiled"],
    (1, 32, 32): ["tiled", "wide", "tiled", "tiled", "tiled", "tiled", "tiled", "tiled", "tiled", "tiled", "tiled"],
}


# synthetic_weights(0): sha256 over name + bytes of every tensor in order, taken at the commit before detector.LAYERS became layers()
SYNTHETIC_WEIGHTS_SEED0_SHA256 = "018db6e5b8aec9de50a02373fb6ceda8b5c780af473520bb6c5f65dde87bc970"


def detector_layer_rows():
    from glomeruli_segmentation_amd import _lib
    lib = _lib.load()
    name, v = ctypes.c_char_p(), [ctypes.c_int() for _ in range(6)]
    rows = []
    while lib.gs_detector_layer_info(len(rows), ctypes.byref(name), *[ctypes.byref(x) for x in v]):
        rows.append((name.value.decode(),) + tuple(x.value for x in v))
        assert len(rows) <= 16
    return rows


def test_detector_layer_table_and_lazy_import():
    """gs_detector_layer_info enumerates the 11 rows synthetic_weights produced its tensors for (and 0 outside them); detector.py
    reads them lazily: importing it does not load the library; the seeded arrays are what they were"""
    import hashlib
    import subprocess
    import sys
    from glomeruli_segmentation_amd import _lib
    from glomeruli_segmentation_amd import detector
    rows = detector_layer_rows()
    assert rows == DET_LAYER_ROWS and len(rows) == 11
    lib = _lib.load()
    assert lib.gs_detector_layer_info(-1, None, None, None, None, None, None, None) == 0
    assert lib.gs_detector_layer_info(0, None, None, None, None, None, None, None) == 1
    assert list(detector.layers().items()) == [(r[0], r[1:4]) for r in DET_LAYER_ROWS]
    assert lib.gs_detector_num_proposals() == do.PROPOSALS == 300 and lib.gs_detector_max_detections() == do.MAX_DET == 100
    sd = detector.synthetic_weights(0)
    assert [(k, v.shape) for k, v in sd.items()] == [
        (r[0] + s, shape) for r in DET_LAYER_ROWS for s, shape in ((".weight", (r[1], r[1], r[2], r[3])), (".bias", (r[3],)))]
    h = hashlib.sha256()
    for k, v in sd.items():
        h.update(k.encode() + v.tobytes())
    assert h.hexdigest() == SYNTHETIC_WEIGHTS_SEED0_SHA256
    code = ("import sys; import glomeruli_segmentation_amd.detector as d, glomeruli_segmentation_amd._lib as l; "
            "assert l._lib is None, 'importing detector loaded the library'; d.layers(); assert l._lib is not None")
    subprocess.run([sys.executable, "-c", code], check=True, cwd=REPO, timeout=120)


def detector_plan(n, H, W):
    from glomeruli_segmentation_amd import detector
    return detector.plan(n, H, W)


@pytest.mark.parametrize("shape", sorted(DET_PLAN_KNOWN))
def test_detector_plan_known_answers(shape):
    n, H, W = shape
    (h2, w2), (h4, w4), (h8, w8), (hf, wf), ws_bytes = DET_PLAN_KNOWN[shape]
    p = detector_plan(n, H, W)
    L = p.layers
    assert p.n_layers == 11 and (p.hf, p.wf) == (hf, wf) and p.workspace_bytes == ws_bytes
    P = 300
    want = [(n, h2, w2, h2, w2), (n, h4, w4, h4, w4), (n, h4, w4, h8, w8), (n, h8, w8, h8, w8), (n, h8, w8, hf, wf), (n, hf, wf, hf, wf),
            (n, hf, wf, hf, wf), (n, hf, wf, hf, wf), (n * P, 7, 7, 7, 7), (n * P, 7, 7, 4, 4), (n * P, 1, 1, 1, 1)]
    assert [(L[i].images, L[i].in_h, L[i].in_w, L[i].out_h, L[i].out_w) for i in range(11)] == want
    forms = [CONV_FORMS[L[i].form] for i in range(11)]
    # the plan's form codes are the single-shape entry's answers with packed weights
    for i, (name, k, cin, cout, stride, pad, relu) in enumerate(DET_LAYER_ROWS):
        assert conv_form(L[i].images, L[i].in_h, L[i].in_w, cin, k, k, cout, stride, pad, packed=True) == forms[i], name
    if shape in DET_PLAN_FORMS:
        assert forms == DET_PLAN_FORMS[shape]


def test_detector_plan_limits():
    """the forward's three limit checks (anchors < 2^24, the 32-bit byte offsets of c1's input and of the pooled crops): the last
    batch accepted and the first refused at two window sizes; windows under 32 x 32 are refused as the forward refuses them"""
    from glomeruli_segmentation_amd import _lib
    for (H, W, last) in ((1000, 1000, 134), (32, 32, 142)):
        assert detector_plan(last, H, W).workspace_bytes > 0
        with pytest.raises(_lib.GlomsegError, match=r"batch too large \(n=%d windows of %dx%d\): split it" % (last + 1, H, W)) as e:
            detector_plan(last + 1, H, W)
        assert e.value.status == 1          # GS_ERR_INVALID
    for bad in ((0, 64, 64), (1, 31, 64), (1, 64, 31)):
        with pytest.raises(_lib.GlomsegError, match="windows must be at least 32x32") as e:
            detector_plan(*bad)
        assert e.value.status == 1


@pytest.mark.gpu
@pytest.mark.parametrize("name", [c.name for c in CONV_CASES])
def test_conv_form_against_float64(torch_mod, name):
    torch = torch_mod
    from glomeruli_segmentation_amd import _lib
    lib = _lib.load()
    c = CONV_BY_NAME[name]
    x, w, b = conv_data(name)
    ref = conv_ref64(name)
    xd, wd, bd = torch.from_numpy(x).cuda(), torch.from_numpy(w).cuda(), torch.from_numpy(b).cuda()
    out = torch.full(ref.shape, float("nan"), device="cuda")
    _lib.check(lib.gs_conv2d_nhwc(xd.data_ptr(), c.n, c.h, c.w, c.cin, wd.data_ptr(), c.kh, c.kw, c.cout,
                                  bd.data_ptr() if c.bias else None, c.stride, c.pad, int(c.relu), out.data_ptr(), None))
    torch.cuda.synchronize()
    got = out.cpu().numpy().astype(np.float64)
    assert not np.isnan(got).any(), "output elements left unwritten"
    err, bound = float(np.abs(got - ref).max()), conv_bound(ref)
    print("conv %s (%s): error / bound = %.3f (error %.3g relative to max(1, max|ref|))" % (
        name, c.form, err / bound, err / max(1.0, float(np.abs(ref).max()))))
    assert err <= bound, (name, c.form, err, bound)


# ---------------------------------------------------------------------------------------------- 2. gs_roialign
def test_crop_and_resize_oracle_crop1_and_box_image():
    """crop == 1 samples 0.5 (y1 + y2) (h - 1), 0.5 (x1 + x2) (w - 1) (tf.image.crop_and_resize); hand-computed values"""
    feat = np.arange(12, dtype=F32).reshape(3, 4, 1)          # feat[y, x] = 4 y + x
    # centre (0.5 * 1 * 2, 0.5 * 0.5 * 3) = (1, 0.75): 4 + 0.75
    got = do.crop_and_resize(feat, np.array([[0, 0, 1, 0.5]], F32), 1)
    assert got.shape == (1, 1, 1, 1) and got[0, 0, 0, 0] == F32(4.75)
    # centre (0.5 * 1.5 * 2, ..) = (1.5, 1.5): mean of the four cells (1,1) (1,2) (2,1) (2,2) = 7.5; a flipped box has the same centre
    assert do.crop_and_resize(feat, np.array([[0.5, 0, 1, 1]], F32), 1)[0, 0, 0, 0] == F32(7.5)
    assert do.crop_and_resize(feat, np.array([[1, 1, 0.5, 0]], F32), 1)[0, 0, 0, 0] == F32(7.5)
    # centre beyond the border: extrapolated
    assert do.crop_and_resize(feat, np.array([[0.5, 0, 2, 1]], F32), 1)[0, 0, 0, 0] == 0
    # per-box image index; outside [0, n) gives zeros; crop > 1 is what it was
    feats = np.stack([feat, feat + 100])
    boxes = np.array([[0, 0, 1, 1]] * 4, F32)
    got = do.crop_and_resize(feats, boxes, 2, box_image=[1, 0, -1, 2])
    assert np.array_equal(got[0, :, :, 0], [[100, 103], [108, 111]]) and np.array_equal(got[1, :, :, 0], [[0, 3], [8, 11]])
    assert not got[2:].any()
    assert np.array_equal(do.crop_and_resize(feat, boxes[:1], 2), got[1:2])


ROI_MAPS = [(1, 13), (11, 1), (2, 2), (11, 13)]
ROI_CROPS = [1, 2, 7, 14]
ROI_CHANNELS = [1, 5, 256]


def roi_case(mi, ci):
    """(n, h, w, c, crop, feat, boxes, box_image) of one case: a handful of boxes on, at, just beyond and far outside the border"""
    h, w = ROI_MAPS[mi]
    crop = ROI_CROPS[ci]
    c = ROI_CHANNELS[(mi + ci) % 3]
    n = 2
    rng = np.random.default_rng(100 * mi + ci)
    feat = rng.standard_normal((n, h, w, c)).astype(F32)
    up = np.nextafter(F32(1), F32(2))            # one ulp beyond the border
    boxes = [
        [0, 0, 1, 1],                            # the whole map: the last sample on h-1 / w-1 (exactly, for crop 2 and 7)
        [0.25, 0.25, 1, 1], [0, 0.5, 0.75, 1],   # dyadic: 0.75 (h-1) / 6 and 0.5 (w-1) / 6 round nowhere at crop 7 on the 11x13 map
        [0, 0, up, 1], [0, 0, 1, up], [0.25, 0.25, up, up],   # one ulp beyond
        [-0.0, -0.0, 1, 1],
        [1.5, 1.5, 2, 2], [-1, -1, -0.5, -0.5], [0.2, 1.25, 0.8, 1.5],   # fully outside (one of them in x only)
        [0.9, 0.1, 0.2, 0.8], [0.3, 0.9, 0.7, 0.2],                      # flipped in y / in x
        [0.5, 0.5, 0.5, 0.5], [1, 1, 1, 1],                              # zero area: every sample the same point
        [0.1, 0.2, 0.7, 0.9], [-0.2, 0.3, 0.5, 1.2],                     # ordinary, partly outside
        [0, 0, 1, 1], [0, 0, 1, 1],                                      # box_image -1 and n: guarded to zeros
        [0.33, 0.11, 0.77, 0.95],
    ]
    boxes = np.array(boxes, dtype=F32)
    bimg = np.array([i % n for i in range(len(boxes))], dtype=np.int32)
    bimg[-3], bimg[-2] = -1, n
    return n, h, w, c, crop, feat, boxes, bimg


def test_roialign_cases_reach_the_edges():
    totals = []
    for mi in range(len(ROI_MAPS)):
        for ci in range(len(ROI_CROPS)):
            n, h, w, c, crop, feat, boxes, bimg = roi_case(mi, ci)
            totals.append(len(boxes) * crop * crop * c)
    assert any(t % 256 for t in totals) and any(t > 256 for t in totals)
    assert {ROI_CHANNELS[(mi + ci) % 3] for mi in range(4) for ci in range(4) if ROI_CROPS[ci] == 1} == set(ROI_CHANNELS)
    # on the 11x13 map at crop 7 the dyadic boxes' last samples land exactly on the border (inside), one ulp beyond is outside
    n, h, w, c, crop, feat, boxes, bimg = roi_case(3, 2)
    ref = do.crop_and_resize(feat, boxes, crop, box_image=bimg)
    assert ref[0, -1, -1].all() and ref[1, -1, -1].all() and ref[2, -1, -1].all()
    assert not ref[3, -1].any() and ref[3, 0].all() and not ref[4, :, -1].any() and ref[4, :, 0].all()
    assert not ref[7:10].any() and not ref[-3:-1].any() and ref[-1].all()


@pytest.mark.gpu
@pytest.mark.parametrize("mi", range(len(ROI_MAPS)))
@pytest.mark.parametrize("ci", range(len(ROI_CROPS)))
def test_roialign_against_float32_oracle(torch_mod, mi, ci):
    torch = torch_mod
    from glomeruli_segmentation_amd import _lib
    lib = _lib.load()
    n, h, w, c, crop, feat, boxes, bimg = roi_case(mi, ci)
    ref = do.crop_and_resize(feat, boxes, crop, box_image=bimg)
    fd, bd, idd = torch.from_numpy(feat).cuda(), torch.from_numpy(boxes).cuda(), torch.from_numpy(bimg).cuda()
    out = torch.full(ref.shape, float("nan"), device="cuda")
    _lib.check(lib.gs_roialign(fd.data_ptr(), n, h, w, c, bd.data_ptr(), idd.data_ptr(), len(boxes), crop, out.data_ptr(), None))
    torch.cuda.synchronize()
    got = out.cpu().numpy()
    assert not np.isnan(got).any()
    # the extrapolated samples (exactly 0 in the oracle; an interpolated sample of these maps never is) are the same set ...
    assert np.array_equal(got == 0, ref == 0), np.argwhere((got == 0) != (ref == 0))[:5]
    # ... and everything else is the same arithmetic in the same order
    err = float(np.abs(got - ref).max())
    print("roialign %dx%d c %d crop %d: max error %.3g" % (h, w, c, crop, err))
    assert err <= 1e-6 * max(1.0, float(np.abs(feat).max()))


# ---------------------------------------------------------------------------------------------- 3. gs_nms
NmsCase = namedtuple("NmsCase", "name boxes scores iou_thr score_thr max_out exact_pairs")


def _grid_boxes(rng, k, max_size=32):
    """k boxes with every coordinate a multiple of 1/64 in [0, 4]: areas and intersections are exact in float32"""
    size = rng.integers(1, max_size + 1, (k, 2))
    y1x1 = (rng.integers(0, 257, (k, 2)) * (256 - size) // 256)
    return (np.concatenate([y1x1, y1x1 + size], 1) / 64.0).astype(F32)


@lru_cache(maxsize=None)
def nms_cases():
    cases = []

    def add(name, boxes, scores, iou_thr=0.3717, score_thr=0.25, max_out=None, exact=False):
        boxes = np.asarray(boxes, dtype=F32).reshape(-1, 4)
        scores = np.asarray(scores, dtype=F32).reshape(-1)
        assert np.array_equal(boxes * 64, np.round(boxes * 64)) and boxes.min(initial=0) >= 0 and boxes.max(initial=0) <= 4
        cases.append(NmsCase(name, boxes, scores, iou_thr, score_thr, len(scores) + 7 if max_out is None else max_out, exact))

    rng = np.random.default_rng(5)
    add("k0", np.zeros((0, 4)), np.zeros(0))
    add("k1", [[0.5, 0.5, 1.5, 2]], [0.9])
    add("k1_below", [[0.5, 0.5, 1.5, 2]], [0.25])
    for k in (64, 65, 300):
        add("k%d" % k, _grid_boxes(rng, k, 96), rng.permutation(k) / F32(k))                  # distinct scores, some below the threshold
    add("k4200", _grid_boxes(rng, 4200, 24), rng.permutation(4200) / F32(4200), score_thr=0.0078125)   # 66 mask words: the strided loops
    add("k4200_ties", _grid_boxes(rng, 4200, 40), rng.integers(1, 9, 4200) / F32(8), iou_thr=0.2917, score_thr=0.0625)
    add("all_below", _grid_boxes(rng, 70), np.where(np.arange(70) % 2, 0.25, 0.125))          # at or below: n_keep == 0
    add("all_equal", _grid_boxes(rng, 130, 96), np.full(130, 0.5))                            # lower index first
    add("tie_groups", _grid_boxes(rng, 300, 96), rng.integers(0, 5, 300) / F32(4), score_thr=0.0)
    add("identical", np.tile([[1, 1, 2, 2.5]], (70, 1)), rng.permutation(70) / F32(64) + 1)   # one survivor
    b = _grid_boxes(rng, 100, 96)
    b[::5, 2] = b[::5, 0]                    # zero height
    b[1::10, 3] = b[1::10, 1]                # zero width
    b[2::7] = b[2::7][:, [2, 1, 0, 3]]       # flipped in y
    b[3::11] = b[3::11][:, [0, 3, 2, 1]]     # flipped in x
    add("zero_area_and_flipped", b, rng.permutation(100) / F32(128) + 0.5, iou_thr=0.2917)
    # IoU exactly 1/2 at threshold 1/2 is NOT suppressed; just above it is
    add("exact_threshold", [[0, 0, 1, 1], [0, 0, 1, 2], [2, 2, 3, 3], [3, 3, 2, 2], [0, 2.5, 1.5, 4], [0, 2.5, 0.75, 4],
                            [2, 0, 3, 1], [2, 0, 3, 2 - 1 / 64]], [0.9, 0.8, 0.7, 0.6, 0.5, 0.45, 0.4, 0.35], iou_thr=0.5, exact=True)
    base = cases[5]                          # k300
    assert base.name == "k300"
    for mo in (0, 1, 10, 307):
        add("k300_max_out_%d" % mo, base.boxes, base.scores, max_out=mo)
    return {c.name: c for c in cases}


NMS_NAMES = ["k0", "k1", "k1_below", "k64", "k65", "k300", "k4200", "k4200_ties", "all_below", "all_equal", "tie_groups", "identical",
             "zero_area_and_flipped", "exact_threshold", "k300_max_out_0", "k300_max_out_1", "k300_max_out_10", "k300_max_out_307"]


def test_nms_oracle_against_nms_sorted():
    """on score-sorted input with ordinary boxes nms_unsorted is nms_sorted; on unsorted input it is nms_sorted of the
    sorted list, mapped back"""
    rng = np.random.default_rng(9)
    boxes = _grid_boxes(rng, 200, 96)
    scores = np.sort(rng.permutation(200).astype(F32) / F32(200))[::-1].copy()
    for thr, sthr, mo in ((0.5, 0.25, 1000), (0.25, 0.0, 20), (0.75, 0.5, 1000)):
        want = do.nms_sorted(boxes, scores, F32(thr), F32(sthr), mo)
        assert 0 < len(want) < 200 and do.nms_unsorted(boxes, scores, thr, sthr, mo) == want
        perm = rng.permutation(200)
        inv = np.argsort(perm)
        assert do.nms_unsorted(boxes[inv], scores[inv], thr, sthr, mo) == [int(perm[i]) for i in want]
    # box_iou: the scalar iou on ordinary boxes, the mirror image on flipped ones, 0 on empty ones
    a, B = boxes[0], boxes[1:]
    assert np.array_equal(do.box_iou(a, B), np.array([do.iou(a, b) for b in B], dtype=F32))
    assert np.array_equal(do.box_iou(a[[2, 3, 0, 1]], B[:, [0, 3, 2, 1]]), do.box_iou(a, B))
    assert not do.box_iou([1, 1, 1, 2], B).any() and not do.box_iou(a, np.array([[0, 0, 1, 0], [0, 0, 1, 1]], F32))[:1].any()
    assert do.box_iou([0, 0, 1, 1], [[0, 0, 1, 2]])[0] == 0.5


def test_nms_cases_are_decided_by_exact_arithmetic():
    """float64 IoU of every pair of every case: none within 1e-6 of the threshold (a pair that close could be decided by a
    rounding), except the deliberate pairs at exactly the threshold; and the cases reach what they are for"""
    cases = nms_cases()
    assert sorted(cases) == sorted(NMS_NAMES)
    for c in cases.values():
        exact = 0
        for i in range(len(c.boxes) - 1):
            v = do.iou64(c.boxes[i], c.boxes[i + 1:], normalise=True)
            d = np.abs(v - float(F32(c.iou_thr)))          # the threshold the kernel gets
            assert not ((d <= 1e-6) & (d > 0)).any(), c.name
            exact += int((d == 0).sum())
        assert (exact > 0) == c.exact_pairs, (c.name, exact)
    keep = {name: do.nms_unsorted(c.boxes, c.scores, c.iou_thr, c.score_thr, c.max_out) for name, c in cases.items()}
    assert keep["k0"] == [] and keep["k1"] == [0] and keep["k1_below"] == [] and keep["all_below"] == []
    assert len(keep["identical"]) == 1 and keep["identical"][0] == int(np.argmax(cases["identical"].scores))
    assert keep["all_equal"] == sorted(keep["all_equal"]) and 1 < len(keep["all_equal"]) < 130
    assert keep["exact_threshold"] == [0, 1, 2, 4, 5, 6]        # the flipped copy and the pair just above 1/2 go, the pairs at 1/2 stay
    assert 300 > len(keep["k300"]) > 10 and [len(keep["k300_max_out_%d" % m]) for m in (0, 1, 10, 307)] == [0, 1, 10, len(keep["k300"])]
    assert keep["k300_max_out_10"] == keep["k300"][:10]
    for name in ("k4200", "k4200_ties"):                         # survivors and victims in the words beyond the 64th
        n_valid = int((cases[name].scores > cases[name].score_thr).sum())
        assert n_valid > 4096 and 100 < len(keep[name]) < n_valid, (name, n_valid, len(keep[name]))
    za = cases["zero_area_and_flipped"]
    empty = [i for i in range(100) if (za.boxes[i, 2] - za.boxes[i, 0]) * (za.boxes[i, 3] - za.boxes[i, 1]) == 0]
    assert len(empty) >= 20 and set(empty) <= set(keep["zero_area_and_flipped"]) and len(keep["zero_area_and_flipped"]) < 100


@pytest.mark.gpu
@pytest.mark.parametrize("name", NMS_NAMES)
def test_nms_exact(torch_mod, name):
    torch = torch_mod
    from glomeruli_segmentation_amd import _lib
    lib = _lib.load()
    c = nms_cases()[name]
    k = len(c.scores)
    want = do.nms_unsorted(c.boxes, c.scores, c.iou_thr, c.score_thr, c.max_out)
    bd = torch.from_numpy(np.concatenate([c.boxes, np.zeros((1, 4), F32)])).cuda()       # (never an empty allocation)
    sd = torch.from_numpy(np.concatenate([c.scores, np.zeros(1, F32)])).cuda()
    keep = torch.full((max(k, c.max_out) + 1,), -7, dtype=torch.int32, device="cuda")
    nk = torch.full((1,), -7, dtype=torch.int32, device="cuda")
    _lib.check(lib.gs_nms(bd.data_ptr(), sd.data_ptr(), k, ctypes.c_float(c.iou_thr), ctypes.c_float(c.score_thr), c.max_out,
                          keep.data_ptr(), nk.data_ptr(), None))
    torch.cuda.synchronize()
    n = int(nk.item())
    got = keep.cpu().numpy()
    assert n == len(want), (n, len(want))
    assert got[:n].tolist() == want
    assert (got[n:] == -7).all()              # nothing written beyond the count


# ---------------------------------------------------------------------------------------------- 4. the assembled detector
WINDOW_160 = (160, 192)


@lru_cache(maxsize=None)
def det_weights(kind):
    """'random': synthetic_weights(0); 'bias': the same with every weight zeroed (every RPN cell identical: ties everywhere);
    'gradient': bias-only, but rpn.head keeps its weights on the objectness columns; 'border': 'gradient' with rpn.conv's
    weights too, so that the cells on the map's border (whose 3x3 windows reach into the zero padding) differ from the
    tied interior"""
    from glomeruli_segmentation_amd.detector import synthetic_weights
    sd = synthetic_weights(0)
    if kind == "random":
        return sd
    full = sd
    sd = {k: (np.zeros_like(v) if k.endswith(".weight") else v) for k, v in full.items()}
    if kind in ("gradient", "border"):
        sd["rpn.head.weight"][..., :2 * do.A] = full["rpn.head.weight"][..., :2 * do.A]
    if kind == "border":
        sd["rpn.conv.weight"] = full["rpn.conv.weight"]
    assert kind in ("bias", "gradient", "border")
    return sd


@lru_cache(maxsize=None)
def det_window(H, W):
    rng = np.random.default_rng(11 + 1000 * H + W)
    img = rng.integers(0, 256, (1, H, W, 3), dtype=np.uint8)
    img[0, H // 4:3 * H // 4, W // 4:3 * W // 4] = (img[0, H // 4:3 * H // 4, W // 4:3 * W // 4] // 4 + 180).astype(np.uint8)   # some structure
    return img


@lru_cache(maxsize=None)
def det_dense_reference(kind, H, W):
    """the oracle's backbone and RPN of the case's window, computed once per (weights, window)"""
    import torch
    sd = det_weights(kind)
    with torch.no_grad():
        feats = do.backbone(det_window(H, W), sd)
        r = do.rpn(feats, sd)
    return feats.permute(0, 2, 3, 1).contiguous().numpy(), r.permute(0, 2, 3, 1).contiguous().numpy()


def check_detector_stages(out, kind, H, W, rpn_iou, det_iou, score_thr, image=0):
    """one image of a forward's taps and outputs, stage by stage against the oracle run on the GPU's own previous tap (the
    way test_detector_small_against_oracle does) -> what the stages saw, for the case's own asserts"""
    sd = det_weights(kind)
    i = image
    f_ref, r_ref = det_dense_reference(kind, H, W)
    assert out["features"].shape[1:] == f_ref.shape[1:] and out["rpn"].shape[1:] == r_ref.shape[1:]
    assert np.abs(out["features"][i] - f_ref[0]).max() <= 1e-4 * max(1.0, np.abs(f_ref).max())
    assert np.abs(out["rpn"][i] - r_ref[0]).max() <= 1e-4 * max(1.0, np.abs(r_ref).max())
    # RPN selection: input condition first (the decisions the oracle's NMS takes must not hang on a rounding) ...
    cand, csc, cidx = do.rpn_candidates(out["rpn"][i], H, W)
    near1 = do.nms_near_threshold(cand, csc, rpn_iou, 0.0, do.PROPOSALS, 1e-4)
    assert near1 <= 2, "input condition: %d RPN pairs within 1e-4 of IoU %g" % (near1, rpn_iou)
    prop, nv = do.proposals_from_rpn(out["rpn"][i], H, W, rpn_iou)
    got_nv = int((np.abs(out["proposals"][i]).sum(1) > 0).sum())
    assert got_nv == nv, (got_nv, nv)
    assert not out["proposals"][i][nv:].any()
    assert np.abs(out["proposals"][i] - prop).max() <= 2e-3
    # ... box head on the GPU's features and proposals
    got_head = out["head"][i * do.PROPOSALS:(i + 1) * do.PROPOSALS]
    if nv:                                   # (the padding rows are never detected: their head output is not compared)
        head = do.box_head(out["features"][i], out["proposals"][i][:nv], H, W, sd)
        assert np.abs(got_head[:nv] - head).max() <= 2e-4 * max(1.0, np.abs(head).max())
    # ... detections from the GPU's head
    hb, hsc, hidx = do.head_candidates(got_head, out["proposals"][i], nv, H, W)
    near2 = do.nms_near_threshold(hb, hsc, det_iou, score_thr, do.MAX_DET, 1e-4)
    assert near2 <= 2, "input condition: %d detection pairs within 1e-4 of IoU %g" % (near2, det_iou)
    b, s, c, k, kept = do.detections_from_head(got_head, out["proposals"][i], nv, H, W, det_iou, score_thr, with_index=True)
    assert int(out["num"][i]) == k and out["num"][i] == k, (out["num"][i], k)
    assert np.array_equal(out["classes"][i], c)
    assert np.abs(out["scores"][i] - s).max() <= 1e-6
    assert np.abs(out["boxes"][i] - b).max() <= 1e-5
    assert not out["scores"][i][k:].any() and not out["classes"][i][k:].any() and not out["boxes"][i][k:].any()
    # how many each NMS would keep without its cap (whether a full list was truncated)
    rpn_survivors = len(do.nms_sorted(cand, csc, F32(rpn_iou), F32(0), 1 << 30)) if nv == do.PROPOSALS else nv
    det_survivors = len(do.nms_sorted(hb, hsc, F32(det_iou), F32(score_thr), 1 << 30)) if k == do.MAX_DET else k
    return {"anchors": out["rpn"][i].shape[0] * out["rpn"][i].shape[1] * do.A, "rpn_scores": csc, "rpn_index": cidx,
            "n_proposals": nv, "head_scores": hsc, "head_index": hidx, "num": k, "kept": kept, "det_scores": s,
            "n_head_valid": int((hsc > F32(score_thr)).sum()), "rpn_survivors": rpn_survivors, "det_survivors": det_survivors}


def run_detector(torch, kind, H, W, rpn_iou=0.7, det_iou=0.6, score_thr=0.0, batch=1):
    from glomeruli_segmentation_amd.detector import FrcnnDetector
    det = FrcnnDetector(det_weights(kind), rpn_nms_iou=rpn_iou, det_nms_iou=det_iou, score_threshold=score_thr)
    imgs = np.ascontiguousarray(np.repeat(det_window(H, W), batch, axis=0))
    out = {k: v.cpu().numpy() for k, v in det.forward_device(torch.from_numpy(imgs).cuda(), taps=True).items()}
    det.close()
    return out


def detection_proposal_index(out, H, W, image=0):
    """the proposal every GPU detection came from, read back through the GPU's own `proposals` and `head` taps"""
    got_head = out["head"][image * do.PROPOSALS:(image + 1) * do.PROPOSALS]
    boxes = do.decode_clip(out["proposals"][image], got_head[:, 2:], H, W) / np.array([H, W, H, W], dtype=F32)
    nv = int((np.abs(out["proposals"][image]).sum(1) > 0).sum())
    idx = []
    for j in range(int(out["num"][image])):
        d = np.abs(boxes[:nv] - out["boxes"][image][j]).max(1)
        hit = np.flatnonzero(d <= 1e-5)
        assert len(hit) == 1, (j, hit)
        idx.append(int(hit[0]))
    return idx


def assert_batch_is_the_single_window(torch, kind, H, W, single):
    """the same window three times in one batch: every image's taps and outputs are the single-window run's, bit for bit"""
    out3 = run_detector(torch, kind, H, W, batch=3)
    P = do.PROPOSALS
    for key, v in single.items():
        for i in range(3):
            part = out3[key][i * P:(i + 1) * P] if key == "head" else out3[key][i]
            want = v[:P] if key == "head" else v[0]
            assert np.array_equal(part, want), (key, i)


def test_bias_only_weights_tie_and_their_nms_is_clean():
    """what the tie cases rest on, from the oracle alone (a convolution with zero weights is its bias on any implementation,
    so these are the GPU's inputs too): 1 440 anchors with 12 distinct scores, a top-1024 cut inside a tie group, one score
    shared by every detection, and no NMS decision of either stage within 1e-4 of the default thresholds 0.7 / 0.6"""
    H, W = WINDOW_160
    sd = det_weights("bias")
    ref = do.detect(det_window(H, W), sd)
    cand, csc, cidx = do.rpn_candidates(ref["rpn"][0], H, W)
    cls = ref["rpn"][0][:, :, :2 * do.A].reshape(-1, 2)
    full = np.sort((F32(1) / (F32(1) + np.exp(cls[:, 0] - cls[:, 1]))).astype(F32))[::-1]      # every anchor's objectness
    assert len(full) == 1440 and len(np.unique(full)) == 12
    assert full[1023] == full[1024] and int((full == full[1023]).sum()) == 120      # the cut falls inside a 120-way tie
    assert (np.diff(cidx[csc == csc[-1]]) > 0).all()                               # ... and takes its lowest indices
    assert do.nms_near_threshold(cand, csc, 0.7, 0.0, do.PROPOSALS, 1e-4) == 0
    nv = int((np.abs(ref["proposals"][0]).sum(1) > 0).sum())
    hb, hsc, hidx = do.head_candidates(ref["head"][0], ref["proposals"][0], nv, H, W)
    assert do.nms_near_threshold(hb, hsc, 0.6, 0.0, do.MAX_DET, 1e-4) == 0
    assert 100 < nv < 300 and ref["num"][0] == 100 and len(np.unique(ref["scores"][0])) == 1
    print("bias-only 160x192: %d proposals, %d detections, score %.6f" % (nv, ref["num"][0], ref["scores"][0][0]))


@pytest.mark.gpu
def test_detector_ties(torch_mod):
    """bias-only weights: the top-1024 cut inside a 120-way tie, 100 detections sharing one score, tie order = lower index;
    and the window three times in a batch"""
    H, W = WINDOW_160
    out = run_detector(torch_mod, "bias", H, W)
    seen = check_detector_stages(out, "bias", H, W, 0.7, 0.6, 0.0)
    assert seen["anchors"] == 1440 and int((seen["rpn_scores"] == seen["rpn_scores"][-1]).sum()) < 120
    assert seen["num"] == 100 and len(np.unique(seen["det_scores"])) == 1 and len(np.unique(seen["head_scores"][:seen["n_proposals"]])) == 1
    # every score is tied, so the detections are the NMS survivors in proposal order: index for index the oracle's
    assert detection_proposal_index(out, H, W) == seen["kept"].tolist() == sorted(seen["kept"].tolist())
    assert_batch_is_the_single_window(torch_mod, "bias", H, W, out)


@pytest.mark.gpu
@pytest.mark.parametrize("kind", ["gradient", "border"])
def test_detector_partial_ties(torch_mod, kind):
    """'gradient' (bias-only plus the objectness columns of rpn.head): other tie groups, another cut; 'border': the map's
    border cells carry distinct scores around a tied interior, so the top-k sorts tie groups mixed with distinct scores"""
    H, W = WINDOW_160
    out = run_detector(torch_mod, kind, H, W)
    seen = check_detector_stages(out, kind, H, W, 0.7, 0.6, 0.0)
    sc = seen["rpn_scores"]
    groups = np.unique(sc, return_counts=True)[1]
    assert (groups > 1).any()
    if kind == "border":
        assert (groups == 1).sum() >= 10 and (groups >= 10).any()
    for v in np.unique(sc):                                       # the order the proposals above were held to: inside a tie
        assert (np.diff(seen["rpn_index"][sc == v]) > 0).all()    # group, lower anchor index first
    assert detection_proposal_index(out, H, W) == seen["kept"].tolist()


@pytest.mark.gpu
@pytest.mark.parametrize("kind,H,W", [("random", 32, 32), ("bias", 32, 32), ("random", 48, 80), ("bias", 48, 80)])
def test_detector_few_anchors(torch_mod, kind, H, W):
    """fewer anchors than the top-k keeps (n_per < K in both top-k kernels, the -1 tails, the ai < 0 decode), fewer than 300
    proposals, a handful of detections; and the window three times in a batch"""
    out = run_detector(torch_mod, kind, H, W)
    seen = check_detector_stages(out, kind, H, W, 0.7, 0.6, 0.0)
    assert seen["anchors"] == {32: 48, 48: 180}[H] and len(seen["rpn_scores"]) == seen["anchors"] < do.PRE_NMS
    assert 0 < seen["num"] <= seen["n_proposals"] < 100
    assert_batch_is_the_single_window(torch_mod, kind, H, W, out)


@pytest.mark.gpu
@pytest.mark.parametrize("H,W", [(33, 47), (50, 37), (61, 95)])
def test_detector_odd_sizes(torch_mod, H, W):
    """odd heights and widths: the zero padding of the odd edge in the preprocessing, odd h2 / h4 / h8 in the max-pool and
    the stride-2 layers"""
    out = run_detector(torch_mod, "random", H, W)
    seen = check_detector_stages(out, "random", H, W, 0.7, 0.6, 0.0)
    assert seen["num"] > 0


@pytest.mark.gpu
def test_detector_nothing_suppressed(torch_mod):
    """IoU thresholds 0.99: more than 300 RPN survivors truncated to the first 300, more than 100 detections truncated"""
    H, W = WINDOW_160
    out = run_detector(torch_mod, "random", H, W, 0.99, 0.99, 0.0)
    seen = check_detector_stages(out, "random", H, W, 0.99, 0.99, 0.0)
    assert seen["n_proposals"] == 300 and seen["rpn_survivors"] > 300 and seen["num"] == 100 and seen["det_survivors"] > 100


@pytest.mark.gpu
def test_detector_heavy_suppression(torch_mod):
    """IoU thresholds 0.05: long walks across the mask words, few survivors"""
    H, W = WINDOW_160
    out = run_detector(torch_mod, "random", H, W, 0.05, 0.05, 0.0)
    seen = check_detector_stages(out, "random", H, W, 0.05, 0.05, 0.0)
    assert 0 < seen["num"] <= seen["n_proposals"] < 64


@pytest.mark.gpu
def test_detector_score_thresholds(torch_mod):
    """a score threshold above every score: num == 0 and all outputs zero; and one between the two middle scores of the
    default run: a valid count below 100 that is no multiple of 64"""
    H, W = WINDOW_160
    out = run_detector(torch_mod, "random", H, W, 0.7, 0.6, 0.9999)
    seen = check_detector_stages(out, "random", H, W, 0.7, 0.6, 0.9999)
    assert seen["num"] == 0 and seen["n_head_valid"] == 0 and out["num"][0] == 0
    assert not out["boxes"].any() and not out["scores"].any() and not out["classes"].any()
    # the head scores do not depend on the score threshold: take the middle of them from this run
    sc = seen["head_scores"][:seen["n_proposals"]]                 # descending
    m = len(sc) // 2
    while not (sc[m - 1] - sc[m] > 1e-5 and m % 64 and m < 100):    # a gap the two sigmoids cannot disagree about
        m -= 1
    thr = float(F32(0.5) * (sc[m - 1] + sc[m]))
    out = run_detector(torch_mod, "random", H, W, 0.7, 0.6, thr)
    seen = check_detector_stages(out, "random", H, W, 0.7, 0.6, thr)
    assert seen["n_head_valid"] == m and 0 < seen["num"] <= m < 100 and m % 64


# ---------------------------------------------------------------------------------------------- 5. the host entry
@pytest.mark.gpu
@pytest.mark.parametrize("pinned", [False, True])
def test_detect_host_is_forward_device(torch_mod, pinned):
    """one detector through a sequence of calls: slots made for a larger batch reused by smaller ones, a ragged last batch,
    batch > n, then another window size; pageable numpy windows and pinned CPU tensors"""
    torch = torch_mod
    from glomeruli_segmentation_amd.detector import FrcnnDetector
    det = FrcnnDetector(det_weights("random"))
    rng = np.random.default_rng(21)
    for (H, W, n, batches) in ((96, 128, 5, (16, 2, 5, 1)), (64, 160, 3, (2,))):
        wins = rng.integers(0, 256, (n, H, W, 3), dtype=np.uint8)
        wins[:, H // 4:H // 2, W // 4:W // 2] //= 3
        want = det.forward_device(torch.from_numpy(wins).cuda())
        want = {k: v.cpu().numpy() for k, v in want.items()}
        assert (want["num"] > 0).all()
        if pinned:
            host = [torch.from_numpy(w.copy()).pin_memory() for w in wins]
            assert all(t.is_pinned() for t in host)
        else:
            host = [w.copy() for w in wins]
        for batch in batches:
            boxes, scores, classes, num = det.detect_host(host, batch=batch)
            for key, got in (("boxes", boxes), ("scores", scores), ("classes", classes), ("num", num)):
                assert np.array_equal(got, want[key]), (H, W, batch, key)
    det.close()
