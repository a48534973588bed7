"""Plain restatements of the detector's glue steps (csrc/detector.hip), written from the definitions in its comments and from
TF object-detection's formulas; imports nothing from the package and nothing from oracle/.

Each step has a float64 reference (`dtype=np.float64`: every operation in float64 on the float32 inputs) and, where it rounds,
a float32 restatement (`dtype=np.float32`: every operation rounded to float32 on its own).  The float32 forms are used only to
measure how far honest float32 arithmetic lies from float64 (the tests' bounds are multiples of that) and to build the wrong
variants a bound must reject; the GPU is compared with float64 alone.
"""
import numpy as np

A = 12                                   # anchors per cell: scale index a // 3, ratio index a % 3
STRIDE = 16
BASE = 256.0
PROPOSALS = 300
SCALES = (0.25, 0.5, 1.0, 2.0)
RATIOS = (0.5, 1.0, 2.0)                 # height / width = 1 / ratio: ah = s / sqrt(r) * base, aw = s * sqrt(r) * base
LIM = 4.135166556742356                  # log(1000 / 16): the clamp of the scaled size deltas


# ------------------------------------------------------------------------------------------------ preprocess
def preprocess(img, dtype=np.float64, fused=False, bgr=False, edge=0.0):
    """uint8 RGB [n,H,W,3] -> [n,ceil(H/2),ceil(W/2),16]: 2 x / 255 - 1, 2 x 2 space-to-depth with channel (dy*2+dx)*3 + c,
    channels 12..15 zero, positions beyond an odd edge `edge` (the definition: 0).  float32: the constant 2/255 rounded, then
    either product and difference rounded one after the other or (`fused`) the exact product minus one rounded once.
    `bgr`, `edge=-1`: the wrong variants."""
    n, H, W, _ = img.shape
    h2, w2 = (H + 1) // 2, (W + 1) // 2
    x = img[..., ::-1] if bgr else img
    if dtype == np.float64:
        v = 2.0 * x.astype(np.float64) / 255.0 - 1.0
    else:
        c = np.float32(2.0) / np.float32(255.0)
        if fused:
            v = (x.astype(np.float64) * np.float64(c) - 1.0).astype(np.float32)     # (8 x 24 bits: the product is exact in float64)
        else:
            v = (x.astype(np.float32) * c).astype(np.float32) - np.float32(1.0)
    out = np.zeros((n, h2, w2, 16), dtype=dtype)
    out[..., :12] = edge
    for dy in range(2):
        for dx in range(2):
            part = v[:, dy::2, dx::2]
            q = (dy * 2 + dx) * 3
            out[:, :part.shape[1], :part.shape[2], q:q + 3] = part
    return out


# ------------------------------------------------------------------------------------------------ max-pool
def maxpool(x, k, s, pad, pad_value=-np.inf):
    """[n,h,w,c] -> [n,ho,wo,c] float64, window k, stride s, padding `pad` that never wins (-inf); pad_value=0: the wrong variant"""
    n, h, w, c = x.shape
    ho, wo = (h + 2 * pad - k) // s + 1, (w + 2 * pad - k) // s + 1
    xp = np.full((n, h + 2 * pad + k, w + 2 * pad + k, c), pad_value, dtype=np.float64)
    xp[:, pad:pad + h, pad:pad + w] = x
    out = np.full((n, ho, wo, c), -np.inf)
    for ky in range(k):
        for kx in range(k):
            out = np.maximum(out, xp[:, ky:ky + (ho - 1) * s + 1:s, kx:kx + (wo - 1) * s + 1:s])
    return out


# ------------------------------------------------------------------------------------------------ scores
def sigmoid_fg(bg, fg, dtype=np.float64):
    """softmax over (background, foreground), the foreground's share: 1 / (1 + exp(bg - fg))"""
    bg, fg = np.asarray(bg, dtype=dtype), np.asarray(fg, dtype=dtype)
    with np.errstate(over="ignore", under="ignore"):
        return (dtype(1) / (dtype(1) + np.exp(bg - fg))).astype(dtype)


def objectness(rpn, dtype=np.float64, swap=False):
    """rpn [n,cells,6A] (per cell: 2A class logits anchor-major, bg then fg; then 4A deltas) -> [n,cells*A]"""
    cls = rpn[..., :2 * A].reshape(rpn.shape[0], -1, 2)
    return sigmoid_fg(cls[..., 1], cls[..., 0], dtype) if swap else sigmoid_fg(cls[..., 0], cls[..., 1], dtype)


# ------------------------------------------------------------------------------------------------ box decode
def anchor_boxes(idx, hf, wf, dtype=np.float64, cell_mod=None):
    """grid anchors [len(idx),4] (ymin,xmin,ymax,xmax, pixels) of anchor indices idx = cell * A + a, cell = cy * wf + cx:
    centre (cy, cx) * STRIDE, height s / sqrt(r) * BASE, width s * sqrt(r) * BASE.  cell_mod: the wrong variant's divisor."""
    idx = np.asarray(idx, dtype=np.int64)
    a, cell = idx % A, idx // A
    m = wf if cell_mod is None else cell_mod
    cx, cy = cell % m, cell // m
    sc = np.array(SCALES, dtype=dtype)[a // 3]
    rs = np.sqrt(np.array(RATIOS, dtype=np.float64)).astype(dtype)[a % 3]
    ah, aw = (sc / rs * dtype(BASE)).astype(dtype), (sc * rs * dtype(BASE)).astype(dtype)
    yc, xc = (cy * STRIDE).astype(dtype), (cx * STRIDE).astype(dtype)
    half = dtype(0.5)
    return np.stack([yc - half * ah, xc - half * aw, yc + half * ah, xc + half * aw], axis=1).astype(dtype)


def decode_clip(anc, d, H, W, dtype=np.float64, centre_scale=0.1, size_scale=0.2, clip_to=None):
    """faster_rcnn_box_coder with scale factors 10, 10, 5, 5 (deltas ty, tx, th, tw), the scaled size deltas clamped at LIM, the
    corners clipped to [0,H] x [0,W].  min / max ignore a NaN operand, as C's fminf / fmaxf do.  centre_scale / size_scale /
    clip_to: the wrong variants."""
    anc, d = np.asarray(anc, dtype=dtype), np.asarray(d, dtype=dtype)
    half = dtype(0.5)
    Hc, Wc = (dtype(H), dtype(W)) if clip_to is None else (dtype(clip_to[0]), dtype(clip_to[1]))
    with np.errstate(all="ignore"):
        ha, wa = anc[:, 2] - anc[:, 0], anc[:, 3] - anc[:, 1]
        yca, xca = anc[:, 0] + half * ha, anc[:, 1] + half * wa
        th = np.fmin(d[:, 2] * dtype(size_scale), dtype(LIM))
        tw = np.fmin(d[:, 3] * dtype(size_scale), dtype(LIM))
        hh, ww = np.exp(th).astype(dtype) * ha, np.exp(tw).astype(dtype) * wa
        yc = d[:, 0] * dtype(centre_scale) * ha + yca
        xc = d[:, 1] * dtype(centre_scale) * wa + xca
        zero = dtype(0)
        out = np.stack([np.fmin(np.fmax(yc - half * hh, zero), Hc), np.fmin(np.fmax(xc - half * ww, zero), Wc),
                        np.fmin(np.fmax(yc + half * hh, zero), Hc), np.fmin(np.fmax(xc + half * ww, zero), Wc)], axis=1)
    return out.astype(dtype)


def rpn_decode(rpn, sel, hf, wf, H, W, dtype=np.float64, **wrong):
    """rpn [n,hf*wf,6A], sel int [n,K] (anchor index, negative = none) -> [n,K,4]; a `none` row is four zeros"""
    n, K = sel.shape
    out = np.zeros((n, K, 4), dtype=dtype)
    cell_mod = wrong.pop("cell_mod", None)
    for i in range(n):
        ok = sel[i] >= 0
        idx = sel[i][ok]
        deltas = rpn[i][:, 2 * A:].reshape(-1, 4)[idx]                    # [cells*A,4] by anchor index
        out[i][ok] = decode_clip(anchor_boxes(idx, hf, wf, dtype, cell_mod), deltas, H, W, dtype, **wrong)
    return out


def head_decode(head, prop, keep, H, W, dtype=np.float64):
    """head [total,6] = 2 class logits + 4 deltas relative to the proposal; keep < 0 (a padded proposal): score -1
    -> (score [total], boxes [total,4])"""
    score = np.where(keep >= 0, sigmoid_fg(head[:, 0], head[:, 1], dtype), dtype(-1)).astype(dtype)
    return score, decode_clip(prop, head[:, 2:], H, W, dtype)


# ------------------------------------------------------------------------------------------------ proposals
def gather_proposals(boxes, keep, H, W):
    """boxes [n,K,4], keep int [n,P] (position, negative = padding) -> prop [n,P,4] (the boxes' own bits), the float64 quotients
    prop / (H,W,H,W), image index of every row [n*P]"""
    n, P = keep.shape
    prop = np.zeros((n, P, 4), dtype=boxes.dtype)
    for i in range(n):
        ok = keep[i] >= 0
        prop[i][ok] = boxes[i][keep[i][ok]]
    norm = prop.astype(np.float64) / np.array([H, W, H, W], dtype=np.float64)
    return prop, norm, np.repeat(np.arange(n, dtype=np.int32), P)


# ------------------------------------------------------------------------------------------------ pools of the box head
def pool2x2(crops):
    """[b,2m,2m,c] -> [b,m,m,c]: the 2 x 2 / stride-2 max"""
    b, s, _, c = crops.shape
    return crops.reshape(b, s // 2, 2, s // 2, 2, c).max(axis=(2, 4))


def avgpool(x, dtype=np.float64, divisor=None, drop_last=False):
    """[n,hw,c] -> [n,c]: the mean over hw.  float32: summed in index order, then divided.  divisor / drop_last: wrong variants"""
    n, hw, c = x.shape
    div = hw if divisor is None else divisor
    last = hw - 1 if drop_last else hw
    if dtype == np.float64:
        return x[:, :last].astype(np.float64).sum(axis=1) / div
    s = np.zeros((n, c), dtype=np.float32)
    for i in range(last):
        s = (s + x[:, i]).astype(np.float32)
    return (s / np.float32(div)).astype(np.float32)


def avgpool_bound(x):
    """per output: 2^-24 (sum |x_i| + |mean|) (1 + 2^-10): recursive summation in any order errs by at most (hw - 1) u sum|x|,
    divided by hw that is below u sum|x|; the quotient's rounding adds u |mean|; the last factor covers the second-order terms"""
    x64 = x.astype(np.float64)
    return 2.0 ** -24 * (np.abs(x64).sum(axis=1) + np.abs(x64.mean(axis=1))) * (1 + 2.0 ** -10)
