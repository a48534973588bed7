#!/usr/bin/env python3
"""Golden class map of the five-fold ESPNet-C ENSEMBLE (the build's own definition, DESIGN.md section 2, extended to --modelType 2).

Runs only in the build container (imports /root/reference/module/espnet/test/Model.py).  The reference has no ensemble code; what
it has is the member: `ESPNet_Encoder(5, 2, 8)` built from the `encoder.*` keys of each fold's .pth and its
`Upsample(scale_factor=8, mode='bilinear')` (VisualizeResults_iou.py:258-261).  This script runs the five fp32 encoders on torch CPU,
each on the tile normalised with its own fold's mean/std, and then the definition in float64:

    v_k[c]  = x8 bilinear upsampling (align_corners=False) of member k's 1/8-scale logits
    p_k     = softmax_c(v_k)               P = mean_k p_k               class = first maximum of P

for glomeruli_segmentation_amd.synth.synth_tile(14, 512, 1024, blobs=3), and records (arrays only):

    mask    the class map, uint8 [512, 1024]
    edge    packed bits [512 * 1024]: pixels whose float64 top-2 margin of P is < 1e-3 (the convention of ensemble.npz): a build
            may differ from `mask` on such pixels only
    seed    (seed, height, width, blobs) of the tile

The edge set of this tile is 778 of 524 288 pixels (1.5e-3); asserted <= 2e-3 below.  (Seed 0 with six blobs gives 5.7e-3.)

Known: the mean of the five encoders yields only TWO classes on this tile, and only background on small synth tiles (the encoders
alone are weak segmenters and disagree where one of them sees a third class).  Multi-class coverage of the ensemble head therefore
comes from the random-weight cases of tests/test_espnet_c_ensemble.py, not from this fixture.

    python tests/golden/make_golden_espnet_c_ensemble.py        ->  tests/golden/espnet_c_ensemble.npz
"""
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(os.path.dirname(HERE))
REF = os.environ.get("GS_REFERENCE", "/root/reference")
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.join(REF, "module", "espnet", "test"))

import Model as RefModel  # noqa: E402  (the reference's Model.py)
from glomeruli_segmentation_amd.synth import FOLD_MEAN_STD, synth_tile  # noqa: E402

EDGE = 1e-3
MAX_EDGE_FRACTION = 2e-3
TILE = (14, 512, 1024, 3)      # (seed, height, width, blobs)


def upsample64(lg):
    """float64 bilinear x8 of [C, h, w] (align_corners=False: half-pixel centres, edge taps clamped)"""
    lg = lg.astype(np.float64)

    def taps(n):
        s = np.maximum((np.arange(8 * n) + 0.5) / 8.0 - 0.5, 0.0)
        i0 = np.floor(s).astype(int)
        return i0, np.minimum(i0 + 1, n - 1), s - i0
    y0, y1, wy = taps(lg.shape[1])
    x0, x1, wx = taps(lg.shape[2])
    top = lg[:, y0][:, :, x0] * (1 - wx) + lg[:, y0][:, :, x1] * wx
    bot = lg[:, y1][:, :, x0] * (1 - wx) + lg[:, y1][:, :, x1] * wx
    return top * (1 - wy)[None, :, None] + bot * wy[None, :, None]


def preprocess(tile_u8, mean, std):
    """VisualizeResults_iou.py:107-119 (BGR order kept, no channel swap)."""
    img = tile_u8.astype(np.float32)
    for j in range(3):
        img[:, :, j] -= mean[j]
    for j in range(3):
        img[:, :, j] /= std[j]
    img /= 255
    return torch.from_numpy(np.ascontiguousarray(img.transpose((2, 0, 1)))).unsqueeze(0)


def main():
    torch.set_grad_enabled(False)
    seed, h, w, blobs = TILE
    tile = synth_tile(seed, h, w, blobs=blobs)
    P = np.zeros((5, h, w), dtype=np.float64)
    for fold in range(1, 6):
        sd = torch.load(os.path.join(REF, "models", "espnet_fold%d.pth" % fold), map_location="cpu")
        enc = RefModel.ESPNet_Encoder(5, 2, 8)                                    # :258
        msg = enc.load_state_dict({k[len("encoder."):]: v for k, v in sd.items() if k.startswith("encoder.")})
        assert not msg.missing_keys and not msg.unexpected_keys, msg
        enc.eval()
        mean, std = FOLD_MEAN_STD[fold]
        v = upsample64(enc(preprocess(tile, mean, std))[0].numpy())
        e = np.exp(v - v.max(0, keepdims=True))
        P += e / e.sum(0, keepdims=True) * (1.0 / 5.0)
    mask = P.argmax(0).astype(np.uint8)
    top2 = np.sort(P, axis=0)[-2:]
    edge = (top2[1] - top2[0]) < EDGE
    counts = np.bincount(mask.ravel(), minlength=5)
    print("seed %d %dx%d: counts %s; edge set %d of %d pixels (%.2g)" % (seed, h, w, counts.tolist(), int(edge.sum()), edge.size, edge.mean()))
    assert edge.mean() <= MAX_EDGE_FRACTION
    path = os.path.join(HERE, "espnet_c_ensemble.npz")
    np.savez_compressed(path, mask=mask, edge=np.packbits(edge.ravel()), seed=np.array([seed, h, w, blobs]))
    print("espnet_c_ensemble.npz %.1f KB" % (os.path.getsize(path) / 1024.0))


if __name__ == "__main__":
    main()
