#!/usr/bin/env python3
"""Golden class maps of the REFERENCE's ESPNet-C path (--modelType 2, VisualizeResults_iou.py:125-128,258-272).

Runs only in the build container (imports /root/reference/module/espnet/test/Model.py).  Builds the reference's
`ESPNet_Encoder(5, 2, 8)` with the fold-1 encoder weights and its `up = torch.nn.Upsample(scale_factor=8, mode='bilinear')`,
and records on torch CPU (the reference's default device, --gpu_id -1), for two seeded 512 x 1024 synth tiles and one
136 x 264 tile (17 x 33 at 1/8 scale: both odd):

    logits_K   the encoder's 1/8-scale logits, fp32 [5, H/8, W/8]
    mask_K     up(img_out)[0].max(0)[1] as uint8 [H, W]                                   (:125-128)
    margin_K   packed bits [H * W]: pixels whose float64 top-2 margin -- of the float64 bilinear upsampling of logits_K --
               is <= MARGIN.  A build whose 1/8 logits are within LOGIT_TOL = 5e-5 of the reference's may differ from
               mask_K on such pixels only (the upsampling is a convex combination: every upsampled logit inherits at most
               LOGIT_TOL, a difference of two at most 2 * LOGIT_TOL = MARGIN).
    seed_K / size_K   the tile is glomeruli_segmentation_amd.synth.synth_tile(seed, height, width, blobs)

The seeds and blob counts are chosen so that every full-size class map holds at least three classes AND the margin set holds
at most 1e-4 of the tile's pixels (both asserted below).  The twelve-blob tiles of the other fixtures have too much class
boundary for the second condition: 56 to 281 of 524 288 pixels (1.1e-4 to 5.4e-4) over seeds 0..39, so these tiles have
three and six blobs.

    python tests/golden/make_golden_espnet_c.py        ->  tests/golden/espnet_c.npz (arrays only)
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

MARGIN = 1e-4                    # 2 * LOGIT_TOL (tests/test_gpu_parity.py)
MAX_MARGIN_FRACTION = 1e-4
# (seed, height, width, blobs)
TILES = [(14, 512, 1024, 3), (0, 512, 1024, 6), (27, 136, 264, 6)]


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
    sd = torch.load(os.path.join(REF, "models", "espnet_fold1.pth"), map_location="cpu")
    enc = RefModel.ESPNet_Encoder(5, 2, 8)                                        # :258
    msg = enc.load_state_dict({k[len("encoder."):]: v for k, v in sd.items() if k.startswith("encoder.")})
    assert not msg.missing_keys and not msg.unexpected_keys, msg
    enc.eval()
    up = torch.nn.Upsample(scale_factor=8, mode='bilinear')                       # :259-261
    mean, std = FOLD_MEAN_STD[1]
    out = {"margin": np.float64(MARGIN)}
    for k, (seed, h, w, blobs) in enumerate(TILES):
        tile = synth_tile(seed, h, w, blobs=blobs)
        lg = enc(preprocess(tile, mean, std))                                     # :123
        mask = up(lg)[0].max(0)[1].byte().numpy()                                 # :125-128
        present = np.flatnonzero(np.bincount(mask.ravel(), minlength=5))
        print("tile %d seed %d %dx%d: classes %s counts %s" % (k, seed, h, w, present.tolist(), np.bincount(mask.ravel(), minlength=5).tolist()))
        if (h, w) == (512, 1024):
            assert len(present) >= 3, "seed %d: the class map holds %d classes" % (seed, len(present))
        v = upsample64(lg[0].numpy())
        top2 = np.sort(v, axis=0)[-2:]
        edge = (top2[1] - top2[0]) <= MARGIN
        print("   margin set: %d of %d pixels; outside it the float64 argmax differs from the map on %d" % (
            int(edge.sum()), edge.size, int(((v.argmax(0) != mask) & ~edge).sum())))
        assert edge.mean() <= MAX_MARGIN_FRACTION
        assert not ((v.argmax(0) != mask) & ~edge).any()
        out["logits_%d" % k] = lg[0].numpy()
        out["mask_%d" % k] = mask
        out["margin_%d" % k] = np.packbits(edge.ravel())
        out["seed_%d" % k] = np.array([seed, h, w, blobs])
    path = os.path.join(HERE, "espnet_c.npz")
    np.savez_compressed(path, **out)
    print("espnet_c.npz %.1f KB" % (os.path.getsize(path) / 1024.0))


if __name__ == "__main__":
    main()
