"""The boundary test of csrc/boundary_links.h and the two row passes that link a row's pixels to it, seen through the three entries
built on them: gs_rim_classes (lesions.hip), gs_foreign_dist (zones.hip) and gs_instance_boundary_dist (boundary_dist.hip) must
agree with ONE definition of a boundary pixel, helpers.instance_maps.boundary_mask, on the shapes where a row pass can go wrong: a
width of one lane, one below, at and above a chunk of 64, one below, at and above a round of 256, two rounds and one; a single
row, two rows, five.

The maps are raw label maps (as outlines_ref.raw_labels are, not label_instances' output): random int32 values in -2 .. N + 2, of
which only 1..N are instances.  Every comparison is exact.  A map of 1 x 1 cannot hold two instances: there the map is the
hand-made [[1]], and the one statement that needs a second instance -- near_d2 >= 0 on every boundary pixel -- is the checker's
alone (no pixel has a foreign one, near_d2 is -1 throughout)."""
import ctypes
import functools

import numpy as np
import pytest

from helpers import zones_ref as zr
from helpers.instance_maps import boundary_mask

pytestmark = pytest.mark.gpu

N = 3
CLASS, CLASSES = 2, 5
WIDTHS = (1, 63, 64, 65, 255, 256, 257, 513)
HEIGHTS = (1, 2, 5)
SENTINEL = -77


def _valid(lab):
    return np.unique(lab[(lab >= 1) & (lab <= N)])


@functools.lru_cache(maxsize=None)
def label_map(h, w):
    """-> a read-only int32 [h,w] map with values in -2 .. N + 2 and at least two distinct labels of 1..N: the first seed that gives
    them; [[1]] for the one pixel"""
    if h * w == 1:
        lab = np.ones((1, 1), dtype=np.int32)
    else:
        for seed in range(64):
            lab = np.random.default_rng(seed).integers(-2, N + 3, (h, w)).astype(np.int32)
            if len(_valid(lab)) >= 2:
                break
    lab.setflags(write=False)
    return lab


def _device():
    import torch
    return torch, torch.device("cuda", 0)


def _stream(torch, dev):
    return ctypes.c_void_p(torch.cuda.current_stream(dev).cuda_stream)


def run_rim(lab):
    from glomeruli_segmentation_amd import lesions
    torch, dev = _device()
    h, w = lab.shape
    d_lab = torch.from_numpy(np.array(lab)).to(dev)
    d_cm = torch.full((h, w), CLASS, dtype=torch.uint8, device=dev)
    out = torch.full((h, w), SENTINEL, dtype=torch.int32, device=dev)
    with torch.cuda.device(dev):
        status = lesions.load().gs_rim_classes(d_lab.data_ptr(), d_cm.data_ptr(), N, CLASSES, h, w, 0, out.data_ptr(), _stream(torch, dev))
        torch.cuda.synchronize()
    assert status == 0
    return out.cpu().numpy()


def run_foreign(lab):
    from glomeruli_segmentation_amd import zones
    torch, dev = _device()
    h, w = lab.shape
    d_lab = torch.from_numpy(np.array(lab)).to(dev)
    ws = torch.full((zones.foreign_workspace_bytes(h, w),), 0xA5, dtype=torch.uint8, device=dev)
    near_d2 = torch.full((h, w), SENTINEL, dtype=torch.int32, device=dev)
    near_id = torch.full((h, w), SENTINEL, dtype=torch.int32, device=dev)
    with torch.cuda.device(dev):
        status = zones.load().gs_foreign_dist(d_lab.data_ptr(), N, h, w, 2 ** 30, ws.data_ptr(), ws.numel(), near_d2.data_ptr(),
                                              near_id.data_ptr(), _stream(torch, dev))
        torch.cuda.synchronize()
    assert status == 0
    return near_d2.cpu().numpy(), near_id.cpu().numpy()


def run_boundary_dist(lab):
    """the map as both sides, every instance matched with itself -> dist_gt"""
    from glomeruli_segmentation_amd import _lib, instance_eval
    torch, dev = _device()
    h, w = lab.shape
    d_lab = torch.from_numpy(np.array(lab)).to(dev)
    match = torch.arange(1, N + 1, dtype=torch.int32, device=dev)
    ws = torch.full((instance_eval.boundary_workspace_bytes(h, w),), 0xA5, dtype=torch.uint8, device=dev)
    dist_gt = torch.full((h, w), SENTINEL, dtype=torch.int32, device=dev)
    stats = torch.empty((N, 2, 3), dtype=torch.int64, device=dev)
    with torch.cuda.device(dev):
        status = _lib.load().gs_instance_boundary_dist(d_lab.data_ptr(), d_lab.data_ptr(), match.data_ptr(), N, match.data_ptr(), N, h, w,
                                                       ws.data_ptr(), ws.numel(), dist_gt.data_ptr(), None, stats.data_ptr(),
                                                       _stream(torch, dev))
        torch.cuda.synchronize()
    assert status == 0
    return dist_gt.cpu().numpy()


@pytest.mark.parametrize("h", HEIGHTS)
@pytest.mark.parametrize("w", WIDTHS)
def test_three_entries_one_boundary(w, h):
    lab = label_map(h, w)
    assert lab.min() >= -2 and lab.max() <= N + 2 and (len(_valid(lab)) >= 2 or lab.shape == (1, 1))
    mask = boundary_mask(lab, N)
    assert mask.any()

    rim = run_rim(lab)
    assert np.array_equal(rim != 0, mask) and np.array_equal(rim, np.where(mask, 1 << CLASS, 0))

    near_d2, near_id = run_foreign(lab)
    want_d2, want_id = zr.foreign_direct(lab, N, 2 ** 30)
    assert np.array_equal(near_d2, want_d2) and np.array_equal(near_id, want_id)
    assert np.array_equal(near_d2 >= 0, mask if h * w > 1 else np.zeros_like(mask))

    dist_gt = run_boundary_dist(lab)
    assert np.array_equal(dist_gt == 0, mask) and np.array_equal(dist_gt, np.where(mask, 0, -1))
