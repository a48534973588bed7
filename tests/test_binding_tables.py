"""The Python binding's tables (_lib.HEADERS: one prototype table per public header) and the call plumbing the wrappers share
(_call.py).  Host-only except the one refusal of a GPU tensor."""
import ctypes
import glob
import os

import numpy as np
import pytest

from conftest import REPO
from glomeruli_segmentation_amd import _call, _lib, engine, instance_eval, instances, split

OPTIONAL = {"glomseg_plan.h", "glomseg_lean.h", "glomseg_workspace.h", "glomseg_forms.h", "glomseg_detector_steps.h"}


def test_one_table_per_header():
    on_disk = sorted(os.path.basename(p) for p in glob.glob(os.path.join(REPO, "include", "*.h")))
    assert sorted(_lib.HEADERS) == on_disk and len(on_disk) == 12
    tables = list(_lib.HEADERS.values())
    assert len({id(t) for t in tables}) == len(tables)
    names = [name for t in tables for name in t]
    assert len(names) == len(set(names))                              # no symbol is in two tables
    assert _lib.OPTIONAL_HEADERS == OPTIONAL and _lib.OPTIONAL_HEADERS <= set(_lib.HEADERS)
    by_name = {k: v for k, v in vars(_lib).items() if k.endswith("PROTOTYPES")}
    assert {id(t) for t in by_name.values()} == {id(t) for t in tables}      # every *_PROTOTYPES is some header's table


def test_load_binds_every_symbol_of_every_table():
    lib = _lib.load()
    for header, table in _lib.HEADERS.items():
        for name, (res, args) in table.items():
            fn = getattr(lib, name)
            assert fn.restype is res and fn.argtypes == args, (header, name)


def _direct(fn, *ints):
    need = ctypes.c_size_t(0)
    assert fn(*ints, ctypes.byref(need)) == _lib.GS_OK
    return need.value


@pytest.mark.parametrize("entry,ints,public", [
    ("gs_instances_plan", (37, 53, 5, 100), lambda: instances.workspace_bytes(37, 53, 5, 100)),
    ("gs_morphometry_plan", (37, 53, 91), lambda: instances.morphometry_workspace_bytes(37, 53, 91)),
    ("gs_instance_match_plan", (37, 53, 77), lambda: instance_eval.workspace_bytes(37, 53, 77)),
    ("gs_boundary_dist_plan", (37, 53), lambda: instance_eval.boundary_workspace_bytes(37, 53)),
    ("gs_espnet_workspace_plan", (2, 64, 128, 2, 8, 5, 0), lambda: engine.workspace_bytes(2, 64, 128, 2, 8, 5)),
    ("gs_edt_plan", (37, 53), lambda: split.edt_workspace_bytes(37, 53)),
    ("gs_label_peaks_plan", (19,), lambda: split.peaks_workspace_bytes(19)),
    ("gs_split_plan", (37, 53, 19, 7), lambda: split.split_workspace_bytes(37, 53, 19, 7)),
])
def test_planned_bytes_is_the_plan_entry(entry, ints, public):
    fn = getattr(_lib.load(), entry)
    want = _direct(fn, *ints)
    assert want > 0 and _call.planned_bytes(fn, *ints) == want == public()


def test_planned_bytes_refusal_raises():
    with pytest.raises(_lib.GlomsegError) as e:
        _call.planned_bytes(_lib.load().gs_edt_plan, -1, 8)
    assert e.value.status == 1 and _lib.STATUS_NAMES[1] == "GS_ERR_INVALID"
    with pytest.raises(_lib.GlomsegError):
        split.edt_workspace_bytes(-1, 8)


def test_packed_slots():
    sizes = [1, 255, 256, 257, 0]
    shapes = [(1,), (5, 51), (16, 16), (257, 1), (0, 3)]
    import torch
    buf, offsets, ptrs = _call.packed_pinned(sizes, pin=False)
    assert not buf.is_pinned() and buf.dtype == torch.uint8 and buf.dim() == 1
    assert offsets.tolist() == [0, 256, 512, 768, 1280, 1280]
    starts = offsets[:-1]
    assert all(int(o) % 256 == 0 for o in offsets) and all(a < b for a, b in zip(starts[:-1], starts[1:]))
    assert int(offsets[-1]) == buf.numel()                            # the last offset is the buffer length
    assert [p for p in ptrs] == [buf.data_ptr() + int(o) for o in starts]
    views = _call.packed_views(buf, offsets, shapes)
    base = buf.data_ptr()
    spans = []
    for v, s, o, size in zip(views, shapes, starts, sizes):
        assert v.shape == s and v.dtype == np.uint8 and v.size == size and v.flags.c_contiguous
        assert v.size == 0 or v.ctypes.data == base + int(o)
        spans.append((int(o), int(o) + v.size))
    assert all(a[1] <= b[0] for a, b in zip(spans[:-1], spans[1:]))   # no view reaches into the next slot
    buf.zero_()
    for k, v in enumerate(views):
        v[...] = k + 1                                                # views, not copies: the buffer sees every write ...
    flat = buf.numpy()
    for k, (lo, hi) in enumerate(spans):
        assert (flat[lo:hi] == k + 1).all()                           # ... and no write landed in another view
    assert int(flat.astype(np.int64).sum()) == sum((k + 1) * n for k, n in enumerate(sizes))


def test_host_image_ptrs():
    import torch
    rng = np.random.default_rng(0)
    a = rng.integers(0, 256, (5, 7, 3), dtype=np.uint8)
    t = torch.from_numpy(rng.integers(0, 256, (4, 6, 3), dtype=np.uint8))
    wide = rng.integers(0, 256, (5, 7, 6), dtype=np.uint8)
    strided = wide[:, :, ::2]                                         # uint8 [5,7,3], not contiguous
    assert not strided.flags.c_contiguous
    as_int = a.astype(np.int32)
    ptrs, shapes, keep = _call.host_image_ptrs([a, t, strided, as_int], "crop")
    assert shapes == [(5, 7), (4, 6), (5, 7), (5, 7)] and len(keep) == 4
    assert ptrs[0] == a.ctypes.data and keep[0] is a                  # the address of the data itself, no copy
    assert ptrs[1] == t.data_ptr() and keep[1] is t
    for k, src in ((2, strided), (3, a)):                             # converted: a contiguous uint8 copy, owned by keep
        assert keep[k].flags.c_contiguous and keep[k].dtype == np.uint8 and ptrs[k] == keep[k].ctypes.data
        assert ptrs[k] != src.ctypes.data and np.array_equal(keep[k], src)
    for what, tensor_text, shape_text in (
            ("crop", "crop 1: expected a contiguous uint8 [h,w,3] CPU tensor", "crop 1: expected uint8 [h,w,3]"),
            ("window", "window 1: expected a contiguous uint8 CPU tensor", "window 1: expected uint8 [H,W,3], every window of one size")):
        for bad in (t.to(torch.int32), t.permute(1, 0, 2)):
            with pytest.raises(ValueError) as e:
                _call.host_image_ptrs([a, bad], what)
            assert str(e.value) == tensor_text
        with pytest.raises(ValueError) as e:
            _call.host_image_ptrs([a, a[:, :, 0]], what)
        assert str(e.value) == shape_text
    with pytest.raises(ValueError) as e:
        _call.host_image_ptrs([t[:, :, :2].contiguous()], "crop")
    assert str(e.value) == "crop 0: expected a contiguous uint8 [h,w,3] CPU tensor"
    assert _call.host_image_ptrs([], "window")[1:] == ([], [])


@pytest.mark.gpu
def test_host_image_ptrs_refuses_a_gpu_tensor():
    import torch
    t = torch.zeros((4, 6, 3), dtype=torch.uint8, device="cuda")
    for what, text in (("crop", "crop 0: expected a contiguous uint8 [h,w,3] CPU tensor"),
                       ("window", "window 0: expected a contiguous uint8 CPU tensor")):
        with pytest.raises(ValueError) as e:
            _call.host_image_ptrs([t], what)
        assert str(e.value) == text


def test_mean_std_arrays():
    means, stds = _call.mean_std_arrays([((1, 2, 3), (4, 5, 6)), ((7, 8, 9), (10, 11, 12.5))], 2)
    assert list(means) == [1, 2, 3, 7, 8, 9] and list(stds) == [4, 5, 6, 10, 11, 12.5]
    assert means._type_ is ctypes.c_float and stds._type_ is ctypes.c_float
