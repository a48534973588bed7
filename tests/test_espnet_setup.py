"""The set-up of an ESPNet handle without a device: the weight packer (csrc/espnet_weights.h through gs_espnet_pack_weights) and the
activation layout (csrc/workspace_plan.h through gs_espnet_workspace_plan).

1. The packed blob and the workspace size are those of the commit before the two headers existed, bit for bit:
   tests/golden/espnet_setup.json was recorded from that commit's own code (tests/golden/make_golden_espnet_setup.py).
2. A few pieces are restated here in numpy, independently of any packer.
3. The structure every kernel relies on: aligned, disjoint pieces, a zero guard, padding planes that stay exact zeros.
4. The refusals of gs_espnet_create and gs_espnet_reserve that need no device.
5. Both headers under AddressSanitizer + UndefinedBehaviorSanitizer in a stand-alone program (tests/helpers/espnet_setup_driver.cpp).
"""
import ctypes
import functools
import hashlib
import json
import os

import numpy as np
import pytest

from conftest import GOLDEN, REPO, load_weights, random_state_dict

from helpers.sanitized_driver import run_sanitized_driver

# (name, p, q, classes, encoder_only); "fold1": tests/golden/weights_fold1.npz, else random_state_dict(p, q, classes, seed=0).
# The padded class counts 4, 5, 8, 12, 16 and 20, p = 0, q = 0, blocks with and without a fused next reduce, both handle kinds.
MODELS = [("p2_q8_c5", 2, 8, 5, False), ("p0_q0_c5", 0, 0, 5, False), ("p1_q1_c5", 1, 1, 5, False), ("p1_q2_c7", 1, 2, 7, False),
          ("p2_q3_c12", 2, 3, 12, False), ("p3_q1_c16", 3, 1, 16, False), ("p2_q3_c20", 2, 3, 20, False), ("p1_q1_c2", 1, 1, 2, False),
          ("p1_q1_c3", 1, 1, 3, False), ("fold1", 2, 8, 5, False), ("p2_q8_c5_encoder", 2, 8, 5, True),
          ("p1_q2_c7_encoder", 1, 2, 7, True)]
SHAPES = [(1, 8, 8), (4, 64, 128), (32, 512, 1024), (1, 4096, 4096)]
WS_MODELS = [("c5_p2", 5, 2, False), ("c5_p0", 5, 0, False), ("c20_p2", 20, 2, False), ("c5_p2_encoder", 5, 2, True)]   # (name, classes, p, encoder_only)
GS_ERR_INVALID, GS_ERR_UNSUPPORTED = 1, 4


def state_dict(name, p, q, classes, encoder_only):
    sd = load_weights(1) if name == "fold1" else random_state_dict(p, q, classes, seed=0)
    if encoder_only:   # ESPNet-C tables: the full net's "encoder." tensors without the prefix (tests/test_espnet_c.py, encoder_sd)
        sd = {k[len("encoder."):]: v for k, v in sd.items() if k.startswith("encoder.")}
    return sd


@functools.lru_cache(maxsize=None)
def packed(name):
    """(state_dict, blob, pieces, classes) of a model of MODELS, packed once"""
    from glomeruli_segmentation_amd.engine import pack_weights
    _, p, q, classes, enc = next(m for m in MODELS if m[0] == name)
    sd = state_dict(name, p, q, classes, enc)
    blob, pieces = pack_weights(sd, classes, p, q, enc)
    blob.setflags(write=False)
    return sd, blob, pieces, classes


@functools.lru_cache(maxsize=None)
def parent():
    with open(os.path.join(GOLDEN, "espnet_setup.json")) as fh:
        return json.load(fh)


def piece(name, which):
    _, blob, pieces, _ = packed(name)
    off, n = pieces[which]
    return blob[off:off + n]


# ---------------------------------------------------------------------------------------------- the parent's values
@pytest.mark.parametrize("name", [m[0] for m in MODELS])
def test_packed_blob_is_the_parent_commits(name):
    _, blob, _, _ = packed(name)
    want = parent()["weights"][name]
    assert blob.size == want["floats"]
    assert hashlib.sha256(blob.tobytes()).hexdigest() == want["sha256"]


@pytest.mark.parametrize("model", WS_MODELS, ids=[m[0] for m in WS_MODELS])
@pytest.mark.parametrize("shape", SHAPES, ids=["%dx%dx%d" % s for s in SHAPES])
def test_workspace_bytes_are_the_parent_commits(model, shape):
    from glomeruli_segmentation_amd.engine import workspace_bytes
    name, classes, p, enc = model
    n, h, w = shape
    for q in (0, 8):   # (no activation depends on q)
        assert workspace_bytes(n, h, w, p, q, classes, enc) == parent()["workspace"]["%s/%dx%dx%d" % (name, n, h, w)]


def test_workspace_refusals():
    from glomeruli_segmentation_amd import _lib
    from glomeruli_segmentation_amd.engine import workspace_bytes
    lib = _lib.load()
    b = ctypes.c_size_t()
    # output1_cat of one 8192 x 8192 image: 132 planes x 2049 rows x 2112 floats, more than 2^31 bytes
    assert 132 * 2049 * 2112 * 4 >= 2 ** 31
    assert lib.gs_espnet_workspace_plan(1, 8192, 8192, 2, 8, 5, 0, ctypes.byref(b)) == GS_ERR_UNSUPPORTED
    assert b"exceeds 2 GiB" in lib.gs_last_error()
    assert workspace_bytes(1, 4096, 4096, 2, 8, 5) > 0
    assert lib.gs_espnet_workspace_plan(0, 64, 128, 2, 8, 5, 0, ctypes.byref(b)) == GS_ERR_INVALID     # as check_shape refuses it
    assert b"batch size must be positive" in lib.gs_last_error()
    assert lib.gs_espnet_workspace_plan(1, 12, 64, 2, 8, 5, 0, ctypes.byref(b)) == GS_ERR_INVALID
    assert b"multiple of 8" in lib.gs_last_error()
    for classes in (1, 21):
        assert lib.gs_espnet_workspace_plan(1, 64, 128, 2, 8, classes, 0, ctypes.byref(b)) == GS_ERR_UNSUPPORTED
    assert lib.gs_espnet_workspace_plan(1, 64, 128, 2, 8, 5, 0, None) == GS_ERR_INVALID
    # ... and the parent commit answered the three shapes the same way
    assert parent()["workspace_status"] == {"c5_p2/1x8192x8192": GS_ERR_UNSUPPORTED, "c5_p2/0x64x128": GS_ERR_INVALID,
                                            "c5_p2/1x12x64": GS_ERR_INVALID}


# ---------------------------------------------------------------------------------------------- restated in numpy
def fold_bn64(sd, bn, act):
    """[scale | shift | alpha][C]: BatchNorm2d(eps=1e-3).eval() folded in float64, rounded to fp32 once"""
    g, b, m, v = (sd[bn + "." + k].astype(np.float64) for k in ("weight", "bias", "running_mean", "running_var"))
    inv = 1.0 / np.sqrt(v + 1e-3)
    return np.concatenate([(g * inv).astype(np.float32), (b - (m * g) * inv).astype(np.float32), sd[act + ".weight"]])


@pytest.mark.parametrize("name", ["p1_q2_c7", "fold1"])
def test_pieces_restated_in_numpy(name):
    sd, _, pieces, c = packed(name)
    cp = 5 if c == 5 else (c + 3) // 4 * 4
    # b2: [scale | shift | alpha][131]
    assert np.array_equal(piece(name, "b2")[:393], fold_bn64(sd, "encoder.b2.bn", "encoder.b2.act"))
    # the level-2 stride-2 reduce: [tap][cin padded to 20][12], zero in the padding plane
    w = sd["encoder.level2_0.c1.conv.weight"]                                   # [12, 19, 3, 3]
    img = np.zeros((9, 20, 12), np.float32)
    img[:, :19, :] = w.reshape(12, 19, 9).transpose(2, 1, 0)
    assert pieces["l2_0.c1"][1] == img.size and np.array_equal(piece(name, "l2_0.c1"), img.ravel())
    # up_l3's deconvolution: [cp][cp][2][2], zero beyond `classes`
    up = np.zeros((cp, cp, 2, 2), np.float32)
    up[:c, :c] = sd["up_l3.0.weight"]
    assert pieces["wup3"][1] == up.size and np.array_equal(piece(name, "wup3"), up.ravel())
    if name == "fold1":
        # the fused decoder tail's A operands: [ty][6 plane groups][64 lanes], lane = k-group * 16 + row, row = tx * classes + o
        wc = sd["conv.conv.weight"]                                             # [5, 24, 3, 3]
        a = np.zeros((3, 6, 4, 16), np.float32)
        for ty in range(3):
            for g in range(6):
                for kq in range(4):
                    for tx in range(3):
                        a[ty, g, kq, tx * c:(tx + 1) * c] = wc[:, 4 * g + kq, ty, tx]
        assert np.array_equal(piece(name, "wtail")[:a.size], a.ravel())
    else:
        assert "wtail" not in pieces and "wconv" in pieces


# ---------------------------------------------------------------------------------------------- structure
@pytest.mark.parametrize("name", [m[0] for m in MODELS])
def test_piece_structure(name):
    _, blob, pieces, _ = packed(name)
    spans = sorted(pieces.values())
    assert all(off % 4 == 0 and n > 0 for off, n in spans)                      # float4 staging
    assert all(a[0] + a[1] <= b[0] for a, b in zip(spans, spans[1:]))           # disjoint ...
    assert spans[0][0] >= 0 and spans[-1][0] + spans[-1][1] <= blob.size        # ... and inside the blob
    assert pieces["guard"] == (blob.size - 512, 512) and not blob[-512:].any()  # LDS-DMA staging reads whole 1-KiB pieces
    assert np.isfinite(blob).all()


def test_padding_planes_stay_exact_zeros():
    """seven classes in eight planes: plane 7 of every folded BN gets scale 0, shift 0 and (where the piece carries a PReLU
    slope: `br` is BatchNorm alone, [scale | shift]) slope 1, so whatever a kernel computes for it is +0"""
    for which, rows in (("br", 2), ("bncc", 3), ("bnu2", 3)):
        t = piece("p1_q2_c7", which)[:rows * 8].reshape(rows, 8)
        assert t[0, 7] == 0.0 and t[1, 7] == 0.0 and (rows == 2 or t[2, 7] == 1.0), which
        assert (t[0, :7] != 0.0).all()


# ---------------------------------------------------------------------------------------------- refusals
def _pack_status(sd, classes, p=2, q=8):
    from glomeruli_segmentation_amd import _lib
    from glomeruli_segmentation_amd.engine import pack_state_dict
    lib = _lib.load()
    blob, table = pack_state_dict(sd)
    n = ctypes.c_size_t()
    rc = lib.gs_espnet_pack_weights(blob.ctypes.data_as(ctypes.c_void_p), table, len(table), classes, p, q, 0, None, 0, ctypes.byref(n),
                                    None, 0, None)
    return rc, lib.gs_last_error()


def test_pack_refusals_without_a_device(sd1):
    key = "encoder.level3.1.d4.conv.weight"
    rc, err = _pack_status({k: v for k, v in sd1.items() if k != key}, 5)
    assert rc == GS_ERR_INVALID and key.encode() in err and b"missing" in err
    rc, err = _pack_status(dict(sd1, **{key: np.zeros((25, 25, 1, 1), np.float32)}), 5)
    assert rc == GS_ERR_INVALID and key.encode() in err and b"wrong shape" in err
    for classes in (1, 21):
        rc, err = _pack_status(sd1, classes)
        assert rc == GS_ERR_UNSUPPORTED and b"classes must be 2..20" in err
    rc, err = _pack_status(sd1, 5, p=-1)
    assert rc == GS_ERR_INVALID
    # a buffer that is too small is refused, not overrun
    from glomeruli_segmentation_amd import _lib
    from glomeruli_segmentation_amd.engine import pack_state_dict
    lib = _lib.load()
    blob, table = pack_state_dict(sd1)
    n, out = ctypes.c_size_t(), np.zeros(1000, np.float32)
    head = (blob.ctypes.data_as(ctypes.c_void_p), table, len(table), 5, 2, 8, 0)
    assert lib.gs_espnet_pack_weights(*head, out.ctypes.data_as(ctypes.c_void_p), out.size, ctypes.byref(n), None, 0, None) == GS_ERR_INVALID
    assert n.value == parent()["weights"]["fold1"]["floats"] and not out.any()
    few = (_lib.WeightPiece * 3)()
    assert lib.gs_espnet_pack_weights(*head, None, 0, ctypes.byref(n), few, 3, None) == GS_ERR_INVALID


def test_header_declares_the_setup_entries():
    import re
    from glomeruli_segmentation_amd import _lib
    with open(os.path.join(REPO, "include", "glomseg_plan.h")) as fh:
        header = re.sub(r"/\*.*?\*/", "", fh.read(), flags=re.S)
    assert {"gs_espnet_pack_weights", "gs_espnet_workspace_plan"} <= set(re.findall(r"\b(gs_[a-z0-9_]+)\s*\(", header)) == set(_lib.PLAN_PROTOTYPES)
    assert ctypes.sizeof(_lib.WeightPiece) == 48 and _lib.load().gs_abi_version() == 10


# ---------------------------------------------------------------------------------------------- sanitizers
def test_setup_headers_under_asan_ubsan(tmp_path):
    """csrc/espnet_weights.h and csrc/workspace_plan.h need no HIP: tests/helpers/espnet_setup_driver.cpp is built with g++ alone
    and run as a program of its own (no preload) -- every class count 2..20, p and q in 0..3, both handle kinds; tile sizes 8,
    64 and 520 in both dimensions at batch 1 and 3"""
    run_sanitized_driver(tmp_path, "espnet_setup_driver.cpp", "espnet setup ok: 608 packs, 2736 plans", flags=("-D_GLIBCXX_SANITIZE_VECTOR",))
