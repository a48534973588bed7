"""What a forward leaves behind in its workspace, and what it picks up from the forwards before it.

Every convolution of the ESPNet forward takes its padding from words of the activation workspace that are zeroed once, when the
workspace is laid out, and that no kernel may write afterwards (csrc/espnet_facts.h, struct Act; csrc/workspace_plan.h).  A
store past a row end, into a plane tail, a padding plane or the slack is invisible in the forward that makes it: it shows in a
later forward at the same shape, and a test that runs one forward per shape always starts on clean halos.  Likewise nothing
showed that a forward reads only what it wrote itself: lazy b2, lean forwards that skip stores, side sums parked in `tt`,
images left from a larger batch and the block hook all leave finite, similar data behind.

csrc/workspace_audit.h states the must-be-zero set; include/glomseg_workspace.h audits a lane's workspace against it and
poisons everything else.  Here:
1. CPU: the classifier against a numpy restatement of make_act / plan_workspace, and the audit against hand-corrupted copies.
2. GPU, per model kind and shape: a first forward held to float64, then a sequence of batches, mask-only forwards and block
   hook calls on the same engine -- every repeat gives the first forward's bits, every audit is clean -- and the same after the
   workspace was filled with quiet NaNs.
3. GPU: the entries that own workspaces of their own (host pipelines, two lanes, ensembles), and the large forms at 264 x 1000.
"""
import ctypes
import time
from functools import lru_cache

import numpy as np
import pytest

from conftest import random_state_dict
from helpers.header_binding import assert_declared_exported_prototyped
from test_kernel_forms import RANDOM_MEAN_STD, TAU, Case, batch_for, bound, engine_stages, over, reference, stage_errors

FREE, INTERIOR, MUST_BE_ZERO = 0, 1, 2
QNAN = 0x7fc00000
WS_SLACK = 64 * 1024
# (name, classes, p, q, encoder_only): the fused tail, side sums and lean forwards; no second class-sum producer; b2 not lazy,
# bb[0] with storage of its own; cp = 8, dec3_kernel + dec4; dec3 on the matrix cores, tt with a halo and t3 live; ESPNet-C at
# test_espnet_c.py's depths; and cp = 20 with two class planes no kernel writes, in a0c and in both halves of tt
KINDS = [("c5_p2_q8", 5, 2, 8, False), ("c5_p1_q0", 5, 1, 0, False), ("c5_p0_q1", 5, 0, 1, False), ("c7_p2_q3", 7, 2, 3, False),
         ("c20_p2_q3", 20, 2, 3, False), ("c5_encoder", 5, 2, 8, True), ("c18_p1_q1", 18, 1, 1, False)]
# every map 1 x 1 at 1/8; W/4 = 6: a vector-of-four tail of two, W/8 = 3; W/8 = 33: the non-vector level-3 forms, W/4 = 66;
# H/8 = 17: the lone last row of the stride-2 row pairs
SHAPES = [(8, 8), (16, 24), (64, 264), (136, 24)]
KIND_IDS, SHAPE_IDS = [k[0] for k in KINDS], ["%dx%d" % s for s in SHAPES]


def padded_classes(classes):
    return 5 if classes == 5 else -(-classes // 4) * 4


# ---------------------------------------------------------------------------------------------- make_act / plan_workspace in numpy
def np_act(C, Cp, H, W, pt, pb, pl, pr):
    pitch = -(-(pl + W + pr) // 32) * 32
    rows = pt + H + pb
    return dict(C=C, Cp=Cp, H=H, W=W, pt=pt, pl=pl, rows=rows, pitch=pitch, sc=rows * pitch + 96, padded=bool(pt or pb or pl or pr or Cp > C),
                dead=())


def np_pieces(ws_n, H, W, classes, p, encoder_only):
    """[(name, act | None, byte offset, span words)] in allocation order"""
    cls = padded_classes(classes)
    H1, W1, H2, W2, H3, W3 = H // 2, W // 2, H // 4, W // 4, H // 8, W // 8
    token = np_act(1, 1, 8, 8, 0, 0, 0, 0)
    mfma = cls >= 12
    acts = [("a0c", np_act(cls + 19, cls + 20, H1, W1, 1, 1, 32, 1)), ("inp1", np_act(3, 3, H1, W1, 0, 0, 0, 0)),
            ("inp2", np_act(3, 3, H2, W2, 0, 0, 0, 0))]
    acts += [("r2[%d]" % i, np_act(12, 12, H2, W2, 16, 16, 32, 16)) for i in range(2)]
    acts += [("bb[%d]" % i, None if i == 0 and p > 0 else np_act(64, 64, H2, W2, 0, 0, 0, 0)) for i in range(3)]
    acts += [("a1", np_act(131, 132, H2, W2, 1, 0, 32, 1))]
    acts += [("r3[%d]" % i, np_act(25, 26, H3, W3, 16, 16, 32, 16)) for i in range(2)]
    acts += [("cc[%d]" % i, np_act(128, 128, H3, W3, 0, 0, 0, 0)) for i in range(3)]
    acts += [("o2c", np_act(cls, cls, H2, W2, 0, 0, 0, 0)),
             ("l3c", np_act(cls, cls, H2, W2, 0, 0, 0, 0) if cls == 5 and not encoder_only else token),
             ("tt", np_act(2 * cls, 2 * cls, H2, W2, *((1, 1, 32, 1) if mfma else (0, 0, 0, 0)))),
             ("t3", np_act(cls, cls, H2, W2, 0, 0, 0, 0) if mfma else token), ("ff", np_act(cls, cls, H1, W1, 0, 0, 0, 0))]
    # the decoder kernels' stores stop at the model's class count: the class planes beyond it that a matrix-core convolution
    # reads (comb_l2_l3 in a0c; both halves of tt when dec3 runs there) are written by nothing and read as zeros
    dict(acts)["a0c"]["dead"] = tuple(range(classes, cls))
    if mfma:
        dict(acts)["tt"]["dead"] = tuple(k for k in range(2 * cls) if k % cls >= classes)
    out, at = [], 0
    for name, a in acts:
        own = ws_n * a["Cp"] * a["sc"] * 4 if a else 0
        span = -(-(own + WS_SLACK) // 256) * 256
        out.append((name, a, at, span // 4))
        at += span
    return out, at


def np_class_map(a, ws_n, span_words):
    m = np.full(span_words, MUST_BE_ZERO, np.uint8)
    if a is None:
        return m
    other = MUST_BE_ZERO if a["padded"] else FREE
    plane = np.full(a["sc"], other, np.uint8)
    plane[:a["rows"] * a["pitch"]].reshape(a["rows"], a["pitch"])[a["pt"]:a["pt"] + a["H"], a["pl"]:a["pl"] + a["W"]] = INTERIOR
    image = np.concatenate([np.tile(plane, a["C"]), np.full((a["Cp"] - a["C"]) * a["sc"], other, np.uint8)])
    for c in a["dead"]:
        image[c * a["sc"]:(c + 1) * a["sc"]] = MUST_BE_ZERO
    m[:ws_n * image.size] = np.tile(image, ws_n)
    return m


@lru_cache(maxsize=None)
def library_classes(ws_n, H, W, classes, p, q, enc):
    from glomeruli_segmentation_amd.engine import workspace_classes
    return workspace_classes(ws_n, H, W, p, q, classes, enc)


# ---------------------------------------------------------------------------------------------- CPU: the classifier
@pytest.mark.parametrize("shape", SHAPES + [(264, 1000)], ids=SHAPE_IDS + ["264x1000"])
@pytest.mark.parametrize("kind", KINDS, ids=KIND_IDS)
def test_classifier_is_the_numpy_restatement(kind, shape):
    from glomeruli_segmentation_amd.engine import workspace_bytes
    _, classes, p, q, enc = kind
    H, W = shape
    ws_n = 2 if H > 136 else 5
    want, total = np_pieces(ws_n, H, W, classes, p, enc)
    got = library_classes(ws_n, H, W, classes, p, q, enc)
    assert [pc["name"] for pc, _ in got] == [name for name, _, _, _ in want] and len(got) == 19
    # the spans tile the allocation: the views (ee, a0, lazy bb[0]) add nothing to it
    assert total == workspace_bytes(ws_n, H, W, p, q, classes, enc)
    assert sum(pc["span_words"] for pc, _ in got) * 4 == total
    padded = set()
    for (pc, cmap), (name, a, at, span) in zip(got, want):
        assert (pc["offset"], pc["span_words"]) == (at, span), name
        assert pc["own_words"] == (ws_n * a["Cp"] * a["sc"] if a else 0), name
        ref = np_class_map(a, ws_n, span)
        assert np.array_equal(cmap, ref), (name, int(np.flatnonzero(cmap != ref)[0]))
        # the three classes partition the span
        counts = np.bincount(cmap, minlength=3)
        assert counts.size == 3 and counts.sum() == span
        assert counts[INTERIOR] == (ws_n * (a["C"] - len(a["dead"])) * a["H"] * a["W"] if a else 0), name
        slack = span - pc["own_words"]
        assert slack >= WS_SLACK // 4 and (cmap[pc["own_words"]:] == MUST_BE_ZERO).all()
        if pc["padded"]:
            padded.add(name)
            assert counts[FREE] == 0
        else:   # a halo-less piece: its must-be-zero set is exactly its slack
            assert counts[MUST_BE_ZERO] == slack, name
    assert padded == {"a0c", "r2[0]", "r2[1]", "a1", "r3[0]", "r3[1]"} | ({"tt"} if padded_classes(classes) >= 12 else set())
    bb0 = got[5][0]
    assert bb0["name"] == "bb[0]" and (bb0["own_words"] == 0) == (p > 0)


def test_classifier_refusals():
    from glomeruli_segmentation_amd import _lib
    lib = _lib.load()
    n = ctypes.c_int()
    info = _lib.WorkspacePiece()
    assert lib.gs_espnet_workspace_classes(1, 8, 8, 2, 8, 5, 0, 0, None, None, 0, ctypes.byref(n)) == _lib.GS_OK and n.value == 19
    assert lib.gs_espnet_workspace_classes(1, 12, 8, 2, 8, 5, 0, 0, None, None, 0, ctypes.byref(n)) != _lib.GS_OK      # as check_shape refuses it
    assert lib.gs_espnet_workspace_classes(0, 8, 8, 2, 8, 5, 0, 0, None, None, 0, ctypes.byref(n)) != _lib.GS_OK
    assert lib.gs_espnet_workspace_classes(1, 8, 8, 2, 8, 21, 0, 0, None, None, 0, ctypes.byref(n)) != _lib.GS_OK
    for piece in (-1, 19):
        assert lib.gs_espnet_workspace_classes(1, 8, 8, 2, 8, 5, 0, piece, ctypes.byref(info), None, 0, None) != _lib.GS_OK
    small = np.zeros(16, np.uint8)      # a map that is too small is refused, not overrun
    assert lib.gs_espnet_workspace_classes(1, 8, 8, 2, 8, 5, 0, 0, None, small.ctypes.data_as(ctypes.c_void_p), small.size, None) != _lib.GS_OK
    assert not small.any()
    rep = _lib.WorkspaceReport()
    assert lib.gs_espnet_workspace_audit_host(1, 8, 8, 2, 8, 5, 0, small.ctypes.data_as(ctypes.c_void_p), small.size, ctypes.byref(rep)) != _lib.GS_OK
    assert lib.gs_espnet_workspace_audit(None, 0, ctypes.byref(rep)) != _lib.GS_OK
    assert lib.gs_espnet_workspace_poison(None, 0, QNAN) != _lib.GS_OK


def test_header_declares_the_workspace_entries():
    from glomeruli_segmentation_amd import _lib
    text = assert_declared_exported_prototyped("glomseg_workspace.h", _lib.WORKSPACE_PROTOTYPES,
                                               {"gs_espnet_workspace_classes", "gs_espnet_workspace_audit_host", "gs_espnet_workspace_audit",
                                                "gs_espnet_workspace_poison"})
    assert "TEST TOOLS" in text and "1 GiB" in text
    assert ctypes.sizeof(_lib.WorkspaceReport) == 56 and ctypes.sizeof(_lib.WorkspacePiece) == 72
    assert (_lib.GS_WS_FREE, _lib.GS_WS_INTERIOR, _lib.GS_WS_MUST_BE_ZERO) == (FREE, INTERIOR, MUST_BE_ZERO)


# ---------------------------------------------------------------------------------------------- CPU: the audit can fail
def test_audit_names_a_hand_corrupted_word():
    """A zeroed host copy of a workspace (two images of 16 x 24, the 20-class network: every padded piece) audits clean, also with
    every interior and free word a NaN; one word set in each region of the must-be-zero set is reported as THE offender with
    its coordinates; of two, the first in allocation order."""
    from glomeruli_segmentation_amd.engine import workspace_audit_host
    ws_n, H, W, classes, p, q = 2, 16, 24, 20, 2, 3
    pieces, total = np_pieces(ws_n, H, W, classes, p, False)
    by_name = {name: (a, at // 4) for name, a, at, _ in pieces}
    copy = np.zeros(total // 4, np.uint32)

    def audit():
        return workspace_audit_host(copy, ws_n, H, W, p, q, classes)
    must = sum(int((np_class_map(a, ws_n, span) == MUST_BE_ZERO).sum()) for _, a, _, span in pieces)
    assert audit() == {"must_be_zero": must, "offenders": 0, "first": None}
    for name, a, at, span in pieces:      # what the poison entry writes is no offender
        copy[at // 4:at // 4 + span][np_class_map(a, ws_n, span) != MUST_BE_ZERO] = QNAN
    assert audit() == {"must_be_zero": must, "offenders": 0, "first": None}
    assert int((copy == QNAN).sum()) == copy.size - must

    def word(name, image, plane, row, col):
        a, base = by_name[name]
        return base + (image * a["Cp"] + plane) * a["sc"] + (row + a["pt"]) * a["pitch"] + col + a["pl"]
    a1, r3, a0c, tt = (by_name[k][0] for k in ("a1", "r3[0]", "a0c", "tt"))
    assert (a1["W"], a1["pitch"], r3["W"], r3["pitch"], a0c["H"], a0c["rows"], tt["pl"]) == (6, 64, 3, 64, 8, 10, 32)
    cases = [("a left halo", ("a1", 1, 3, 2, -1)), ("a right halo", ("tt", 0, 39, 0, 6)), ("a top halo", ("r3[1]", 1, 0, -16, 0)),
             ("a bottom halo", ("r2[0]", 0, 11, 4 + 15, 5)), ("a pitch tail", ("r3[0]", 0, 24, 1, 3 + 16 + 2)),
             ("a + 96 tail", ("a0c", 1, 0, 9, -32 + 5)), ("the last word of a + 96 tail", ("a0c", 0, 23, 10, -1)), ("a padding plane", ("a1", 0, 131, 0, 0)), ("a padding plane", ("a0c", 1, 39, 7, 11)),
             ("a padding plane", ("r3[0]", 1, 25, 1, 2))]
    for what, (name, image, plane, row, col) in cases:
        w = word(name, image, plane, row, col)
        keep, copy[w] = copy[w], 0x3f800000
        assert keep == 0, what
        assert audit() == {"must_be_zero": must, "offenders": 1, "first": {"piece": name, "image": image, "plane": plane, "row": row,
                                                                            "col": col, "bits": 0x3f800000}}, what
        copy[w] = keep
    # the slack: behind a halo-less piece, behind a padded one, and the span of lazy bb[0], which is slack alone
    for name, a, at, span in pieces:
        if name not in ("ff", "a1", "bb[0]", "cc[1]"):
            continue
        own = ws_n * a["Cp"] * a["sc"] if a else 0
        for k in (0, span - own - 1):
            copy[at // 4 + own + k] = 0x80000000      # -0.0 is not the zero the workspace was filled with
            assert audit()["first"] == {"piece": name, "image": ws_n if a else 0, "plane": 0, "row": 0, "col": k, "bits": 0x80000000}, name
            copy[at // 4 + own + k] = 0
    # class planes beyond the model's count that a matrix-core convolution reads as zeros: comb_l2_l3's of a 7-class model
    # (cp = 8), and of an 18-class one (cp = 20, dec3 on the matrix cores) those of both halves of tt too
    for cls_, dead in ((7, [("a0c", 7)]), (18, [("a0c", 18), ("a0c", 19), ("tt", 18), ("tt", 19), ("tt", 38), ("tt", 39)])):
        pcs, tot = np_pieces(1, 16, 24, cls_, 2, False)
        buf = np.zeros(tot // 4, np.uint32)
        for name, plane in dead:
            a, at = next((a, at) for nm, a, at, _ in pcs if nm == name)
            w = at // 4 + plane * a["sc"] + (1 + a["pt"]) * a["pitch"] + 2 + a["pl"]
            buf[w] = QNAN
            rep = workspace_audit_host(buf, 1, 16, 24, 2, 3, cls_)
            assert rep["offenders"] == 1 and rep["first"] == {"piece": name, "image": 0, "plane": plane, "row": 1, "col": 2, "bits": QNAN}
            buf[w - a["sc"] * (plane % padded_classes(cls_) - cls_ + 1)] = QNAN      # the last real class's plane: interior
            assert workspace_audit_host(buf, 1, 16, 24, 2, 3, cls_)["offenders"] == 1
            buf[:] = 0
    # two offenders: the count is two, the first in allocation order is named
    copy[word("r3[0]", 0, 25, 0, 0)] = 7
    copy[word("a1", 1, 131, 3, 5)] = 9
    rep = audit()
    assert rep["offenders"] == 2 and rep["first"] == {"piece": "a1", "image": 1, "plane": 131, "row": 3, "col": 5, "bits": 9}


def test_audit_header_under_asan_ubsan(tmp_path):
    """csrc/workspace_audit.h needs no HIP: tests/helpers/workspace_audit_driver.cpp is built with g++ alone and run as a program of
    its own (no preload) -- runs, class map, poison, audit and ws_where over heap copies of exactly each span's size, six class
    counts, both handle kinds, b2 lazy and not, seven shapes"""
    from helpers.sanitized_driver import assert_no_hip, run_sanitized_driver
    assert_no_hip("workspace_audit.h")
    run_sanitized_driver(tmp_path, "workspace_audit_driver.cpp", "workspace audit ok: 98 plans, 126805120 words", flags=("-D_GLIBCXX_SANITIZE_VECTOR",))


# ---------------------------------------------------------------------------------------------- the GPU cases
@pytest.fixture(scope="module")
def torch_mod():
    import torch
    assert torch.cuda.is_available(), "the gpu-marked tests need a HIP device"
    return torch


def kind_case(kind, H, W):
    name, classes, p, q, _ = kind
    return Case(name, "random", classes, p, q, H, W, 1, {}, set())


def kind_weights(kind):
    _, classes, p, q, enc = kind
    sd = random_state_dict(p, q, classes=classes, seed=7100 + 37 * classes + 5 * p + q)
    return sd, ({k[len("encoder."):]: v for k, v in sd.items() if k.startswith("encoder.")} if enc else sd)


@lru_cache(maxsize=None)
def tiles_ab(H, W):
    """A: five tiles, synthetic in even slots and noise in odd ones; B: five different ones, the middle one pure noise"""
    from glomeruli_segmentation_amd.synth import noise_tile, synth_tile
    a = np.stack([(noise_tile if k % 2 else synth_tile)(8800 + H + W + k, H, W) for k in range(5)])
    b = np.stack([(noise_tile if k == 2 else synth_tile)(8900 + H + W + k, H, W) for k in range(5)])
    a.setflags(write=False)
    b.setflags(write=False)
    return a, b


def stage_names(kind, H, W, num_cus, n, want_logits):
    """the stages read_stage serves after such a forward"""
    from glomeruli_segmentation_amd.engine import plan_flags, plan_lean
    _, classes, p, q, enc = kind
    names = engine_stages(kind_case(kind, H, W))
    if enc:
        return [s for s in names if s not in ("up_l3", "combine_t", "up_l2", "conv")]
    if plan_flags(n, H, W, p, q, classes, num_cus)["l3c_in_reduce"]:
        names.append("level3_C")
    if not want_logits:
        names.remove("conv")
        if plan_lean(n, H, W, p, q, classes, num_cus):
            names = [s for s in names if s not in ("combine_t", "level3.%d" % (q - 1))]
    return names


def bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


class Audited:
    """an engine whose every call is followed by an audit of its workspace"""

    def __init__(self, torch, kind, H, W):
        from glomeruli_segmentation_amd.engine import EspnetEngine
        self.torch, self.kind, self.H, self.W = torch, kind, H, W
        _, self.classes, self.p, self.q, self.enc = kind
        self.full_sd, sd = kind_weights(kind)
        self.eng = EspnetEngine(sd, classes=self.classes, p=self.p, q=self.q, encoder_only=self.enc)
        self.num_cus = torch.cuda.get_device_properties(0).multi_processor_count
        self.mean, self.std = RANDOM_MEAN_STD
        self.audits, self.audit_s, self.words = 0, 0.0, 0

    def audit(self, what):
        t0 = time.perf_counter()
        rep = self.eng.workspace_audit()
        self.audit_s += time.perf_counter() - t0
        self.audits += 1
        self.words = rep["must_be_zero"]
        assert rep["offenders"] == 0, "%s %dx%d after %s: %d of %d must-be-zero words are not zero, the first: %s" % (
            self.kind[0], self.H, self.W, what, rep["offenders"], rep["must_be_zero"], rep["first"])
        assert rep["must_be_zero"] > 0

    def forward(self, tiles, want_logits, what):
        """-> {"mask", "hist", "logits" | None, "stages": {name: [n, ...]}} on the host, audited"""
        torch, eng, n = self.torch, self.eng, len(tiles)
        t = torch.from_numpy(np.array(tiles)).cuda()
        key = "want_enc_logits" if self.enc else "want_logits"
        mask, hist, logits = eng.segment(t, self.mean, self.std, **{key: want_logits})
        torch.cuda.synchronize()
        out = {"mask": mask.cpu().numpy(), "hist": hist.cpu().numpy(), "logits": logits.cpu().numpy() if want_logits else None}
        out["stages"] = {name: np.stack([eng.read_stage(name, image=k) for k in range(n)])
                         for name in stage_names(self.kind, self.H, self.W, self.num_cus, n, want_logits)}
        self.audit(what)
        return out

    def same_bits(self, got, first, what):
        """`got` of a forward of the first k tiles of the first forward's batch: its bits, and nothing that is not finite"""
        k = len(got["mask"])
        where = "%s %dx%d, %s" % (self.kind[0], self.H, self.W, what)
        assert np.array_equal(got["mask"], first["mask"][:k]), where
        assert np.array_equal(got["hist"], first["hist"][:k]) and (got["hist"].sum(1) == self.H * self.W).all(), where
        if got["logits"] is not None:
            assert np.isfinite(got["logits"]).all(), where
            assert np.array_equal(bits(got["logits"]), bits(first["logits"][:k])), where
        assert got["stages"]
        for name, v in got["stages"].items():
            assert np.isfinite(v).all(), (where, name, int((~np.isfinite(v)).sum()))
            assert np.array_equal(bits(v), bits(first["stages"][name][:k])), (where, name)

    def hold_to_float64(self, tiles, first):
        """the first forward against oracle/espnet_torch_port.py in float64 with test_kernel_forms.py's bounds; ESPNet-C: the
        1/8-scale logits against its encoder classifier, and the class map against test_espnet_c.py's head reference"""
        case = kind_case(self.kind, self.H, self.W)
        tiles = np.array(tiles)      # (a writable copy: the port hands it to torch)
        if not self.enc:
            ref = reference(case, self.full_sd, self.mean, self.std, tiles)
            got = dict(first["stages"], logits=first["logits"])
            ref = {name: v for name, v in ref.items() if name in got}
            assert set(ref) >= set(engine_stages(case)) | {"logits"}
        else:
            from oracle import espnet_torch_port as port
            from test_espnet_c import check_head
            st = {}
            port.forward64(tiles, self.full_sd, self.mean, self.std, self.p, self.q, st)
            ref = {name: st[name].numpy() for name in first["stages"]}
            ref["logits"] = st["enc_classifier"].numpy()
            got = dict(first["stages"], logits=first["logits"])
            check_head(first["mask"], first["hist"], first["logits"], self.classes, case.name)
        errors = stage_errors(case, got, ref)
        assert all(b == TAU[name.split(".")[0]] * max(1.0, float(np.abs(ref[name]).max())) for name, (_, b) in errors.items())
        assert bound(case, "logits", ref["logits"]) == errors["logits"][1]
        print("%s %dx%d, first forward, worst error / bound: %s" % (
            case.name, self.H, self.W, ", ".join("%s %.1e/%.1e" % (k, e, b) for k, (e, b) in errors.items())))
        assert not over(errors), (case.name, self.H, self.W, over(errors))
        if not self.enc:
            for k in range(len(tiles)):
                assert np.array_equal(first["mask"][k], first["logits"][k].argmax(0).astype(np.uint8)), k
        for k in range(len(tiles)):
            assert np.array_equal(first["hist"][k], np.bincount(first["mask"][k].ravel(), minlength=self.classes)), k

    def block_hooks(self):
        """one down-sampler and one ESP block through gs_espnet_block_forward at this tile size: inputs written into the very
        buffers the forward uses"""
        rng = np.random.default_rng(55)
        H, W, eng = self.H, self.W, self.eng
        out = eng.block_forward(1, 2, 0, rng.standard_normal((19, H // 2, W // 2)).astype(np.float32))
        assert np.isfinite(out).all() and out.shape == (64, H // 4, W // 4)
        self.audit("the level-2 down-sampler alone")
        if self.p > 0:
            out = eng.block_forward(0, 2, 0, rng.standard_normal((64, H // 4, W // 4)).astype(np.float32))
            assert np.isfinite(out).all() and out.shape == (64, H // 4, W // 4)
            self.audit("a level-2 ESP block alone")
        if self.q > 0:
            out = eng.block_forward(0, 3, 0, rng.standard_normal((128, H // 8, W // 8)).astype(np.float32))
            assert np.isfinite(out).all() and out.shape == (128, H // 8, W // 8)
            self.audit("a level-3 ESP block alone")
        out = eng.block_forward(1, 3, 0, rng.standard_normal((131, H // 4, W // 4)).astype(np.float32))
        assert np.isfinite(out).all() and out.shape == (128, H // 8, W // 8)
        self.audit("the level-3 down-sampler alone")

    def poison(self):
        self.eng.workspace_poison(QNAN)
        self.audit("the poison")


@pytest.mark.gpu
@pytest.mark.parametrize("shape", SHAPES, ids=SHAPE_IDS)
@pytest.mark.parametrize("kind", KINDS, ids=KIND_IDS)
def test_forwards_leave_the_halos_zero_and_read_no_history(torch_mod, kind, shape):
    """Per model kind and shape (see the module's text): the first forward of five tiles within the float64 bounds; then, on the
    same engine, other tiles, smaller batches, mask-only forwards and block hook calls in between -- every forward of the first
    k tiles gives the first forward's bits, stages included, and after every call no must-be-zero word of the workspace holds
    anything but 0x00000000; then the same with every interior and free word of the workspace a quiet NaN before the call, also
    with images 2..4 left NaN while two tiles run."""
    H, W = shape
    A, B = tiles_ab(H, W)
    t0 = time.perf_counter()
    dev = Audited(torch_mod, kind, H, W)
    try:
        first = dev.forward(A, True, "the first forward")
        dev.hold_to_float64(A, first)
        only = dev.forward(B, False, "B mask-only")
        assert (only["hist"].sum(1) == H * W).all()
        dev.same_bits(dev.forward(A[:2], True, "A[:2] with logits"), first, "A[:2] after B")
        dev.forward(B[:1], False, "B[:1] mask-only")
        dev.same_bits(dev.forward(A[:1], True, "A[:1] with logits"), first, "A[:1] after B[:1]")
        dev.block_hooks()
        dev.same_bits(dev.forward(A, True, "A with logits"), first, "A after the block hooks")
        dev.same_bits(dev.forward(A, False, "A mask-only"), first, "A mask-only after A")
        for tiles, what in ((A, "A"), (A[:2], "A[:2]")):
            for want_logits in (True, False):
                dev.poison()
                how = "%s %s after the poison" % (what, "with logits" if want_logits else "mask-only")
                dev.same_bits(dev.forward(tiles, want_logits, how), first, how)
        dev.eng.check_device_faults()
        print("%s %dx%d: %d audits of %d must-be-zero words clean, %.3f s in audits, %.2f s in all" % (
            kind[0], H, W, dev.audits, dev.words, dev.audit_s, time.perf_counter() - t0))
    finally:
        dev.eng.close()


# ---------------------------------------------------------------------------------------------- lanes and entries that own workspaces
def audit_every_lane(engines, what, lanes=(0, 1)):
    """lanes: the lanes the call went through (another lane may have no workspace yet, and then nothing to audit)"""
    for j, eng in enumerate(engines):
        for lane in lanes:
            rep = eng.workspace_audit(lane)
            assert rep["offenders"] == 0, "%s, engine %d lane %d: %d offenders, the first %s" % (what, j, lane, rep["offenders"], rep["first"])
            assert rep["must_be_zero"] > 0, (what, j, lane)      # (the lane has a workspace: the call went through it)


HOST_KIND = KINDS[0]


@pytest.fixture(scope="module")
def two_lanes(torch_mod):
    from glomeruli_segmentation_amd.engine import EspnetEngine
    eng = EspnetEngine(kind_weights(HOST_KIND)[1], classes=5, p=2, q=8, lanes=2)
    yield eng
    eng.close()


def resident(torch, eng, tiles):
    mean, std = RANDOM_MEAN_STD
    mask, hist, _ = eng.segment(torch.from_numpy(np.array(tiles)).cuda(), mean, std)
    torch.cuda.synchronize()
    return mask.cpu().numpy(), hist.cpu().numpy()


@pytest.mark.gpu
def test_segment_host_leaves_both_lanes_clean(torch_mod, two_lanes):
    """gs_espnet_segment_host: seven tiles of 64 x 264 in batches of two (lanes 0, 1, 0, 1; the last batch one tile), twice"""
    A, B = tiles_ab(64, 264)
    tiles = np.concatenate([A, B[:2]])
    mean, std = RANDOM_MEAN_STD
    want = resident(torch_mod, two_lanes, tiles)
    for k in range(2):
        masks, hist = two_lanes.segment_host(tiles, mean, std, batch=2)
        assert np.array_equal(masks, want[0]) and np.array_equal(hist, want[1])
        audit_every_lane([two_lanes], "segment_host, call %d" % k)
    two_lanes.check_device_faults()


@pytest.mark.gpu
def test_segment_crops_host_leaves_both_lanes_clean(torch_mod, two_lanes):
    """gs_espnet_segment_crops_host with two lanes in flight: crops of seven sizes at a 64 x 264 network size, batches of two"""
    from glomeruli_segmentation_amd.engine import segment_crops_host
    from glomeruli_segmentation_amd.synth import synth_tile
    sizes = [(37, 91), (300, 420), (64, 264), (200, 77), (130, 257), (96, 96), (411, 333)]      # test_gpu_parity.CROP_SIZES, one at the network size
    crops = [synth_tile(8700 + k, -(-h // 8) * 8, -(-w // 8) * 8)[:h, :w].copy() for k, (h, w) in enumerate(sizes)]
    first = None
    for k in range(2):
        r = segment_crops_host([two_lanes], [RANDOM_MEAN_STD], crops, 64, 264, 2, want_net_maps=True)
        audit_every_lane([two_lanes], "segment_crops_host, call %d" % k)
        assert (np.asarray(r["net_maps"]) < 5).all() and [m.shape for m in r["masks"]] == sizes
        got = [np.array(m) for m in r["masks"]] + [np.array(r["net_maps"]), np.array(r["counts"])]
        if first is None:
            first = got
        assert all(np.array_equal(a, b) for a, b in zip(got, first))
    # the crop at the network size is the resident forward's map
    assert np.array_equal(first[2], resident(torch_mod, two_lanes, crops[2][None])[0][0])
    two_lanes.check_device_faults()


@pytest.mark.gpu
def test_ensemble_leaves_every_members_workspace_clean(torch_mod, two_lanes):
    """an ensemble of two five-class members, resident and through the crop host pipeline (both lanes of both members)"""
    from glomeruli_segmentation_amd.engine import EspnetEngine, ensemble_segment, segment_crops_host
    torch = torch_mod
    other = EspnetEngine(random_state_dict(2, 3, classes=5, seed=7199), classes=5, p=2, q=3, lanes=2)
    try:
        engs, ms = [two_lanes, other], [RANDOM_MEAN_STD, ((100.0, 140.0, 120.0), (50.0, 65.0, 60.0))]
        A, B = tiles_ab(64, 264)
        t = torch.from_numpy(np.array(A)).cuda()
        mask, hist = ensemble_segment(engs, t, ms)
        torch.cuda.synchronize()
        audit_every_lane(engs, "the ensemble", lanes=(0,))
        assert (hist.sum(1) == 64 * 264).all()
        ensemble_segment(engs, torch.from_numpy(np.array(B[:3])).cuda(), ms)
        m2, h2 = ensemble_segment(engs, t, ms)
        torch.cuda.synchronize()
        audit_every_lane(engs, "the ensemble again", lanes=(0,))
        assert torch.equal(m2, mask) and torch.equal(h2, hist)
        r = segment_crops_host(engs, ms, list(A) + list(B[:2]), 64, 264, 2, want_net_maps=True)
        audit_every_lane(engs, "the ensemble's crop pipeline")
        assert np.array_equal(np.asarray(r["net_maps"])[:5], mask.cpu().numpy())
        for e in engs:
            e.check_device_faults()
    finally:
        other.close()


@pytest.mark.gpu
def test_a_forward_on_lane_1_between_two_on_lane_0(torch_mod, two_lanes):
    torch = torch_mod
    mean, std = RANDOM_MEAN_STD
    A, B = tiles_ab(64, 264)
    a, b = torch.from_numpy(np.array(A)).cuda(), torch.from_numpy(np.array(B)).cuda()
    m0, h0, l0 = two_lanes.segment(a, mean, std, want_logits=True, lane=0)
    m1, h1, l1 = two_lanes.segment(b, mean, std, want_logits=True, lane=1)
    m2, h2, l2 = two_lanes.segment(a, mean, std, want_logits=True, lane=0)
    two_lanes.wait_lanes()
    torch.cuda.synchronize()
    audit_every_lane([two_lanes], "lane 0, lane 1, lane 0")
    assert torch.equal(m2, m0) and torch.equal(h2, h0) and torch.equal(l2, l0)
    two_lanes.workspace_poison(QNAN, lane=0)      # lane 1's workspace keeps B's activations: lane 0 must not need them, nor its own
    m3, h3, l3 = two_lanes.segment(b, mean, std, want_logits=True, lane=0)
    two_lanes.wait_lanes()
    torch.cuda.synchronize()
    audit_every_lane([two_lanes], "B on lane 0 after the poison")
    assert torch.equal(m3, m1) and torch.equal(h3, h1) and torch.equal(l3, l1) and bool(torch.isfinite(l3).all())
    two_lanes.check_device_faults()


# ---------------------------------------------------------------------------------------------- the large forms
@pytest.mark.gpu
def test_large_forms_leave_the_halos_zero(torch_mod):
    """264 x 1000, the ragged size of test_kernel_forms.py's case C, at its batch: the large level-3 forms and the strip teams
    are chosen from this size on.  Audit only: twice the batch with logits, once mask-only."""
    from test_kernel_forms import CASES
    torch = torch_mod
    case = next(c for c in CASES if c.name == "C")
    kind = ("c5_p2_q8", 5, 2, 8, False)
    assert (case.H, case.W, case.classes, case.p, case.q) == (264, 1000, 5, 2, 8)
    t0 = time.perf_counter()
    dev = Audited(torch, kind, case.H, case.W)
    try:
        n = batch_for(case, dev.num_cus)
        A, B = tiles_ab(case.H, case.W)
        tiles = torch.from_numpy(np.concatenate([A, B])[np.arange(n) % 10]).cuda()
        mean, std = RANDOM_MEAN_STD
        outs = []
        for k, want_logits in enumerate((True, True, False)):
            outs.append(dev.eng.segment(tiles, mean, std, want_logits=want_logits))
            dev.audit("forward %d of %d tiles" % (k, n))
        assert all(torch.equal(o[0], outs[0][0]) and torch.equal(o[1], outs[0][1]) for o in outs[1:])
        assert torch.equal(outs[1][2], outs[0][2]) and bool(torch.isfinite(outs[0][2]).all())
        dev.eng.check_device_faults()
        print("264x1000 x %d: %d audits of %d must-be-zero words clean, %.3f s per audit, %.2f s in all" % (
            n, dev.audits, dev.words, dev.audit_s / dev.audits, time.perf_counter() - t0))
    finally:
        dev.eng.close()
