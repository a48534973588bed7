"""ForwardPlan::lean (csrc/forward_plan.h), the one decision of the forward plan that depends on the request: a forward asked for
no logits whose plan computes both decoder projections as side sums (cls_in_l3 and l3c_in_reduce: a full five-class network with
q >= 1) reads neither the last level-3 block's map nor the normalised cat, so that launch stores no map (F_CLS_ONLY,
csrc/conv_mfma.h) and dec2_br_kernel is not launched.  Host-only: gs_espnet_plan_lean (include/glomseg_lean.h) needs no device.
The GPU side is tests/test_lean_forward.py.
"""
import ctypes
import os
import re

from conftest import REPO
from helpers.header_binding import assert_declared_exported_prototyped
from test_kernel_forms import CASES, batch_for, plan

CSRC = os.path.join(REPO, "glomeruli_segmentation_amd", "csrc")


def lean(n, H, W, p, q, classes, num_cus=256, encoder_only=False, want_logits=False):
    from glomeruli_segmentation_amd.engine import plan_lean
    return plan_lean(n, H, W, p, q, classes, num_cus, encoder_only=encoder_only, want_logits=want_logits)


def test_truth_table():
    """lean <=> no logits, five class planes, q >= 1, not an ESPNet-C handle -- at any batch, tile size, p and CU count.  The class
    counts are those whose padded counts are 4, 5, 8 and 20."""
    for n in (1, 9, 32):
        for H, W in ((8, 8), (16, 24), (64, 264), (512, 1024)):
            for p in (0, 2):
                for num_cus in (64, 256, 304):
                    for classes in (4, 5, 8, 20):
                        for q in (0, 1, 8):
                            for want_logits in (False, True):
                                want = not want_logits and classes == 5 and q >= 1
                                assert lean(n, H, W, p, q, classes, num_cus, want_logits=want_logits) == want, (n, H, W, p, q, classes)
                                assert not lean(n, H, W, p, q, classes, num_cus, encoder_only=True, want_logits=want_logits)


def test_lean_is_both_side_sums_and_no_logits():
    """... which is exactly: the two flags gs_espnet_plan_flags reports, and a request without logits."""
    from glomeruli_segmentation_amd.engine import plan_cls_in_l3, plan_flags
    for classes in range(2, 21):
        for q in (0, 1, 2, 8):
            for enc in (False, True):
                both = plan_flags(4, 64, 264, 2, q, classes, 256, enc)["l3c_in_reduce"] and plan_cls_in_l3(4, 64, 264, 2, q, classes, 256, enc)
                assert lean(4, 64, 264, 2, q, classes, 256, enc) == both
                assert not lean(4, 64, 264, 2, q, classes, 256, enc, want_logits=True)


def test_the_forms_do_not_depend_on_the_request():
    """plan_forward without the new argument returns what it returned before: the known answers of tests/test_kernel_forms.py's
    case table (written by hand for the parent) still hold, and gs_espnet_plan_forward / gs_espnet_plan_flags -- which pass no
    request -- are the entries the forward's own plan is read through: their signatures have not changed."""
    from glomeruli_segmentation_amd import _lib
    for c in CASES:
        f = plan(batch_for(c, 256), c.H, c.W, c.p, c.q, c.classes, 256)
        assert all(f.get(k) == v for k, v in c.targets.items()), c.name
        assert c.n256 == batch_for(c, 256)
    assert _lib.PROTOTYPES["gs_espnet_plan_forward"][1] == [ctypes.c_int] * 7 + [ctypes.POINTER(ctypes.c_int), ctypes.c_int,
                                                                                  ctypes.POINTER(ctypes.c_int)]
    assert _lib.PLAN_PROTOTYPES["gs_espnet_plan_flags"][1] == [ctypes.c_int] * 8 + [ctypes.POINTER(ctypes.c_int)]
    with open(os.path.join(CSRC, "forward_plan.h")) as fh:
        text = fh.read()
    # one trailing parameter with a default that keeps every existing caller's plan
    assert re.search(r"plan_forward\(int n, int H, int W, int p, int q, int cp, int num_cus, bool no_vec, bool encoder_only = false,\s*"
                     r"bool want_logits = true\)", text)


def test_entry_is_declared_exported_and_refuses_what_the_planner_refuses():
    from glomeruli_segmentation_amd import _lib
    text = assert_declared_exported_prototyped("glomseg_lean.h", _lib.LEAN_PROTOTYPES, {"gs_espnet_plan_lean"})
    assert "Host-only" in text
    lib = _lib.load()
    out = ctypes.c_int(7)
    assert lib.gs_espnet_plan_lean(1, 64, 128, 2, 8, 5, 0, 256, 0, ctypes.byref(out)) == _lib.GS_OK and out.value == 1
    assert lib.gs_espnet_plan_lean(1, 64, 128, 2, 8, 5, 0, 256, 1, ctypes.byref(out)) == _lib.GS_OK and out.value == 0
    for bad in ((0, 64, 128, 2, 8, 5), (1, 12, 128, 2, 8, 5), (1, 64, 128, 2, 8, 21), (1, 64, 128, -1, 8, 5)):
        assert lib.gs_espnet_plan_lean(*bad, 0, 256, 0, ctypes.byref(out)) != _lib.GS_OK, bad
        assert lib.gs_last_error()
    assert lib.gs_espnet_plan_lean(1, 64, 128, 2, 8, 5, 0, 256, 0, None) != _lib.GS_OK


def test_the_store_flag_is_guarded():
    """F_CLS_ONLY drops the primary store of an F_CLS1X1 launch and nothing else: the kernel refuses it at compile time without the
    class sums, with a fused next 1x1 (whose block would read the map) or with a second store; only launch_l3_esp_last uses it."""
    with open(os.path.join(CSRC, "conv_mfma.h")) as fh:
        conv = fh.read()
    assert re.search(r"static_assert\(!\(FLAGS & F_CLS_ONLY\) \|\| \(CLSF && !\(FLAGS & \(F_FUSE1X1 \| F_DUAL\)\)\)", conv)
    assert "STORE1 = !(FLAGS & (F_NOSTORE | F_CLS_ONLY))" in conv
    with open(os.path.join(CSRC, "espnet.hip")) as fh:
        espnet = fh.read()
    uses = [m.start() for m in re.finditer(r"\bF_CLS_ONLY\b", espnet) if not espnet[:m.start()].rsplit("\n", 1)[-1].lstrip().startswith("//")]
    start = espnet.index("static gs_status launch_l3_esp_last(")
    end = espnet.index("\n}\n", start)
    # outside comments the flag is named where launch_l3_esp_last builds its modifier mask, once, and as a modifier the four forms
    # of that class may carry, once each: no other launch class, spec or launch site names it
    in_launch = [u for u in uses if start < u < end]
    in_specs = [u for u in uses if espnet[:u].rsplit("\n", 1)[-1].startswith("GS_SPEC(l3_esp_last::")]
    assert len(in_launch) == 1 and len(in_specs) == 4 and len(uses) == 5
    assert len(re.findall(r"^GS_SPEC\(l3_esp_last::", espnet, re.M)) == 4
