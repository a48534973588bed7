"""The cases of tests/test_odd_channel_2b.py and the run both of its sides make: python odd_2b_cases.py <out directory>

F_ODD_2B (csrc/conv_mfma.h) replaces the half-empty last k-step of a tap of the level-3 branch kernels by one two-block K = 1
matrix instruction; `-DCFG_L3_ODD_2B=0` rebuilds the K = 2 step.  The two libraries are held to EQUAL ARRAYS on these cases: the
pytest process runs them on the shipped library, a child process (this file as a script, GLOMSEG_LIB = the off build) on the
other, and the child leaves its arrays in <out directory>/<case>.npz.

A case is a test_kernel_forms.py Case: its targets are the level-3 branch forms a batch of n256 tiles takes at 256 CUs -- the
batch is raised, never the size, until the two-pixel forms are planned.  Level-3 maps of odd width (8 x 65, 17 x 33) cannot take
a vector form, so their down-sampler and fused blocks run CFG_L3_BR_P2F, which does not carry the flag, and their last block
CFG_L3_BR_P2, which does (lanes own pixel x of two 32-pixel runs); 3 x 12 and 8 x 66 take CFG_L3_BR_P2R+F_VEC (lanes own pixel
pairs) in all three launch classes.  8 x 65 is a full 64-pixel task and a one-pixel rest, 8 x 66 the same with the smallest rest
a vector form has, 17 x 33 is odd both ways, 3 x 12 is narrower than one pixel group and shorter than every dilation but d1
and d2.
"""
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
TESTS = os.path.dirname(HERE)
REPO = os.path.dirname(TESTS)
for path in (TESTS, REPO):
    if path not in sys.path:
        sys.path.insert(0, path)

OFF_NAME = "odd2b_off"
OFF_FLAGS = ("-DCFG_L3_ODD_2B=0",)
P2R, P2F, P2, P1R = "CFG_L3_BR_P2R+F_VEC", "CFG_L3_BR_P2F", "CFG_L3_BR_P2", "CFG_L3_BR_P1R"
FLAGGED = {("l3_down", P2R), ("l3_esp_fused", P2R), ("l3_esp_last", P2R), ("l3_esp_last", P2)}
L3_CLASSES = ("l3_down", "l3_esp_fused", "l3_esp_last")


def cases():
    from test_kernel_forms import Case
    lone = {"lone_row", "ragged_task"}
    return [
        Case("O1", "random", 5, 2, 3, 64, 520, 65, {"l3_down": P2F, "l3_esp_fused": P2F, "l3_esp_last": P2}, {"ragged_task"}),
        Case("O2", "random", 5, 2, 3, 136, 264, 61, {"l3_down": P2F, "l3_esp_fused": P2F, "l3_esp_last": P2}, lone),
        Case("O3", "fold1", 5, 2, 8, 24, 96, 342, {"l3_down": P2R, "l3_esp_fused": P2R, "l3_esp_last": P2R}, lone),
        Case("O4", "random", 5, 2, 3, 64, 528, 65, {"l3_down": P2R, "l3_esp_fused": P2R, "l3_esp_last": P2R}, {"ragged_task"}),
    ]


LANES_CASE = "O4"      # the case that also runs lane 1 between two lane-0 forwards


def stage_names(case, lean):
    """what gs_espnet_read_stage serves of level 3 after a forward with logits / a mask-only ("lean") one, whose last block
    stores no map"""
    blocks = ["level3.%d" % i for i in range(max(0, case.q - 2), case.q - (1 if lean else 0))]
    return ["level3_0"] + blocks + ["level3_C", "up_l3"]


def run_case(case, n):
    """{name: array} of the case's first n tiles on the library this process has loaded: the level-3 stages and the logits of
    checked_images(n) after a forward with logits, mask and counts of all n; the same stages, mask and counts after a mask-only
    forward (F_CLS_ONLY on the last block); for LANES_CASE also a lane-1 forward of the REVERSED batch between two lane-0 ones."""
    import numpy as np
    import torch
    import test_kernel_forms as tkf
    from glomeruli_segmentation_amd.engine import EspnetEngine
    sd, mean, std = tkf.case_weights(case)
    tiles = np.stack([tkf.case_tile(case, k) for k in range(n)])
    picks = tkf.checked_images(n)
    out = {}
    eng = EspnetEngine(sd, classes=case.classes, p=case.p, q=case.q, lanes=2 if case.name == LANES_CASE else 1)
    try:
        t = torch.from_numpy(tiles).cuda()
        mask, hist, logits = eng.segment(t, mean, std, want_logits=True)
        torch.cuda.synchronize()
        for k in picks:
            for name in stage_names(case, False):
                out["%s/%d" % (name, k)] = eng.read_stage(name, image=k)
            out["logits/%d" % k] = logits[k].cpu().numpy()
        out["mask"], out["hist"] = mask.cpu().numpy(), hist.cpu().numpy()
        if case.name == LANES_CASE:
            rev = torch.from_numpy(tiles[::-1].copy()).cuda()
            m1, h1, l1 = eng.segment(rev, mean, std, want_logits=True, lane=1)
            eng.wait_lanes()
            mask, hist, logits = eng.segment(t, mean, std, want_logits=True)
            torch.cuda.synchronize()
            out["lane1/mask"], out["lane1/hist"] = m1.cpu().numpy(), h1.cpu().numpy()
            out["again/mask"], out["again/hist"] = mask.cpu().numpy(), hist.cpu().numpy()
            for k in picks:
                out["lane1/logits/%d" % k] = l1[n - 1 - k].cpu().numpy()
                out["again/logits/%d" % k] = logits[k].cpu().numpy()
                out["again/level3_0/%d" % k] = eng.read_stage("level3_0", image=k)
        m2, h2, _ = eng.segment(t, mean, std)
        torch.cuda.synchronize()
        for k in picks:
            for name in stage_names(case, True):
                out["lean/%s/%d" % (name, k)] = eng.read_stage(name, image=k)
        out["lean/mask"], out["lean/hist"] = m2.cpu().numpy(), h2.cpu().numpy()
        eng.check_device_faults()
    finally:
        eng.close()
    return out


def main(out_dir):
    """the child: every case on the library under GLOMSEG_LIB, at the batch the device's CU count asks for; one JSON line each"""
    import numpy as np
    import torch
    import test_kernel_forms as tkf
    from glomeruli_segmentation_amd import _lib
    lib = _lib.load()
    num_cus = torch.cuda.get_device_properties(0).multi_processor_count
    print(json.dumps({"lib": _lib.LIB_PATH, "build_flags": lib.gs_build_flags(), "num_cus": num_cus}), flush=True)
    for case in cases():
        n = tkf.batch_for(case, num_cus)
        np.savez(os.path.join(out_dir, case.name + ".npz"), **run_case(case, n))
        print(json.dumps({"case": case.name, "n": n, "forms": tkf.plan(n, case.H, case.W, case.p, case.q, case.classes, num_cus)}), flush=True)
    return 0


if __name__ == "__main__":
    sys.exit(main(sys.argv[1]))
