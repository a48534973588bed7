"""F_ODD_2B: the odd 25th input channel of the level-3 branch kernels on the two-block K = 1 matrix instruction.

With 25 real input channels on v_mfma_f32_32x32x2_f32 the 13th k-step of a tap multiplies channel 24 together with an all-zero
padding channel, once per pixel group of a wave.  Under F_ODD_2B (csrc/conv_mfma.h; switch CFG_L3_ODD_2B of espnet_config.h,
default 1) that step is ONE v_mfma_f32_32x32x1_2b_f32 per pair of pixel groups: block 0 the first group, block 1 the second,
the weights broadcast from block 0.  The dropped products are 0 x padding, so the arithmetic is the same and the two builds are
held to EQUAL ARRAYS (numpy's array_equal: -0 == +0 passes, nothing else does), not to a tolerance.

On the CPU: which forms may carry the flag and which do in this build (gs_espnet_form_odd_2b); the planner gives the cases'
forms at their batches; the off build reports itself through gs_build_flags.  On the GPU: helpers/odd_2b_cases.py's cases on
the shipped library here and on variants_so/libglomseg_odd2b_off.so in one child process -- level3_0, every level3.<i> the
engine still holds, level3_C, up_l3 and the logits of three tiles, mask and counts of the whole batch, after a forward with
logits and after a mask-only one (F_CLS_ONLY on the last block), and for one case a lane-1 forward between two lane-0 ones --
and the shipped library once against float64 with test_kernel_forms.py's TAU / bound(), imported, no new number.

Not every level-3 form with two or four pixel groups carries the flag: in the forms whose chunk is three row groups of thirteen
(CFG_L3_BR, CFG_L3_BR_P2F) the odd step's place is a run-time value, the step sits behind a wave-uniform branch, and hipcc
answers with hundreds of register copies and scratch (profiles/odd_2b_ab.txt); they keep the K = 2 step.  A case whose launch
runs such a form, or a one-group form, asserts that the flag is absent there -- the arrays are equal all the same.
"""
import json
import os
import subprocess
import sys
import tempfile

import numpy as np
import pytest

from helpers import odd_2b_cases as oc
from helpers.variant_builds import BUILD_TIMEOUT, CHILD_TIMEOUT, REPO, VARIANTS_DIR, faulted
from test_kernel_forms import batch_for, checked_images, form_table, plan

CASES = oc.cases()
OFF_LIB = os.path.join(VARIANTS_DIR, "libglomseg_%s.so" % oc.OFF_NAME)


def odd_table():
    """{(launch class, form name): gs_espnet_form_odd_2b's answer} of the shipped library"""
    from glomeruli_segmentation_amd import _lib
    from glomeruli_segmentation_amd.engine import forward_forms
    lib = _lib.load()
    return {(cls, name): lib.gs_espnet_form_odd_2b(k, f) for k, (cls, forms) in enumerate(forward_forms())
            for f, (name, _) in enumerate(forms)}


# ---------------------------------------------------------------------------------------------- CPU
def test_legality_table():
    """the flag is legal for, and built into, exactly the level-3 branch forms with two pixel groups per wave and a tap row per
    chunk: no one-group (P1R) form, no three-row-group form, no level-2 form, no reduce and no decoder form; past the table: -1"""
    from glomeruli_segmentation_amd import _lib
    table = odd_table()
    both = _lib.GS_FORM_ODD_2B_LEGAL | _lib.GS_FORM_ODD_2B_BUILT
    assert set(table) == {(cls, name) for cls, forms in form_table().items() for name in forms}
    assert {key for key, v in table.items() if v} == oc.FLAGGED
    assert all(table[key] == both for key in oc.FLAGGED)
    assert _lib.load().gs_build_flags() == 0
    for (cls, name), v in table.items():
        if not cls.startswith("l3_") or cls == "l3_reduce" or "P1R" in name:
            assert v == 0, (cls, name)
    lib = _lib.load()
    assert lib.gs_espnet_form_odd_2b(-1, 0) == lib.gs_espnet_form_odd_2b(len(form_table()), 0) == lib.gs_espnet_form_odd_2b(5, 6) == -1


def test_the_header_and_the_binding():
    from helpers.header_binding import assert_declared_exported_prototyped
    from glomeruli_segmentation_amd import _lib
    text = assert_declared_exported_prototyped("glomseg_forms.h", _lib.FORMS_PROTOTYPES, {"gs_espnet_form_odd_2b"})
    assert "#define GS_FORM_ODD_2B_LEGAL %d" % _lib.GS_FORM_ODD_2B_LEGAL in text and "#define GS_FORM_ODD_2B_BUILT %d" % _lib.GS_FORM_ODD_2B_BUILT in text
    with open(os.path.join(REPO, "include", "glomseg.h")) as fh:
        assert "#define GS_BUILD_NO_ODD_2B %d" % _lib.GS_BUILD_NO_ODD_2B in fh.read()


def test_the_switch_and_the_static_assert():
    """CFG_L3_ODD_2B ships as 1, and the kernel refuses the flag where the pairs or the compile-time step are missing"""
    import re
    csrc = os.path.join(REPO, "glomeruli_segmentation_amd", "csrc")
    with open(os.path.join(csrc, "espnet_config.h")) as fh:
        assert re.search(r"#ifndef CFG_L3_ODD_2B\n#define CFG_L3_ODD_2B 1\n", fh.read())
    with open(os.path.join(csrc, "conv_mfma.h")) as fh:
        text = fh.read()
    m = re.search(r"static_assert\(!ODD \|\| \((.*?)\),\s*\"F_ODD_2B", text, flags=re.S)
    assert m
    for clause in ("MT == 32", "TAPS == 9", "STRIDE == 1", "(P == 2 || P == 4)", "CINP % 2 == 0", "(G * M_KL_OF(MT)) % CINP == 0"):
        assert clause in m.group(1), clause


@pytest.mark.parametrize("case", CASES, ids=lambda c: c.name)
def test_cases_plan_the_two_pixel_forms(case):
    """at 256 CUs the case's batch is the smallest that plans its level-3 forms, with and without a logits request the same
    forms (the request decides F_CLS_ONLY, not the form), and below it the one-group forms run, which never carry the flag"""
    from glomeruli_segmentation_amd.engine import plan_lean
    assert batch_for(case, 256) == case.n256
    hit = plan(case.n256, case.H, case.W, case.p, case.q, case.classes, 256)
    assert {cls: hit[cls] for cls in oc.L3_CLASSES} == case.targets
    below = plan(case.n256 - 1, case.H, case.W, case.p, case.q, case.classes, 256)
    assert all(below[cls] == oc.P1R for cls in oc.L3_CLASSES)
    assert plan_lean(case.n256, case.H, case.W, case.p, case.q, case.classes, 256, want_logits=False)
    assert not plan_lean(case.n256, case.H, case.W, case.p, case.q, case.classes, 256, want_logits=True)
    table = odd_table()
    assert any(table[cls, form] for cls, form in case.targets.items()), "no launch of the case carries the flag"
    assert (case.W // 8) % 2 == 0 or all(f != oc.P2R for f in case.targets.values())


def test_cases_cover_the_flagged_forms():
    """the four flagged (launch class, form) pairs are each some case's target; the shapes are the issue's three and 8 x 66"""
    assert {(cls, form) for c in CASES for cls, form in c.targets.items()} >= oc.FLAGGED
    assert [(c.H // 8, c.W // 8) for c in CASES] == [(8, 65), (17, 33), (3, 12), (8, 66)]
    assert oc.LANES_CASE in [c.name for c in CASES] and len({c.name for c in CASES}) == len(CASES)


# ---------------------------------------------------------------------------------------------- the off build
@pytest.fixture(scope="module")
def off_lib():
    """variants_so/libglomseg_odd2b_off.so, built here where it is missing, stale or built with other flags; a build that
    cannot be done fails the tests that need it"""
    from glomeruli_segmentation_amd import build
    flags_file = OFF_LIB[:-3] + ".flags"
    want = " ".join(oc.OFF_FLAGS) + "\n"
    recorded = None
    if os.path.exists(flags_file):
        with open(flags_file) as fh:
            recorded = fh.read()
    build.build_lib(force=recorded != want, out=OFF_LIB, extra_flags=oc.OFF_FLAGS, timeout=BUILD_TIMEOUT)
    if recorded != want:
        with open(flags_file, "w") as fh:
            fh.write(want)
    return OFF_LIB


def child_env(lib):
    return dict(os.environ, GLOMSEG_LIB=lib, GLOMSEG_EXPERIMENT="1")


def test_the_off_build_reports_itself(off_lib):
    """a process that loads the -DCFG_L3_ODD_2B=0 build: gs_build_flags says GS_BUILD_NO_ODD_2B (and not GS_BUILD_DIAG), the
    flagged forms stay legal and are not built, and the planner's answers are the shipped library's"""
    from glomeruli_segmentation_amd import _lib
    code = ("import json, sys; sys.path[:0] = [%r, %r]\n"
            "from glomeruli_segmentation_amd import _lib\n"
            "from glomeruli_segmentation_amd.engine import forward_forms, plan_forward\n"
            "lib = _lib.load()\n"
            "odd = {'%%s|%%s' %% (cls, name): lib.gs_espnet_form_odd_2b(k, f) for k, (cls, forms) in enumerate(forward_forms()) for f, (name, _) in enumerate(forms)}\n"
            "print(json.dumps({'lib': _lib.LIB_PATH, 'flags': lib.gs_build_flags(), 'odd': odd, 'plan': plan_forward(65, 64, 528, 2, 3, 5, 256)}))\n"
            % (os.path.join(REPO, "tests"), REPO))
    res = subprocess.run([sys.executable] + (["-s"] if sys.flags.no_user_site else []) + ["-c", code], env=child_env(off_lib),
                         capture_output=True, text=True, timeout=CHILD_TIMEOUT, cwd=REPO)
    assert res.returncode == 0, res.stderr[-2000:]
    ans = json.loads(res.stdout.strip().splitlines()[-1])
    assert os.path.samefile(ans["lib"], off_lib) and not os.path.samefile(ans["lib"], _lib.LIB_PATH)
    assert ans["flags"] == _lib.GS_BUILD_NO_ODD_2B
    want = {"%s|%s" % key: (_lib.GS_FORM_ODD_2B_LEGAL if v else 0) for key, v in odd_table().items()}
    assert ans["odd"] == want
    assert ans["plan"] == plan(65, 64, 528, 2, 3, 5, 256)


# ---------------------------------------------------------------------------------------------- GPU
_GPU = {}


def off_arrays(off_lib):
    """(head line, {case: its line}, directory of the child's <case>.npz files): ONE child on the off build, started on first
    use.  A child that ran into its time limit, was killed, aborted or crashed fails every test that asks, and is not run again."""
    if "answer" not in _GPU:
        out_dir = tempfile.mkdtemp(prefix="odd2b_")
        cmd = [sys.executable] + (["-s"] if sys.flags.no_user_site else []) + [os.path.join(REPO, "tests", "helpers", "odd_2b_cases.py"), out_dir]
        try:
            res = subprocess.run(cmd, env=child_env(off_lib), capture_output=True, text=True, timeout=CHILD_TIMEOUT, cwd=REPO)
            status, stdout, tail = res.returncode, res.stdout, res.stdout[-2000:] + res.stderr[-3000:]
        except subprocess.TimeoutExpired as e:
            status, stdout, tail = 124, "", "no answer within %d s: %s" % (CHILD_TIMEOUT, (e.stderr or b"")[-2000:])
        lines = [json.loads(ln) for ln in stdout.splitlines() if ln.startswith("{")]
        _GPU["answer"] = (status, lines, tail, out_dir)
    status, lines, tail, out_dir = _GPU["answer"]
    assert not faulted(status), "the child on the off build ended with status %d: %s" % (status, tail)
    assert status == 0 and len(lines) == 1 + len(CASES), (status, tail)
    return lines[0], {ln["case"]: ln for ln in lines[1:]}, out_dir


@pytest.mark.gpu
@pytest.mark.parametrize("case", CASES, ids=lambda c: c.name)
def test_bits_equal_the_k2_step(case, off_lib):
    """every array of the case (helpers/odd_2b_cases.py, run_case) equal between the shipped library and the off build, both at
    the batch the device's CU count asks for, both planning the case's forms; and the tiles of the batch differ, so that the
    two pixel groups of a pair -- which always belong to one tile -- cannot be swapped unseen: tile contents differ along x"""
    import torch
    from glomeruli_segmentation_amd import _lib
    head, answers, out_dir = off_arrays(off_lib)
    assert os.path.samefile(head["lib"], off_lib) and head["build_flags"] == _lib.GS_BUILD_NO_ODD_2B
    assert _lib.load().gs_build_flags() == 0 and not os.path.samefile(_lib.LIB_PATH, off_lib)
    num_cus = torch.cuda.get_device_properties(0).multi_processor_count
    n = batch_for(case, num_cus)
    hit = plan(n, case.H, case.W, case.p, case.q, case.classes, num_cus)
    assert answers[case.name]["n"] == n and answers[case.name]["forms"] == hit and head["num_cus"] == num_cus
    assert all(hit[cls] == form for cls, form in case.targets.items())
    table = odd_table()
    carried = [cls for cls in oc.L3_CLASSES if table[cls, hit[cls]]]
    assert carried, hit
    got = oc.run_case(case, n)
    with np.load(os.path.join(out_dir, case.name + ".npz")) as z:
        assert sorted(z.files) == sorted(got)
        differ = [name for name in z.files if not (z[name].shape == got[name].shape and np.array_equal(z[name], got[name]))]
        zeros = [name for name in z.files if z[name].dtype == np.float32 and not
                 np.array_equal(np.signbit(z[name]), np.signbit(got[name]))]
    print("case %s: n %d, flag carried by %s, %d arrays, unequal %s, sign of a zero differs in %s" % (
        case.name, n, carried, len(got), differ, zeros))
    assert not differ, differ
    picks = checked_images(n)
    assert len(picks) >= 2 and not np.array_equal(got["level3_0/%d" % picks[0]], got["level3_0/%d" % picks[-1]])
    l3 = got["level3_0/%d" % picks[0]]
    half = min(32, l3.shape[2] // 2)
    assert not np.array_equal(l3[:, :, :half], l3[:, :, half:2 * half])      # the two pixel groups of a task hold other values
    if case.name == oc.LANES_CASE:      # lane 1 ran the reversed batch in its own workspace and left lane 0's results alone
        assert np.array_equal(got["lane1/mask"], got["mask"][::-1]) and np.array_equal(got["lane1/hist"], got["hist"][::-1])
        assert np.array_equal(got["again/mask"], got["mask"]) and np.array_equal(got["again/hist"], got["hist"])
        for k in picks:
            assert np.array_equal(got["lane1/logits/%d" % k], got["logits/%d" % k])
            assert np.array_equal(got["again/logits/%d" % k], got["logits/%d" % k])
            assert np.array_equal(got["again/level3_0/%d" % k], got["level3_0/%d" % k])
    assert np.array_equal(got["lean/mask"], got["mask"]) and np.array_equal(got["lean/hist"], got["hist"])


@pytest.mark.gpu
@pytest.mark.parametrize("case", CASES, ids=lambda c: c.name)
def test_flagged_forms_against_float64(case):
    """the shipped library on the case, once, under test_kernel_forms.py's float64 reference and bounds (DeviceCase.forward:
    every held stage and the logits of three tiles within bound(), argmax, counts, mask-only kernels, fault word)"""
    from test_kernel_forms import DeviceCase
    with DeviceCase(case) as dev:
        n = batch_for(case, dev.num_cus)
        dev.forward(n, checked_images(n))
