"""The kernel forms behind build switches, run against float64.

test_kernel_forms.py holds every form the forward picks at the shipped defaults to a float64 reference, and pins six forms
(UNREACHABLE_AT_DEFAULTS) that the library enumerates, compiles and ships but no shape reaches.  Those, and the other value of
every switch of DESIGN.md's "Build switches" that changes a form or its arithmetic, run here: helpers/variant_builds.py holds
the table of variant builds (variants_so/libglomseg_<name>.so) and their cases, and helpers/variant_forms_child.py runs a
variant's cases in a process of its own -- this one has the shipped library loaded -- through test_kernel_forms.py's DeviceCase:
the same float64 reference, the same bounds TAU / bound(), no new number.

On the CPU: each variant's planner gives the cases' hand-written targets and batches, the variants together reach every pinned
form, every flipped switch has a case that runs a launch it changes, the child really loaded the variant (its path, its build
flags, a plan the shipped library does not give), and the bounds reject planted errors at every case's shape.  On the GPU: one
child per variant, one after the other, each GPU test reading its case's line; after a child that faulted or hung no other
child is started.
"""
import os

import pytest

from helpers import variant_builds as vb
from test_kernel_forms import UNREACHABLE_AT_DEFAULTS, bounds_discriminate, case_key, edges, form_table, output_width, plan
from test_kernel_forms_small import planted_errors

VARIANT_CASES = vb.variant_cases()
NAMES = [v.name for v in vb.VARIANTS]


def vcase_id(vc):
    return "%s-%s" % (vc.variant, vc.case.name)


@pytest.fixture(scope="module")
def variant_libs():
    """the three libraries, built here where one is missing or stale; a build that fails fails the tests that need it"""
    return {name: vb.ensure_built(name) for name in NAMES}


_PLANS = {}


@pytest.fixture(scope="module")
def planned(variant_libs):
    """variant -> (the child's first line, {case name: its line}) of mode `plan`, one child per variant"""
    for name in NAMES:
        if name not in _PLANS:
            status, lines, tail = vb.run_child(name, "plan")
            assert status == 0, (name, status, tail)
            assert len(lines) == 1 + len(vb.variant_cases(name)), (name, tail)
            _PLANS[name] = (lines[0], {ln["case"]: ln for ln in lines[1:]})
    return _PLANS


# ---------------------------------------------------------------------------------------------- the table
def test_the_table_of_cases():
    """about a dozen cases, each variant with a fold-1 case at (2, 8) and the issue's shapes, classes and depths; no two cases
    of any table share a seed"""
    from test_kernel_forms import CASES
    from test_kernel_forms_small import SMALL_CASES
    assert 12 <= len(VARIANT_CASES) <= 16
    names = [vc.case.name for vc in VARIANT_CASES]
    keys = [case_key(c) for c in CASES + SMALL_CASES] + [case_key(vc.case) for vc in VARIANT_CASES]
    assert len(set(names)) == len(names) and len(set(keys)) == len(keys)
    for name in NAMES:
        mine = [vc for vc in VARIANT_CASES if vc.variant == name]
        fold1 = [vc.case for vc in mine if vc.case.weights == "fold1"]
        assert len(fold1) == 1 and (fold1[0].classes, fold1[0].p, fold1[0].q) == (5, 2, 8), name
        assert all(vc.case.weights in ("fold1", "random") for vc in mine)
    assert {(vc.case.H, vc.case.W) for vc in VARIANT_CASES} == {(40, 160), (40, 136), (24, 96)}
    assert {vc.case.classes for vc in VARIANT_CASES} == {5, 7, 20}
    assert {(vc.case.p, vc.case.q) for vc in VARIANT_CASES} == {(2, 2), (2, 3), (1, 0), (0, 1), (0, 0), (2, 8)}
    for vc in VARIANT_CASES:
        assert vc.case.edges == edges(vc.case.H, vc.case.W) and vc.tiles >= 1, vc.case.name
    assert set(vb.BY_NAME) == set(NAMES) == {vc.variant for vc in VARIANT_CASES}


def test_every_switch_has_a_case():
    """every switch a variant flips names a launch class and the forms of it that show the other value, and a case of the
    variant runs one of them; vector forms only at widths their pixels per lane divide"""
    table = form_table()
    flipped = set()
    for v in vb.VARIANTS:
        assert len(v.switches) == len([f for f in v.flags if f.startswith("-DCFG_")]) or v.name == "novec"
        for switch, (cls, forms) in v.switches.items():
            flipped.add(switch.split("=")[0])
            assert v.name == "novec" or "-D" + switch in v.flags, switch
            assert set(forms) <= set(table[cls]), (switch, cls)
            hit = [vc.case.name for vc in vb.variant_cases(v.name) if vc.case.targets.get(cls) in forms]
            assert hit, (v.name, switch, cls)
    # DESIGN.md's switches that change a form or its arithmetic (the ring depths, CFG_STAGE_ROT, POL_* and *_XFLAGS do not)
    assert flipped == {"CFG_FUSE_L2", "CFG_FUSE_L3", "CFG_SKIP_PAD", "CFG_S2_FLIP", "CFG_SMALL2_WAVES", "CFG_SMALL3_WAVES",
                       "CFG_SMALL_AGL", "CFG_L2_DOWN_SKIP", "CFG_L3_DOWN_P2", "CFG_L3_LAST_P2", "GS_NO_VEC"}
    both = [v.name for v in vb.VARIANTS for f in v.flags if f.startswith("-DCFG_FUSE_L3=")]
    assert sorted(both) == ["alt", "unfused"]       # CFG_FUSE_L3 has two other values: 1 and 0
    # the two the issue singles out: an n = 1 run for CFG_SMALL_AGL = 0, a level-3 half-row form for CFG_SKIP_PAD = 0
    unfused = vb.variant_cases("unfused")
    assert any(vc.tiles == 1 and vc.case.n256 == 1 and vc.case.targets.get("l3_esp_last") == "CFG_L3_BR_P1R" for vc in unfused)
    assert any(vc.case.targets.get("l3_esp_last") == "CFG_L3_BR_P2R+F_VEC" for vc in unfused)
    for vc in VARIANT_CASES:
        for cls, form in vc.case.targets.items():
            P = table[cls][form]
            assert not P or output_width(cls, vc.case.W) % P == 0, (vc.case.name, cls, form, P)


def test_pinned_forms_have_a_case():
    """every form pinned as unreachable at the defaults is the target of the variant case named for it"""
    assert len(UNREACHABLE_AT_DEFAULTS) == 6
    by_name = {(vc.variant, vc.case.name): vc.case for vc in VARIANT_CASES}
    for (cls, form), (_, variant, name) in UNREACHABLE_AT_DEFAULTS.items():
        assert by_name[variant, name].targets[cls] == form, (cls, form, variant, name)


# ---------------------------------------------------------------------------------------------- the variants' planners
def test_variant_planners_give_the_cases(planned):
    """each variant's planner, asked in a process that loaded that variant: the smallest batch that takes a case's targets on
    256 CUs is its n256, the plan there is the case's targets -- the whole answer -- and so is the plan at the batch a run takes"""
    for name in NAMES:
        head, lines = planned[name]
        for vc in vb.variant_cases(name):
            ln = lines[vc.case.name]
            assert ln["n256"] == vc.case.n256, (name, vc.case.name, ln)
            assert ln["plan"] == vc.case.targets, (name, vc.case.name, ln["plan"])
            assert ln["plan_at_tiles"] == vc.case.targets, (name, vc.case.name, ln["plan_at_tiles"])


def test_variants_reach_every_pinned_form(planned):
    reached = set()
    for name in NAMES:
        reached.update(tuple(cf) for cf in planned[name][0]["reached"])
    enumerated = {(cls, form) for cls, forms in form_table().items() for form in forms}
    assert reached <= enumerated
    assert set(UNREACHABLE_AT_DEFAULTS) <= reached, sorted(set(UNREACHABLE_AT_DEFAULTS) - reached)


def test_the_child_loaded_the_variant(planned, variant_libs):
    """not the shipped library under another name: the child's _lib.LIB_PATH is the variant's file, GS_BUILD_DIAG is set for
    novec alone, and on at least one of its cases each variant plans what the shipped library (loaded here) does not"""
    from glomeruli_segmentation_amd import _lib
    assert _lib.LIB_PATH == os.path.join(os.path.dirname(_lib.__file__), "libglomseg.so") and _lib.load().gs_build_flags() == 0
    for name in NAMES:
        head, lines = planned[name]
        assert os.path.samefile(head["lib"], variant_libs[name]) and not os.path.samefile(head["lib"], _lib.LIB_PATH)
        assert head["build_flags"] == (_lib.GS_BUILD_DIAG if name == "novec" else 0), name
        differ = [vc.case.name for vc in vb.variant_cases(name)
                  if plan(vc.case.n256, vc.case.H, vc.case.W, vc.case.p, vc.case.q, vc.case.classes, 256) != lines[vc.case.name]["plan"]]
        assert differ, name


def test_diag_build_is_refused_without_the_opt_in(variant_libs):
    status, lines, tail = vb.run_child("novec", "plan", env_without=("GLOMSEG_ALLOW_DIAG",))
    assert status != 0 and not lines and "GLOMSEG_ALLOW_DIAG=1" in tail, (status, tail)


# ---------------------------------------------------------------------------------------------- bounds
@pytest.mark.parametrize("vc", VARIANT_CASES, ids=vcase_id)
def test_bounds_discriminate_on_variant_cases(vc):
    """test_bounds_discriminate at the variant cases' shapes: the fp32 C oracle passes every stage bound, and the bounds
    reject a 1e-4 bump of one element of any stage, the zeroed bottom tap row of the widest level-3 dilation some row still
    reads (what a wrong tap sign or a wrong F_SKIP_PAD decision in a CFG_L3_BR form amounts to) and a dropped K-tail channel."""
    bounds_discriminate(vc.case, planted_errors(vc.case))


# ---------------------------------------------------------------------------------------------- the GPU cases
_GPU = {"faulted": None, "answers": {}}


def gpu_answers(name):
    """{case name: its line} of the variant's one GPU child, started on first use.  A child that ran into its time limit, was
    killed, aborted, crashed or gave up after an error of the device stops the module: no other child is started."""
    if name not in _GPU["answers"]:
        assert _GPU["faulted"] is None, "not started: the GPU child of variant %s ended with %s" % _GPU["faulted"]
        vb.ensure_built(name)
        status, lines, tail = vb.run_child(name, "gpu")
        if vb.faulted(status) or status == vb.CHILD_GAVE_UP:
            _GPU["faulted"] = (name, "status %d: %s" % (status, tail))
        _GPU["answers"][name] = (status, {ln["case"]: ln for ln in lines}, tail)
    return _GPU["answers"][name]


@pytest.mark.gpu
@pytest.mark.parametrize("vc", VARIANT_CASES, ids=vcase_id)
def test_variant_form_against_float64(vc):
    """The case on the variant's library (DeviceCase.forward in the child): every held stage and the logits of the checked
    tiles within bound() of float64, mask, counts, mask-only kernels and fault word as there -- and the forms run were the
    case's targets, by the variant's own library."""
    status, answers, tail = gpu_answers(vc.variant)
    ln = answers.get(vc.case.name)
    assert ln is not None, "variant %s: the child (status %d) gave no answer for case %s: %s" % (vc.variant, status, vc.case.name, tail)
    print("variant %s case %s: n %s on %s CUs, worst error / bound %s: %s" % (vc.variant, vc.case.name, ln.get("n"), ln.get("num_cus"),
                                                                             ln.get("ratio"), ln.get("worst")))
    assert ln["ok"], ln.get("error")
    assert ln["lib"] == vb.lib_path(vc.variant) and ln["n"] >= vc.tiles
    assert all(ln["forms"].get(cls) == form for cls, form in vc.case.targets.items()), ln["forms"]
    assert ln["ratio"] is not None and ln["ratio"] <= 1.0
