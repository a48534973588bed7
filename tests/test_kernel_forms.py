"""Every kernel form forward_impl (csrc/espnet.hip) can pick, checked against a float64 reference.

forward_impl does not run one kernel per layer: per launch class it runs the form that plan_forward (csrc/forward_plan.h)
picks from the batch size, the tile size and the device's CU count.  The tests ask the library for that plan
(engine.plan_forward: gs_espnet_plan_forward, the function the forward itself calls): CASES holds known answers for it,
written by hand; test_cases_cover_every_form makes the GPU cases reach every form a sweep of the planner returns;
test_vector_forms_fit_the_width holds the one planner mistake that would become an out-of-bounds access on a card; and each
GPU case checks three tiles of its batch -- every stage the engine still holds after the forward, the logits, the mask and
the counts -- against oracle/espnet_torch_port.py run in float64.

One bound per stage: max|got - ref64| <= tau * max(1, max|ref64|).  test_bounds_discriminate shows on the CPU that the
fp32 C oracle passes them on every case's shape, and that they reject a 1e-4 change of one element in a stage's last
column, a zeroed d16 tap row and a dropped K-tail channel.
"""
import ctypes
import os
import re
from collections import namedtuple
from functools import lru_cache

import numpy as np
import pytest

from conftest import REPO, load_weights, random_state_dict
from test_gpu_parity import DEC_STAGE_TOL, ENC_STAGE_TOL, LOGIT_TOL

CSRC = os.path.join(REPO, "glomeruli_segmentation_amd", "csrc")
RANDOM_MEAN_STD = ((120.0, 130.0, 110.0), (60.0, 55.0, 70.0))

# ---------------------------------------------------------------------------------------------- the plan
# the shipped defaults of espnet_config.h (the two fusion switches: espnet_facts.h) the planner reads (test_dispatch_tripwire pins each one): CASES and
# UNREACHABLE_AT_DEFAULTS are answers for these values
CONFIG = {"CFG_SMALL2_WAVES": 4, "CFG_SMALL3_WAVES": 8, "CFG_L3_DOWN_P2": 1, "CFG_L3_LAST_P2": 1,
          "CFG_L2_DOWN_SKIP": 1, "CFG_FUSE_L2": 1, "CFG_FUSE_L3": 2}
L2SP = 4    # `constexpr int L2SP` there: pixels per lane of the level-2 branch kernels
# switches whose A/B was lost: removed from the sources, none of these names may come back under csrc/
DELETED = ("F_EPI_PIPE", "CFG_EPI_SPLIT", "CFG_EPI_PRIO", "CFG_EPI_PRELOAD", "CFG_REFILL_MID", "CFG_L3_W16",
           "CFG_L3_FUSE_P4", "CFG_AGL_", "CFG_SKIP_PAD_L2", "CFG_RES_RING_DIV", "CFG_RES_TOP", "CFG_L2_MINW", "CFG_LAZY_B2",
           "CFG_L2_C1S_REV", "rev_n", "F_XMERGE", "wconv_xm",
           # the switches that sat outside the table's three headers, with no variant build and no test behind their other value
           "STEM_DWORD", "STEM_LUT_COPIES", "stem_fetch", "NT_STEM_ST", "NT_DEC1_LD", "NT_DEC2_LD", "NT_DEC3_ST", "NT_DEC4_ST",
           "DT_PRIO", "DT_MAIN_WAVES", "CFG_SHORT_LIST_SPLIT")
# the forms the library enumerates and no shape reaches with the shipped defaults, each with the switch that keeps it away
# (found by the sweep of reachable_forms; test_every_enumerated_form_is_accounted_for), and the variant build and case of
# test_variant_forms.py (helpers/variant_builds.py) that runs it against float64 all the same
UNREACHABLE_AT_DEFAULTS = {
    ("l2_down", "CFG_L2_BR_P4+F_VEC"): ("CFG_L2_DOWN_SKIP = 1 takes every width that is a multiple of four first", "alt", "K1"),
    ("l2_esp_fused", "unfused CFG_L2_BR_P4+F_VEC"): ("CFG_FUSE_L2 = 1: every block but the last computes the next 1x1 (the block hook runs it)",
                                                     "unfused", "M1"),
    ("l2_esp_fused", "unfused CFG_L2_BR_P4"): ("CFG_FUSE_L2 = 1 (the block hook runs it)", "unfused", "M2"),
    ("l3_down", "CFG_L3_BR+F_VEC"): ("CFG_L3_DOWN_P2 = 1 takes every even width first", "alt", "K2"),
    ("l3_esp_last", "CFG_L3_BR+F_VEC"): ("CFG_L3_LAST_P2 = 1 takes every even width first (the block hook runs it)", "alt", "K1"),
    ("dec_conv", "MFMA MT32"): ("no switch: tile widths are multiples of 8, so W/2 is always a multiple of the four pixels per lane "
                                "(GS_NO_VEC of a -DGS_DIAG build runs it)", "novec", "N1"),
}


def plan(n, H, W, p, q, classes, num_cus):
    """launch class -> the form a forward runs for it, from the library's planner"""
    from glomeruli_segmentation_amd.engine import plan_forward
    return plan_forward(n, H, W, p, q, classes, num_cus)


@lru_cache(maxsize=None)
def form_table():
    """{launch class: {form name: pixels per lane}} as the library enumerates it"""
    from glomeruli_segmentation_amd.engine import forward_forms
    return {cls: dict(forms) for cls, forms in forward_forms()}


def padded_classes(classes):
    """Model::cp, for engine_stages: the class planes the decoder's stages are stored with"""
    return 5 if classes == 5 else -(-classes // 4) * 4


def output_width(launch_class, W):
    """the width of the activation a launch class writes: level 2 and dec3 at 1/4, level 3 at 1/8, the decoder conv at 1/2"""
    return W // 2 if launch_class == "dec_conv" else W // 8 if launch_class.startswith("l3_") else W // 4


def edges(H, W):
    """the shape edges of the large forms: a lone last row of the level-3 stride-2 reduce's row pairs (odd H/8) and a
    ragged last 64-pixel level-3 task (W/8 not a multiple of 64)"""
    out = set()
    if (H // 8) % 2:
        out.add("lone_row")
    if (W // 8) % 64:
        out.add("ragged_task")
    return out


def _read(name):
    with open(os.path.join(CSRC, name)) as fh:
        return fh.read()


def test_dispatch_tripwire():
    """CASES and UNREACHABLE_AT_DEFAULTS are answers for the shipped defaults: a changed default fails here, so that they are
    revisited with it.  Deleted switches stay deleted, and every switch left anywhere under csrc/ is documented."""
    cfg = _read("espnet_config.h") + _read("espnet_facts.h")   # (CFG_FUSE_L2 / CFG_FUSE_L3: the weight packer reads them too)
    for name, value in CONFIG.items():
        m = re.search(r"#ifndef %s\n#define %s (\S+)" % (name, name), cfg)
        assert m and m.group(1) == str(value), name
    m = re.search(r"constexpr int L2SP = (\d+);", cfg)
    assert m and int(m.group(1)) == L2SP
    # the switches that lost their A/B stay deleted ...
    sources = [f for f in sorted(os.listdir(CSRC)) if f.endswith((".h", ".hip", ".inc", ".cpp", ".cu", ".txt"))]
    assert len(sources) >= 10
    for fname in sources:
        text = _read(fname)
        for name in DELETED:   # whole identifiers (`prev_n` is not `rev_n`); a name ending in "_" is a prefix
            pattern = r"\b%s" % re.escape(name) + ("" if name.endswith("_") else r"\b")
            assert not re.search(pattern, text), (fname, name)
    # ... and a default nobody documents cannot ship: every overridable macro left anywhere under csrc/ (include guards, names
    # ending in _H, apart) is named in the Build switches table of DESIGN.md's kernel section, and the table names nothing else
    with open(os.path.join(REPO, "DESIGN.md")) as fh:
        design = fh.read()
    kernels = design[design.index("\n## 4. Kernels"):design.index("\n## 5. ")]
    table = re.search(r"\n### Build switches\n(?:[^|\n][^\n]*\n|\n)*((?:\|[^\n]*\n)+)", kernels).group(1)   # the section's first table
    macros = [m for f in sources if f.endswith((".h", ".hip", ".inc", ".cpp"))
              for m in re.findall(r"#ifndef (\w+)\n#define \1\b", _read(f)) if not m.endswith("_H")]
    assert len(macros) >= 20 and len(set(macros)) == len(macros)
    for name in macros:
        assert "`%s`" % name in table, name
    listed = [name for row in table.splitlines()[2:] for name in re.findall(r"`(\w+)`", row.split("|")[1])]
    assert len(listed) >= 20 and set(listed) == set(macros), sorted(set(listed) ^ set(macros))


# ---------------------------------------------------------------------------------------------- the cases
Case = namedtuple("Case", "name weights classes p q H W n256 targets edges")
L2_SMALL, L3_SMALL = "CFG_L2_BR_P2S+F_VEC", "CFG_L3_BR_P1R"
L2_SKIP, L2_VEC, P2R = "CFG_L2_BR_P4S+F_VEC+F_SKIP_PAD", "CFG_L2_BR_P4+F_VEC", "CFG_L3_BR_P2R+F_VEC"
CASES = [
    Case("A", "fold1", 5, 2, 8, 512, 1024, 1,       # every small-batch form at full size
         {"l2_down": L2_SMALL, "l2_esp_fused": L2_SMALL, "l2_esp_last": L2_SMALL, "l3_reduce": "CFG_L3_C1S_BNL_P1",
          "l3_down": L3_SMALL, "l3_esp_fused": L3_SMALL, "l3_esp_last": L3_SMALL}, set()),
    Case("B", "fold1", 5, 2, 8, 512, 1024, 9,       # the headline forms
         {"l2_down": L2_SKIP, "l2_esp_fused": L2_VEC, "l2_esp_last": L2_VEC, "l3_reduce": "CFG_L3_C1S_BNL",
          "l3_down": P2R, "l3_esp_fused": P2R, "l3_esp_last": P2R}, set()),
    Case("C", "fold1", 5, 2, 8, 264, 1000, 16,      # H/8 = 33, W/8 = 125: the odd-width forms, non-vector level 2
         {"l2_down": "CFG_L2_BR_P4", "l2_esp_fused": "CFG_L2_BR_P4", "l2_esp_last": "CFG_L2_BR_P4",
          "l3_reduce": "CFG_L3_C1S_BNL", "l3_down": "CFG_L3_BR_P2F", "l3_esp_fused": "CFG_L3_BR_P2F",
          "l3_esp_last": "CFG_L3_BR_P2"}, {"lone_row", "ragged_task"}),
    Case("D", "fold1", 5, 2, 8, 136, 1040, 21,      # W/8 = 130 = 2 * 64 + 2, H/8 = 17
         {"l2_down": L2_SKIP, "l3_reduce": "CFG_L3_C1S_BNL", "l3_down": P2R, "l3_esp_fused": P2R, "l3_esp_last": P2R},
         {"lone_row", "ragged_task"}),
    Case("E", "random", 20, 2, 3, 512, 1024, 9,     # the MT 32 decoder forms at a large batch
         {"l3_reduce": "CFG_L3_C1S_BNL", "l3_esp_fused": P2R, "dec3": "MFMA MT32+F_VEC",
          "dec_conv": "MFMA MT32+F_VEC"}, set()),
    Case("F", "random", 12, 2, 2, 264, 1000, 16,    # MFMA dec3, non-vector MT 16 decoder convs
         {"l3_reduce": "CFG_L3_C1S_BNL", "l3_down": "CFG_L3_BR_P2F", "dec3": "MFMA MT16", "dec_conv": "MFMA MT16"},
         {"lone_row", "ragged_task"}),
    Case("G", "random", 7, 0, 1, 264, 1000, 16,     # p = 0: unfused b2, non-lazy stride-2 reduce; the only L3 block is the last
         {"l2_down": "unfused CFG_L2_BR_P4", "cat_b2": "cat_b2_kernel", "l3_reduce": "CFG_L3_C1S",
          "l3_down": "CFG_L3_BR_P2F", "l3_esp_last": "CFG_L3_BR_P2", "dec3": "dec3_kernel", "dec_conv": "MFMA MT16"},
         {"lone_row", "ragged_task"}),
    Case("H", "random", 5, 3, 0, 512, 1024, 9,      # q = 0: the unfused level-3 down-sampler
         {"l2_down": L2_SKIP, "l3_reduce": "CFG_L3_C1S_BNL", "l3_down": "unfused CFG_L3_BR+F_VEC"}, set()),
    Case("I", "random", 16, 0, 2, 512, 1024, 9,     # the vector forms of the unfused level-2 down-sampler and of MT 16
         {"l2_down": "unfused CFG_L2_BR_P4+F_VEC", "l3_down": P2R, "dec3": "MFMA MT16+F_VEC",
          "dec_conv": "MFMA MT16+F_VEC"}, set()),
    Case("J", "random", 20, 1, 0, 264, 1000, 16,    # the non-vector unfused level-3 down-sampler and MT 32 dec3
         {"l2_esp_last": "CFG_L2_BR_P4", "l3_reduce": "CFG_L3_C1S_BNL", "l3_down": "unfused CFG_L3_BR",
          "dec3": "MFMA MT32", "dec_conv": "MFMA MT32+F_VEC"}, {"lone_row", "ragged_task"}),
]


def batch_for(case, num_cus):
    """the smallest batch whose launches take the case's target forms on a device with num_cus CUs"""
    for n in range(1, 8 * num_cus + 1):
        f = plan(n, case.H, case.W, case.p, case.q, case.classes, num_cus)
        if all(f.get(k) == v for k, v in case.targets.items()):
            return n
    raise AssertionError("case %s: no batch reaches %s on %d CUs" % (case.name, case.targets, num_cus))


SWEEP_DEPTHS = ((0, 0), (0, 1), (0, 2), (1, 0), (1, 1), (2, 2), (2, 8), (3, 0))
SWEEP_CLASSES = (2, 5, 7, 12, 16, 20)
SWEEP_BATCHES = (1, 2, 4, 9, 16, 21, 32)
SWEEP_HEIGHTS = (8, 136, 264, 512)


@lru_cache(maxsize=None)
def sweep(num_cus, heights=SWEEP_HEIGHTS, batches=SWEEP_BATCHES):
    """[(W, plan)] at legal tile sizes (multiples of 8), depths and class counts"""
    out = []
    for n in batches:
        for H in heights:
            for W in range(8, 1048, 8):
                for p, q in SWEEP_DEPTHS:
                    for classes in SWEEP_CLASSES:
                        out.append((W, plan(n, H, W, p, q, classes, num_cus)))
    return out


def reachable_forms(num_cus, heights=SWEEP_HEIGHTS, batches=SWEEP_BATCHES):
    """every (launch class, form) the planner returns over the sweep"""
    out = set()
    for _, f in sweep(num_cus, heights, batches):
        out.update(f.items())
    return out


def test_case_batches_at_256_cus():
    assert {c.name: batch_for(c, 256) for c in CASES} == {c.name: c.n256 for c in CASES}
    for c in CASES:
        assert c.edges <= edges(c.H, c.W), c.name


def test_cases_cover_every_form():
    hit = set()
    for c in CASES:
        hit.update(plan(batch_for(c, 256), c.H, c.W, c.p, c.q, c.classes, 256).items())
    every = reachable_forms(256)
    assert hit == every, ("not covered: %s" % sorted(every - hit), "not reachable: %s" % sorted(hit - every))


def test_vector_forms_fit_the_width():
    """A form with a vector pixel mapping (pixels per lane P > 0 in the library's table) is planned only when its launch
    class's output width is a multiple of P: lanes of such a kernel store P pixels at once, so anything else writes past a
    row.  Over the sweep, and over every width 8..1040 at one tile and at 32."""
    table = form_table()
    plans = list(sweep(256))
    for n in (1, 32):
        for W in range(8, 1048, 8):
            for p, q in ((0, 0), (2, 8)):
                for classes in (5, 16, 20):
                    plans.append((W, plan(n, 512, W, p, q, classes, 256)))
    vector = 0
    for W, f in plans:
        for cls, form in f.items():
            P = table[cls][form]
            assert P >= 0
            if P:
                vector += 1
                assert output_width(cls, W) % P == 0, (cls, form, W, P)
    assert vector > len(plans)      # (the check is not vacuous: most plans hold several vector forms)
    # every form named "+F_VEC" reports its P, and no other form reports one
    for cls, forms in table.items():
        for form, P in forms.items():
            assert (P > 0) == ("+F_VEC" in form), (cls, form, P)


def test_every_enumerated_form_is_accounted_for():
    """every (launch class, form) of the library's table is reached by the sweep or pinned, with the switch that gates it, in
    UNREACHABLE_AT_DEFAULTS -- and nothing pinned there is reachable"""
    enumerated = {(cls, form) for cls, forms in form_table().items() for form in forms}
    assert {cls for cls, _ in enumerated} == {"l2_down", "l2_esp_fused", "l2_esp_last", "cat_b2", "l3_reduce", "l3_down",
                                              "l3_esp_fused", "l3_esp_last", "dec3", "dec_conv"}
    reached = reachable_forms(256)
    assert reached <= enumerated, sorted(reached - enumerated)
    assert enumerated - reached == set(UNREACHABLE_AT_DEFAULTS), sorted((enumerated - reached) ^ set(UNREACHABLE_AT_DEFAULTS))
    # ... and every pinned form names the switch that keeps it away and a variant case that exists and has it as a target
    from helpers.variant_builds import BY_NAME, variant_cases
    for (cls, form), (why, variant, name) in UNREACHABLE_AT_DEFAULTS.items():
        assert why and variant in BY_NAME, (cls, form)
        named = [vc.case for vc in variant_cases(variant) if vc.case.name == name]
        assert len(named) == 1 and named[0].targets.get(cls) == form, (cls, form, variant, name)


def test_plan_refuses_bad_arguments():
    """the entry applies the forward's own rules: a positive batch, sizes that are positive multiples of 8, 2..20 classes"""
    from glomeruli_segmentation_amd import _lib
    lib = _lib.load()
    count = ctypes.c_int()

    def status(n=1, H=512, W=1024, p=2, q=8, classes=5, num_cus=256):
        return lib.gs_espnet_plan_forward(n, H, W, p, q, classes, num_cus, None, 0, ctypes.byref(count))
    assert status() == _lib.GS_OK and count.value == len(form_table()) == 10
    for bad in ({"n": 0}, {"n": -1}, {"H": 0}, {"W": 0}, {"H": 4}, {"H": 508}, {"W": 1028}, {"W": 1001}, {"H": -8},
                {"classes": 1}, {"classes": 21}, {"classes": 0}, {"p": -1}, {"q": -1}, {"num_cus": 0}):
        assert status(**bad) != _lib.GS_OK, bad
        assert lib.gs_last_error()
    for ok in ({"classes": 2}, {"classes": 20}, {"H": 8, "W": 8}, {"p": 0, "q": 0}):
        assert status(**ok) == _lib.GS_OK, ok
    codes = (ctypes.c_int * 10)()
    assert lib.gs_espnet_plan_forward(1, 512, 1024, 2, 8, 5, 256, codes, 9, ctypes.byref(count)) != _lib.GS_OK      # too little room
    assert lib.gs_espnet_plan_forward(1, 512, 1024, 2, 8, 5, 256, codes, 10, ctypes.byref(count)) == _lib.GS_OK
    # the enumeration ends with GS_ERR_INVALID
    name, P = ctypes.c_char_p(), ctypes.c_int()
    for k, f in ((10, 0), (10, -1), (-1, 0), (0, -2), (3, 1)):                            # (cat_b2, class 3, has one form)
        assert lib.gs_espnet_form_info(k, f, ctypes.byref(name), ctypes.byref(P)) == 1, (k, f)
    assert lib.gs_espnet_form_info(3, 0, ctypes.byref(name), ctypes.byref(P)) == _lib.GS_OK and name.value == b"cat_b2_kernel"
    assert lib.gs_espnet_form_info(3, -1, ctypes.byref(name), ctypes.byref(P)) == _lib.GS_OK and name.value == b"cat_b2"


def case_key(case):
    """the number a case's seeds are made of: the letter of a one-letter name; of a name like "S3" (the small-map cases of
    test_kernel_forms_small.py, whose batches run to thousands of tiles) a number past every letter, 32 apart, so that no
    two cases share a tile seed either"""
    if len(case.name) == 1:
        return ord(case.name)
    return 256 * ord(case.name[0]) + 32 * int(case.name[1:])


def case_weights(case):
    from glomeruli_segmentation_amd.synth import FOLD_MEAN_STD
    if case.weights == "fold1":
        mean, std = FOLD_MEAN_STD[1]
        return load_weights(1), mean, std
    mean, std = RANDOM_MEAN_STD
    sd = random_state_dict(case.p, case.q, classes=case.classes, seed=4000 + case_key(case))
    if case.weights == "edge":      # trained-range and limit PReLU slopes, negative and zero BN weights (helpers/edge_weights.py)
        from helpers.edge_weights import edge_state_dict
        sd = edge_state_dict(sd)
    else:
        assert case.weights == "random", case.weights
    return sd, mean, std


def case_tile(case, k):
    """tile k of the case's batch: synthetic in even slots, noise in odd ones, no seed used twice"""
    from glomeruli_segmentation_amd.synth import noise_tile, synth_tile
    return (noise_tile if k % 2 else synth_tile)(100 * case_key(case) + k, case.H, case.W)


def checked_images(n):
    """the first, the last and a middle noise tile"""
    return sorted({0, min((n // 2) | 1, n - 1), n - 1})


def engine_stages(case):
    """the stages EspnetEngine.read_stage still holds after a forward: forward_impl drops a stage when its ping-pong buffer
    is written again (level2.<i>, level3.<i>), the last level-2 block stores only into b2, and combine_t exists when the
    class count needs no padding planes"""
    p, q = case.p, case.q
    names = ["b1", "sample2", "level2_0"] + ["level2.%d" % i for i in range(max(0, p - 3), p - 1)]
    names += ["b2", "level3_0"] + ["level3.%d" % i for i in range(max(0, q - 2), q)] + ["up_l3"]
    if padded_classes(case.classes) == case.classes:
        names.append("combine_t")
    return names + ["up_l2", "conv"]


def reference(case, sd, mean, std, tiles):
    """float64 stages (engine_stages) and logits of uint8 tiles [k,H,W,3], each [k,C,h,w]"""
    from oracle import espnet_torch_port as port
    stages = {}
    logits = port.forward64(tiles, sd, mean, std, case.p, case.q, stages)
    out = {name: stages[name].numpy() for name in engine_stages(case)}
    out["logits"] = logits.numpy()
    return out


# ---------------------------------------------------------------------------------------------- bounds
# tau per stage family, relative to max(1, max|ref64|): about four times the fp32 C oracle's own worst error against
# float64 over all the cases' shapes, a synthetic and a noise tile each (measured: sample2 4e-9, b1 4.5e-7, level-2
# stages and b2 <= 1.7e-6, everything after <= 3.2e-6).  The fold-1 cases are also held to test_gpu_parity's absolute
# bounds.
TAU = {"sample2": 2e-8, "b1": 2e-6, "level2_0": 6e-6, "level2": 6e-6, "b2": 6e-6, "level3_0": 1.2e-5, "level3": 1.2e-5,
       "up_l3": 1.2e-5, "combine_t": 1.2e-5, "up_l2": 1.2e-5, "conv": 1.2e-5, "logits": 1.2e-5}
DECODER_STAGES = ("up_l3", "combine_t", "up_l2", "conv")


def bound(case, name, ref):
    b = TAU[name.split(".")[0]] * max(1.0, float(np.abs(ref).max()))
    if case.weights == "fold1":
        b = min(b, LOGIT_TOL if name == "logits" else DEC_STAGE_TOL if name in DECODER_STAGES else ENC_STAGE_TOL)
    return b


def stage_errors(case, got, ref):
    """name -> (max|got - ref|, bound) for every stage of ref"""
    out = {}
    for name, r in ref.items():
        g = np.asarray(got[name], dtype=np.float64)
        assert g.shape == r.shape, (case.name, name, g.shape, r.shape)
        out[name] = (float(np.abs(g - r).max()), bound(case, name, r))
    return out


def over(errors):
    return {name: eb for name, eb in errors.items() if not eb[0] <= eb[1]}


D16_ROW2_AND_K_TAIL = (("d16.conv.weight", (slice(None), slice(None), 2)), ("c1.conv.weight", (slice(None), -1)))


def bounds_discriminate(case, planted=D16_ROW2_AND_K_TAIL):
    """The body of test_bounds_discriminate for one case.  planted: (weight of the first level-3 block, the part to zero) per
    planted weight error."""
    from oracle import espnet_oracle as orc
    sd, mean, std = case_weights(case)
    tile = case_tile(case, 0)
    ref = {name: v[0] for name, v in reference(case, sd, mean, std, tile[None]).items()}
    st = {}
    st["logits"] = orc.espnet_forward(orc.preprocess(tile, mean, std), sd, case.p, case.q, st)
    st["combine_t"] = orc.br(np.concatenate([st["level3_C"], st["up_l3"]], 0), sd, "combine_l2_l3.0")
    fp32 = {name: st[name] for name in ref}
    errors = stage_errors(case, fp32, ref)
    print("case %s, fp32 C oracle vs float64, error / bound: %s" % (
        case.name, ", ".join("%s %.1e/%.1e" % (k, e, b) for k, (e, b) in errors.items())))
    assert not over(errors), over(errors)
    for name, v in fp32.items():
        bumped = v.copy()
        bumped[-1, v.shape[1] // 2, -1] += 1e-4 * float(np.abs(ref[name]).max())
        assert name in over(stage_errors(case, {name: bumped}, {name: ref[name]})), name
    blk = "encoder.level3.0" if case.q else "encoder.level3_0"
    for suffix, part in planted:
        key = blk + "." + suffix
        w = np.array(sd[key])
        assert np.abs(w[part]).max() > 0
        w[part] = 0
        wrong = reference(case, dict(sd, **{key: w}), mean, std, tile[None])
        assert over(stage_errors(case, {name: v[0] for name, v in wrong.items()}, ref)), key


@pytest.mark.parametrize("case", CASES, ids=lambda c: c.name)
def test_bounds_discriminate(case):
    """On the case's shape the fp32 C oracle passes the bounds, and they reject (a) a 1e-4 * max|ref| change of one element
    in the last column of any stage, (b) the reference with the bottom tap row of a level-3 d16 weight zeroed -- what a
    wrong F_SKIP_PAD decision computes -- and (c) with the last input channel of a level-3 reduce dropped, a K-tail bug."""
    bounds_discriminate(case)


# ---------------------------------------------------------------------------------------------- the GPU cases
class DeviceCase:
    """A case's engine on the HIP path.  forward(n, picks) runs the case's first n tiles and holds tiles `picks` to float64:
    every stage the engine still holds and the logits within the bounds, the mask the first-max argmax of the returned
    logits and off the float64 argmax only where its top-2 margin is below the logit bound, the counts its bincount; the
    mask-only kernels give the same mask and counts."""

    def __init__(self, case, weights=None):
        """weights: (state dict, mean, std) in place of case_weights(case) (test_kernel_forms_edge.py's tied weights)"""
        import torch
        from glomeruli_segmentation_amd.engine import EspnetEngine
        assert torch.cuda.is_available(), "the gpu-marked tests need a HIP device"
        self.torch, self.case = torch, case
        self.num_cus = torch.cuda.get_device_properties(0).multi_processor_count
        self.sd, self.mean, self.std = weights or case_weights(case)
        self.eng = EspnetEngine(self.sd, classes=case.classes, p=case.p, q=case.q)

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.eng.close()

    def forward(self, n, picks):
        """-> (mask, hist, logits) of all n tiles, on the host; prints the worst error / bound per stage over picks"""
        torch, case, eng, mean, std = self.torch, self.case, self.eng, self.mean, self.std
        hit = plan(n, case.H, case.W, case.p, case.q, case.classes, self.num_cus)
        assert all(hit[k] == v for k, v in case.targets.items()) and case.edges <= edges(case.H, case.W)
        tiles = np.stack([case_tile(case, k) for k in range(n)])
        ref = reference(case, self.sd, mean, std, tiles[picks])
        t = torch.from_numpy(tiles).cuda()
        mask, hist, logits = eng.segment(t, mean, std, want_logits=True)
        torch.cuda.synchronize()
        worst = self.worst = {}     # stage -> (error, bound) of the worst image so far: there to be read after a failure too
        for j, k in enumerate(picks):
            got = {name: eng.read_stage(name, image=k) for name in ref if name != "logits"}
            got["logits"] = logits[k].cpu().numpy()
            errors = stage_errors(case, got, {name: v[j] for name, v in ref.items()})
            for name, eb in errors.items():
                worst[name] = max(worst.get(name, eb), eb)
            bad = over(errors)
            assert not bad, "case %s, image %d of %d: %s" % (case.name, k, n, bad)
            m = mask[k].cpu().numpy()
            assert np.array_equal(m, got["logits"].argmax(0).astype(np.uint8)), (case.name, k)   # first maximum wins
            assert np.array_equal(hist[k].cpu().numpy(), np.bincount(m.ravel(), minlength=case.classes)), (case.name, k)
            r = ref["logits"][j]
            top2 = np.partition(r, r.shape[0] - 2, axis=0)[-2:]
            flips = (m != r.argmax(0)) & (top2[1] - top2[0] >= errors["logits"][1])
            assert not flips.any(), (case.name, k, int(flips.sum()))
        m2, h2, _ = eng.segment(t, mean, std)                                    # the mask-only kernels
        assert torch.equal(m2, mask) and torch.equal(h2, hist)
        eng.check_device_faults()
        print("case %s: n %d on %d CUs, forms %s; worst error / bound: %s" % (
            case.name, n, self.num_cus, hit, ", ".join("%s %.1e/%.1e" % (k, e, b) for k, (e, b) in worst.items())))
        return mask.cpu(), hist.cpu(), logits.cpu()


@pytest.mark.gpu
@pytest.mark.parametrize("case", CASES, ids=lambda c: c.name)
def test_kernel_form_against_float64(case):
    """The case's batch on the HIP path, sized from the device's CU count to take its target forms.  Tiles 0, n-1 and a
    middle one: every stage the engine still holds and the logits within the bounds of float64, the mask the first-max
    argmax of the returned logits and off the float64 argmax only where its top-2 margin is below the logit bound, the
    counts its bincount; the mask-only kernels give the same mask and counts."""
    with DeviceCase(case) as dev:
        n = batch_for(case, dev.num_cus)
        dev.forward(n, checked_images(n))
