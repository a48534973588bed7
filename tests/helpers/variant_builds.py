"""The variant builds of libglomseg.so that tests/test_variant_forms.py runs against float64: one table.

A variant is the shipped sources with other values of espnet_config.h's / espnet_facts.h's `#ifndef` switches (DESIGN.md,
"Build switches"), built by glomeruli_segmentation_amd.build into variants_so/libglomseg_<name>.so (git-ignored) and loaded by
a child process through GLOMSEG_LIB / GLOMSEG_EXPERIMENT (tests/helpers/variant_forms_child.py): the process that runs pytest
has the shipped library loaded and keeps it.

Per variant: the extra hipcc flags, the environment of a run, and per flipped switch the launch class whose template arguments
(or whose choice of a form) it changes together with the forms of that class that show the other value -- a case of the variant
must run one of them (test_variant_forms.py, test_every_switch_has_a_case).  CASES are test_kernel_forms.py's Case tuples: n256
is the smallest batch that takes the targets at 256 CUs (with the batch gates switched off that is one tile), `tiles` the batch
a run takes at least, so that a launch walks more than one image.
"""
import os
import subprocess
import sys
from collections import namedtuple

REPO = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
VARIANTS_DIR = os.path.join(REPO, "variants_so")
CHILD = os.path.join(REPO, "tests", "helpers", "variant_forms_child.py")
BUILD_TIMEOUT = 1500     # seconds for one variant's twelve compiler jobs and its link (measured: under a minute on 32 cores)
CHILD_TIMEOUT = 600      # seconds for one child: the planner sweep on the CPU, or a variant's handful of small cases on the card
FAULT_STATUS = (124, 137, 134, 139)     # a time limit, a kill, an abort, a segmentation fault (or any negative status)
CHILD_GAVE_UP = 70       # the child's own status after an error that is no failed assertion: it ran no further case

Variant = namedtuple("Variant", "name flags env switches")
VCase = namedtuple("VCase", "variant case tiles")

ANY_L3_REDUCE = ("CFG_L3_C1S_BNL_P1", "CFG_L3_C1S_BNL", "CFG_L3_C1S")
VARIANTS = [
    # the batch gates and the half-row / tap-row choices off: the whole-row four-pixel forms at any batch, and F_FUSE1X1 at
    # level 3 in the down-sampler alone
    Variant("alt",
            ("-DCFG_L2_DOWN_SKIP=0", "-DCFG_L3_DOWN_P2=0", "-DCFG_L3_LAST_P2=0", "-DCFG_SMALL2_WAVES=0", "-DCFG_SMALL3_WAVES=0",
             "-DCFG_FUSE_L3=1"), {},
            {"CFG_L2_DOWN_SKIP=0": ("l2_down", ("CFG_L2_BR_P4+F_VEC",)),
             "CFG_L3_DOWN_P2=0": ("l3_down", ("CFG_L3_BR+F_VEC", "CFG_L3_BR_P2F")),
             "CFG_L3_LAST_P2=0": ("l3_esp_last", ("CFG_L3_BR+F_VEC",)),
             # one to three tiles of these sizes are small batches at the shipped values: the large forms run in their place
             "CFG_SMALL2_WAVES=0": ("l2_esp_last", ("CFG_L2_BR_P4+F_VEC", "CFG_L2_BR_P4")),
             "CFG_SMALL3_WAVES=0": ("l3_esp_last", ("CFG_L3_BR+F_VEC", "CFG_L3_BR_P2")),
             # a fused down-sampler (its four-pixel and two-pixel forms) in front of blocks that fuse nothing
             "CFG_FUSE_L3=1": ("l3_down", ("CFG_L3_BR+F_VEC", "CFG_L3_BR_P2F"))}),
    # nothing fused, no skipped tap rows, no flipped stride-2 rows, the small-batch level-3 weights through LDS
    Variant("unfused",
            ("-DCFG_FUSE_L2=0", "-DCFG_FUSE_L3=0", "-DCFG_SKIP_PAD=0", "-DCFG_S2_FLIP=0", "-DCFG_SMALL_AGL=0"), {},
            {"CFG_FUSE_L2=0": ("l2_esp_fused", ("unfused CFG_L2_BR_P4+F_VEC", "unfused CFG_L2_BR_P4")),
             "CFG_FUSE_L3=0": ("l3_down", ("unfused CFG_L3_BR+F_VEC", "unfused CFG_L3_BR")),
             "CFG_SKIP_PAD=0": ("l3_esp_last", ("CFG_L3_BR_P2R+F_VEC",)),      # the level-3 half-row form CFG_FUSE_L3 = 0 leaves
             "CFG_S2_FLIP=0": ("l3_reduce", ANY_L3_REDUCE),                    # (and the level-2 stride-2 reduce of every forward)
             "CFG_SMALL_AGL=0": ("l3_esp_last", ("CFG_L3_BR_P1R",))}),
    # a -DGS_DIAG build run with GS_NO_VEC: every launch off its vector mapping and off the small-batch forms
    Variant("novec", ("-DGS_DIAG",), {"GS_NO_VEC": "1", "GLOMSEG_ALLOW_DIAG": "1"},
            {"GS_NO_VEC=1": ("dec_conv", ("MFMA MT32", "MFMA MT16"))}),
]
BY_NAME = {v.name: v for v in VARIANTS}


def lib_path(name):
    return os.path.join(VARIANTS_DIR, "libglomseg_%s.so" % name)


def _flags_path(name):
    return os.path.join(VARIANTS_DIR, "libglomseg_%s.flags" % name)


def ensure_built(name):
    """-> the variant's library, built where it is missing, older than a source or built with other flags (twelve compiler
    jobs, each under BUILD_TIMEOUT).  A build that cannot be done raises: the tests that need the library fail, none skips."""
    from glomeruli_segmentation_amd import build
    v, lib, flags = BY_NAME[name], lib_path(name), _flags_path(name)
    recorded = None
    if os.path.exists(flags):
        with open(flags) as fh:
            recorded = fh.read()
    want = " ".join(v.flags) + "\n"
    try:
        build.build_lib(force=recorded != want, out=lib, extra_flags=v.flags, timeout=BUILD_TIMEOUT)
    except Exception as e:
        raise AssertionError("variants_so/libglomseg_%s.so is missing or stale and cannot be built here (%s: %s); build it with "
                             "`python -m glomeruli_segmentation_amd.build --out variants_so/libglomseg_%s.so -- %s`"
                             % (name, type(e).__name__, e, name, " ".join(v.flags)))
    if recorded != want:
        with open(flags, "w") as fh:
            fh.write(want)
    return lib


def run_child(name, mode, env_without=(), timeout=CHILD_TIMEOUT):
    """One fresh process that loads the variant's library: -> (exit status, [the JSON lines it printed], the end of its stderr).
    A child that runs into the time limit is killed and reported as status 124."""
    import json
    v = BY_NAME[name]
    env = dict(os.environ, GLOMSEG_LIB=lib_path(name), GLOMSEG_EXPERIMENT="1", **v.env)
    for key in env_without:
        env.pop(key, None)
    cmd = [sys.executable] + (["-s"] if sys.flags.no_user_site else []) + [CHILD, name, mode]
    try:
        res = subprocess.run(cmd, env=env, capture_output=True, text=True, timeout=timeout, cwd=REPO)
    except subprocess.TimeoutExpired as e:
        return 124, [], "no answer within %d s: %s" % (timeout, (e.stderr or b"")[-2000:])
    lines = [json.loads(ln) for ln in res.stdout.splitlines() if ln.startswith("{")]
    return res.returncode, lines, res.stdout[-3000:] + res.stderr[-3000:]


def faulted(status):
    return status < 0 or status in FAULT_STATUS


# ---------------------------------------------------------------------------------------------- the cases
def _cases():
    from test_kernel_forms import Case
    P4, P4V, P2S = "CFG_L2_BR_P4", "CFG_L2_BR_P4+F_VEC", "CFG_L2_BR_P2S+F_VEC"
    U4, U4V = "unfused CFG_L2_BR_P4", "unfused CFG_L2_BR_P4+F_VEC"
    BRV, P2F, P2, P1R, P2R = "CFG_L3_BR+F_VEC", "CFG_L3_BR_P2F", "CFG_L3_BR_P2", "CFG_L3_BR_P1R", "CFG_L3_BR_P2R+F_VEC"
    UBR, UBRV = "unfused CFG_L3_BR", "unfused CFG_L3_BR+F_VEC"
    BNL1, BNL, C1S = ANY_L3_REDUCE
    TAIL5 = {"dec3": "dec3_kernel", "dec_conv": "dec_tail_kernel"}
    lone = {"lone_row", "ragged_task"}      # H/8 = 5 or 3: a lone last row of the stride-2 reduce; W/8 < 64: one ragged task
    return [
        # ---- alt.  No batch gate is left: one tile takes every target (n256 = 1)
        # the pinned level-2 down-sampler and last level-3 block; the down-sampler carries the classifier's sums: two pixels
        VCase("alt", Case("K1", "random", 5, 2, 2, 40, 160, 1,
                          dict(TAIL5, l2_down=P4V, l2_esp_fused=P4V, l2_esp_last=P4V, l3_reduce=BNL1, l3_down=P2F, l3_esp_last=BRV), lone), 3),
        # twenty classes: no classifier sums, the pinned four-pixel fused down-sampler
        VCase("alt", Case("K2", "random", 20, 2, 2, 40, 160, 1,
                          {"l2_down": P4V, "l2_esp_fused": P4V, "l2_esp_last": P4V, "l3_reduce": BNL1, "l3_down": BRV,
                           "l3_esp_last": BRV, "dec3": "MFMA MT32+F_VEC", "dec_conv": "MFMA MT32+F_VEC"}, lone), 2),
        # W/8 = 17, W/4 = 34, W/2 = 68: the odd-width forms behind the same switches; three blocks, none of them fused
        VCase("alt", Case("K3", "random", 7, 2, 3, 40, 136, 1,
                          {"l2_down": P4, "l2_esp_fused": P4, "l2_esp_last": P4, "l3_reduce": BNL1, "l3_down": P2F,
                           "l3_esp_last": P2, "dec3": "dec3_kernel", "dec_conv": "MFMA MT16"}, lone), 3),
        VCase("alt", Case("K4", "fold1", 5, 2, 8, 24, 96, 1,
                          dict(TAIL5, l2_down=P4V, l2_esp_fused=P4V, l2_esp_last=P4V, l3_reduce=BNL1, l3_down=P2F, l3_esp_last=BRV), lone), 2),
        # p = 0: the only level-3 block is the last, behind the fused down-sampler
        VCase("alt", Case("K5", "random", 5, 0, 1, 24, 96, 1,
                          dict(TAIL5, l2_down=U4V, cat_b2="cat_b2_kernel", l3_reduce=C1S, l3_down=P2F, l3_esp_last=BRV), lone), 3),
        # q = 0: nothing to fuse at level 3
        VCase("alt", Case("K6", "random", 7, 1, 0, 24, 96, 1,
                          {"l2_down": P4V, "l2_esp_last": P4V, "l3_reduce": BNL1, "l3_down": UBRV, "dec3": "dec3_kernel",
                           "dec_conv": "MFMA MT16+F_VEC"}, lone), 2),
        # ---- unfused.  The batch gates stand: up to three tiles take the small-batch forms, the half-row form needs 205
        # one tile: CFG_SMALL_AGL = 0 on a launch of five lone waves; the pinned unfused vector form of the level-2 blocks
        VCase("unfused", Case("M1", "random", 5, 2, 2, 40, 160, 1,
                              dict(TAIL5, l2_down=U4V, l2_esp_fused=U4V, l2_esp_last=P2S, l3_reduce=BNL1, l3_down=UBRV, l3_esp_last=P1R), lone), 1),
        # ... and the non-vector one; three level-3 blocks with a 1x1 launch in front of each
        VCase("unfused", Case("M2", "random", 7, 2, 3, 40, 136, 1,
                              {"l2_down": U4, "l2_esp_fused": U4, "l2_esp_last": P2S, "l3_reduce": BNL1, "l3_down": UBR,
                               "l3_esp_last": P1R, "dec3": "dec3_kernel", "dec_conv": "MFMA MT16"}, lone), 3),
        # past the small-batch gate (2048 / (5 * 2) = 204.8): the level-3 half-row form without F_SKIP_PAD -- on a map of five
        # rows, where most tap rows lie in the halo and are now multiplied -- and the whole-row reduce without F_S2_FLIP
        VCase("unfused", Case("M3", "random", 5, 2, 2, 40, 160, 205,
                              dict(TAIL5, l2_down=U4V, l2_esp_fused=U4V, l2_esp_last=P4V, l3_reduce=BNL, l3_down=UBRV, l3_esp_last=P2R), lone), 205),
        VCase("unfused", Case("M4", "fold1", 5, 2, 8, 24, 96, 1,
                              dict(TAIL5, l2_down=U4V, l2_esp_fused=U4V, l2_esp_last=P2S, l3_reduce=BNL1, l3_down=UBRV, l3_esp_last=P1R), lone), 2),
        # p = 0: the plain stride-2 reduce without F_S2_FLIP
        VCase("unfused", Case("M5", "random", 20, 0, 1, 24, 96, 1,
                              {"l2_down": U4V, "cat_b2": "cat_b2_kernel", "l3_reduce": C1S, "l3_down": UBRV, "l3_esp_last": P1R,
                               "dec3": "MFMA MT32+F_VEC", "dec_conv": "MFMA MT32+F_VEC"}, lone), 3),
        VCase("unfused", Case("M6", "random", 7, 1, 0, 40, 136, 1,
                              {"l2_down": U4, "l2_esp_last": P2S, "l3_reduce": BNL1, "l3_down": UBR, "dec3": "dec3_kernel",
                               "dec_conv": "MFMA MT16"}, lone), 2),
        # ---- novec.  No vector mapping and no small-batch form anywhere
        # the pinned MT 32 decoder conv (and MT 32 dec3) at a width the vector form would take
        VCase("novec", Case("N1", "random", 20, 2, 2, 40, 160, 1,
                            {"l2_down": P4, "l2_esp_fused": P4, "l2_esp_last": P4, "l3_reduce": BNL1, "l3_down": P2F,
                             "l3_esp_fused": P2F, "l3_esp_last": P2, "dec3": "MFMA MT32", "dec_conv": "MFMA MT32"}, lone), 3),
        VCase("novec", Case("N2", "random", 20, 0, 0, 40, 136, 1,
                            {"l2_down": U4, "cat_b2": "cat_b2_kernel", "l3_reduce": C1S, "l3_down": UBR, "dec3": "MFMA MT32",
                             "dec_conv": "MFMA MT32"}, lone), 2),
        VCase("novec", Case("N3", "fold1", 5, 2, 8, 24, 96, 1,
                            dict(TAIL5, l2_down=P4, l2_esp_fused=P4, l2_esp_last=P4, l3_reduce=BNL1, l3_down=P2F, l3_esp_fused=P2F,
                                 l3_esp_last=P2), lone), 2),
    ]


_CASES = None


def variant_cases(name=None):
    """the VCase rows, of one variant or of all"""
    global _CASES
    if _CASES is None:
        _CASES = _cases()
    return [vc for vc in _CASES if name in (None, vc.variant)]
