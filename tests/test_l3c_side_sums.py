"""level3_C (the decoder's 1x1 over output1_cat, Model.py:372) computed by the level-3 stride-2 reduce (F_SIDE1X1,
csrc/conv_mfma.h) and dec2 reading its class planes instead of the 131 planes of output1_cat.

The plan owns the decision (ForwardPlan::l3c_in_reduce, engine.plan_flags): the CPU test holds what it must say, the GPU
tests run every form of the reduce that carries the side sums -- 32-pixel tasks, whole rows, the form without BN on load --
at widths with a partial strip, and a twenty-class model that keeps the old dec2.  The reference is the float64 run of
oracle/espnet_torch_port.py; the bounds are the ones tests/test_kernel_forms.py holds the decoder stages to (TAU per stage
relative to max(1, max|ref64|), and test_gpu_parity's absolute DEC_STAGE_TOL / LOGIT_TOL for the fold-1 weights).  The new
stage "level3_C" is the input of "combine_t" and takes that stage's bound.
"""
import numpy as np
import pytest

from conftest import load_weights, random_state_dict
from test_gpu_parity import DEC_STAGE_TOL, LOGIT_TOL
from test_kernel_forms import RANDOM_MEAN_STD, TAU, plan

STAGES = ("level3_C", "combine_t", "up_l2")


def flags(n, H, W, p, q, classes, num_cus, encoder_only=False):
    from glomeruli_segmentation_amd.engine import plan_flags
    return plan_flags(n, H, W, p, q, classes, num_cus, encoder_only)


def test_plan_puts_level3_c_into_the_reduce_for_five_class_decoders_only():
    """l3c_in_reduce: true for every decoder model with five class planes -- lazy b2 or not, any batch, any tile size, any CU
    count -- and false for ESPNet-C handles and for every other class count (eight planes do not fit the reduce's registers
    at four pixel runs per lane; twelve and more were never in scope).  lazy_b2 rides along: p > 0."""
    for n in (1, 9, 32):
        for H, W in ((64, 128), (64, 1088), (512, 128), (512, 1024)):
            for p, q in ((0, 0), (0, 1), (1, 0), (2, 3), (2, 8)):
                for num_cus in (64, 256, 304):
                    for classes in range(2, 21):
                        f = flags(n, H, W, p, q, classes, num_cus)
                        assert f == {"lazy_b2": p > 0, "l3c_in_reduce": classes == 5}, (n, H, W, p, q, classes, num_cus)
                        assert flags(n, H, W, p, q, classes, num_cus, encoder_only=True) == {"lazy_b2": p > 0, "l3c_in_reduce": False}
    # the entry refuses what gs_espnet_plan_forward refuses
    from glomeruli_segmentation_amd import _lib
    for bad in ((0, 64, 128, 2, 8, 5, 256), (1, 60, 128, 2, 8, 5, 256), (1, 64, 128, 2, 8, 21, 256), (1, 64, 128, -1, 8, 5, 256),
                (1, 64, 128, 2, 8, 5, 0)):
        with pytest.raises(_lib.GlomsegError):
            flags(*bad)


def test_header_declares_the_plan_entry():
    import os
    import re
    from conftest import REPO
    from glomeruli_segmentation_amd import _lib
    with open(os.path.join(REPO, "include", "glomseg_plan.h")) as fh:
        header = re.sub(r"/\*.*?\*/", "", fh.read(), flags=re.S)
    # (the two set-up entries the header has gained since: tests/test_espnet_setup.py)
    assert set(re.findall(r"\b(gs_[a-z0-9_]+)\s*\(", header)) == set(_lib.PLAN_PROTOTYPES) == \
        {"gs_espnet_plan_flags", "gs_espnet_pack_weights", "gs_espnet_workspace_plan"}
    assert re.findall(r"^#define (GS_PLAN_\w+) (\d+)$", header, flags=re.M) == [("GS_PLAN_LAZY_B2", "1"), ("GS_PLAN_L3C_IN_REDUCE", "2")]
    assert (_lib.GS_PLAN_LAZY_B2, _lib.GS_PLAN_L3C_IN_REDUCE) == (1, 2)


# ---------------------------------------------------------------------------------------------- GPU
@pytest.fixture(scope="module")
def torch_mod():
    import torch
    assert torch.cuda.is_available(), "the gpu-marked tests need a HIP device"
    return torch


@pytest.fixture(scope="module")
def sd_fold1():
    return load_weights(1)


@pytest.fixture(scope="module")
def engine1(torch_mod, sd_fold1):
    from glomeruli_segmentation_amd.engine import EspnetEngine
    eng = EspnetEngine(sd_fold1, classes=5, p=2, q=8)
    yield eng
    eng.close()


def num_cus(torch):
    return torch.cuda.get_device_properties(0).multi_processor_count


def reference64(tiles, sd, mean, std, p, q, names):
    """float64 stages `names` and logits of uint8 tiles [k,H,W,3], each [k,C,h,w]"""
    from oracle import espnet_torch_port as port
    stages = {}
    logits = port.forward64(tiles, sd, mean, std, p, q, stages)
    out = {name: stages[name].numpy() for name in names}
    out["logits"] = logits.numpy()
    return out


def bound(name, ref, fold1):
    """test_kernel_forms.bound: tau of the stage's family relative to max(1, max|ref64|); fold-1 weights also within
    test_gpu_parity's absolute bounds.  level3_C takes the bound of the stage it feeds."""
    b = TAU["combine_t" if name == "level3_C" else name] * max(1.0, float(np.abs(ref).max()))
    return min(b, LOGIT_TOL if name == "logits" else DEC_STAGE_TOL) if fold1 else b


def check_image(eng, image, logits, ref, j, names, fold1, what):
    """stages `names` of image `image` of the last forward and its logits against row j of the reference"""
    got = {name: eng.read_stage(name, image=image) for name in names}
    got["logits"] = logits[image].cpu().numpy()
    report = {}
    for name, g in got.items():
        r = ref[name][j]
        assert g.shape == r.shape, (what, name, g.shape, r.shape)
        report[name] = (float(np.abs(np.asarray(g, dtype=np.float64) - r).max()), bound(name, r, fold1))
    print("%s, image %d, error / bound: %s" % (what, image, ", ".join("%s %.1e/%.1e" % (k, e, b) for k, (e, b) in report.items())))
    bad = {k: eb for k, eb in report.items() if not eb[0] <= eb[1]}
    assert not bad, (what, image, bad)
    return got


def fold1_tiles(seed, n, H, W):
    from glomeruli_segmentation_amd.synth import synth_tile
    return np.stack([synth_tile(seed + k, H, W) for k in range(n)])


@pytest.mark.gpu
@pytest.mark.parametrize("H,W", [(64, 128), (64, 1088)], ids=["64x128", "64x1088"])
def test_one_tile_32_pixel_tasks(torch_mod, engine1, sd_fold1, H, W):
    """One tile: the 32-pixel form (BNL_P1).  64x128: W/8 = 16, one partial strip.  64x1088: W/8 = 136 = 4 * 32 + 8, the last
    pixel pair of the level-2 row sits at the edge of a partial strip."""
    from glomeruli_segmentation_amd.synth import FOLD_MEAN_STD
    torch = torch_mod
    cus = num_cus(torch)
    assert plan(1, H, W, 2, 8, 5, cus)["l3_reduce"] == "CFG_L3_C1S_BNL_P1" and flags(1, H, W, 2, 8, 5, cus)["l3c_in_reduce"]
    mean, std = FOLD_MEAN_STD[1]
    tiles = fold1_tiles(7100 + W, 1, H, W)
    ref = reference64(tiles, sd_fold1, mean, std, 2, 8, STAGES)
    _, _, logits = engine1.segment(torch.from_numpy(tiles).cuda(), mean, std, want_logits=True)
    torch.cuda.synchronize()
    check_image(engine1, 0, logits, ref, 0, STAGES, True, "%dx%d" % (H, W))
    engine1.check_device_faults()


@pytest.mark.gpu
def test_whole_row_tasks_and_the_same_bits_alone(torch_mod, engine1, sd_fold1):
    """Nine tiles of 512x128: 9 * 64 rows * 1 strip * 4 > 8 tasks per CU on 256 CUs, the whole-row form (BNL, four pixel runs
    per lane; a device with more CUs gets the smallest batch that takes it).  Tiles 0 and n-1 against float64; and tile 0 run
    alone -- the 32-pixel form -- gives the same level3_C and the same logits bit for bit: one summation order in every form."""
    from glomeruli_segmentation_amd.synth import FOLD_MEAN_STD
    torch = torch_mod
    cus = num_cus(torch)
    H, W = 512, 128
    n = 9 if cus <= 256 else next(k for k in range(9, 64) if plan(k, H, W, 2, 8, 5, cus)["l3_reduce"] == "CFG_L3_C1S_BNL")
    assert plan(n, H, W, 2, 8, 5, cus)["l3_reduce"] == "CFG_L3_C1S_BNL" and flags(n, H, W, 2, 8, 5, cus)["l3c_in_reduce"]
    assert plan(1, H, W, 2, 8, 5, cus)["l3_reduce"] == "CFG_L3_C1S_BNL_P1"
    mean, std = FOLD_MEAN_STD[1]
    tiles = fold1_tiles(7300, n, H, W)
    ref = reference64(tiles[[0, n - 1]], sd_fold1, mean, std, 2, 8, STAGES)
    t = torch.from_numpy(tiles).cuda()
    _, _, logits = engine1.segment(t, mean, std, want_logits=True)
    torch.cuda.synchronize()
    got0 = check_image(engine1, 0, logits, ref, 0, STAGES, True, "batch of %d" % n)
    check_image(engine1, n - 1, logits, ref, 1, STAGES, True, "batch of %d" % n)
    _, _, alone = engine1.segment(t[:1], mean, std, want_logits=True)
    torch.cuda.synchronize()
    assert np.array_equal(engine1.read_stage("level3_C", image=0), got0["level3_C"])
    assert torch.equal(alone[0], logits[0])
    engine1.check_device_faults()


@pytest.mark.gpu
@pytest.mark.parametrize("n,H,W", [(1, 64, 1088), (9, 512, 128)], ids=["1x64x1088", "9x512x128"])
def test_the_form_without_bn_on_load(torch_mod, n, H, W):
    """ESPNet(5, p=0, q=1) with the seeded random weights of the depth tests: no lazy b2, so the reduce runs its plain form
    (C1S, four pixel runs per lane at every batch) with the side sums on the operands as loaded."""
    from glomeruli_segmentation_amd.engine import EspnetEngine
    from glomeruli_segmentation_amd.synth import noise_tile, synth_tile
    torch = torch_mod
    cus = num_cus(torch)
    assert plan(n, H, W, 0, 1, 5, cus)["l3_reduce"] == "CFG_L3_C1S"
    assert flags(n, H, W, 0, 1, 5, cus) == {"lazy_b2": False, "l3c_in_reduce": True}
    sd = random_state_dict(0, 1, seed=1)
    mean, std = RANDOM_MEAN_STD
    tiles = np.stack([(noise_tile if k % 2 else synth_tile)(7500 + k, H, W) for k in range(n)])
    picks = sorted({0, n - 1})
    ref = reference64(tiles[picks], sd, mean, std, 0, 1, STAGES)
    eng = EspnetEngine(sd, classes=5, p=0, q=1)
    try:
        _, _, logits = eng.segment(torch.from_numpy(tiles).cuda(), mean, std, want_logits=True)
        torch.cuda.synchronize()
        for j, k in enumerate(picks):
            check_image(eng, k, logits, ref, j, STAGES, False, "p=0, %d x %dx%d" % (n, H, W))
        eng.check_device_faults()
    finally:
        eng.close()


@pytest.mark.gpu
def test_twenty_classes_keep_the_old_dec2(torch_mod):
    """A twenty-class model: the plan says no, the forward leaves no level3_C stage, and the decoder holds its bounds."""
    from glomeruli_segmentation_amd import _lib
    from glomeruli_segmentation_amd.engine import EspnetEngine
    from glomeruli_segmentation_amd.synth import synth_tile
    torch = torch_mod
    H, W = 64, 1088
    assert not flags(1, H, W, 2, 3, 20, num_cus(torch))["l3c_in_reduce"]
    sd = random_state_dict(2, 3, classes=20, seed=23)
    mean, std = RANDOM_MEAN_STD
    tiles = synth_tile(7700, H, W)[None]
    names = ("combine_t", "up_l2")
    ref = reference64(tiles, sd, mean, std, 2, 3, names)
    eng = EspnetEngine(sd, classes=20, p=2, q=3)
    try:
        _, _, logits = eng.segment(torch.from_numpy(tiles).cuda(), mean, std, want_logits=True)
        torch.cuda.synchronize()
        check_image(eng, 0, logits, ref, 0, names, False, "20 classes")
        with pytest.raises(_lib.GlomsegError):
            eng.read_stage("level3_C")
        eng.check_device_faults()
    finally:
        eng.close()
