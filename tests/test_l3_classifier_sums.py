"""The encoder classifier behind b3 (Model.py:368-370) summed in the epilogues of the two launches that hold its input in
registers -- the level-3 down-sampler's branches (output2_0) and the last level-3 ESP block (output2): F_CLS1X1,
csrc/conv_mfma.h -- and dec1_sums_kernel adding the four partial planes per class instead of dec1_kernel re-reading both maps.

The plan owns the decision (ForwardPlan::cls_in_l3, engine.plan_cls_in_l3): the CPU tests hold what it must say and that the
change added nothing to the weight blob or the workspace; the GPU tests run every form of the two launch classes the planner
can pick, at sizes where the side sums can go wrong rather than at the workload's, and the models that keep dec1_kernel.  The
reference is the float64 run of oracle/espnet_torch_port.py; the bounds are those of tests/test_l3c_side_sums.py: TAU per
stage relative to max(1, max|ref64|), and test_gpu_parity's absolute DEC_STAGE_TOL / LOGIT_TOL for the fold-1 weights.
"""
import numpy as np
import pytest

from conftest import load_weights, random_state_dict
from test_gpu_parity import DEC_STAGE_TOL, LOGIT_TOL
from test_kernel_forms import RANDOM_MEAN_STD, TAU, plan

STAGES = ("up_l3",)


def cls_in_l3(n, H, W, p, q, classes, num_cus, encoder_only=False):
    from glomeruli_segmentation_amd.engine import plan_cls_in_l3
    return plan_cls_in_l3(n, H, W, p, q, classes, num_cus, encoder_only)


# ---------------------------------------------------------------------------------------------- CPU
def test_plan_sums_the_classifier_for_full_five_class_networks_with_an_esp_block_only():
    """cls_in_l3 is a fact of the model: five class planes, q >= 1, not an ESPNet-C handle -- at any batch, tile size, p and
    CU count.  The flags it shares the entry with are untouched."""
    from glomeruli_segmentation_amd.engine import plan_flags
    for n in (1, 9, 32):
        for H, W in ((8, 8), (64, 128), (64, 264), (512, 1024)):
            for p in (0, 2):
                for q in (0, 1, 2, 8):
                    for num_cus in (64, 256, 304):
                        for classes in range(2, 21):
                            want = classes == 5 and q >= 1
                            assert cls_in_l3(n, H, W, p, q, classes, num_cus) == want, (n, H, W, p, q, classes, num_cus)
                            assert not cls_in_l3(n, H, W, p, q, classes, num_cus, encoder_only=True)
                        assert plan_flags(n, H, W, p, q, 5, num_cus) == {"lazy_b2": p > 0, "l3c_in_reduce": True}


def test_nothing_is_added_to_the_blob_or_the_workspace():
    """The records are the piece "b3" as packed and the partial planes lie in `tt`: the packed blobs and the workspace bytes of
    the pinned models are those of tests/golden/espnet_setup.json (its own loader; no number is restated here)."""
    import hashlib
    import test_espnet_setup as setup
    from glomeruli_segmentation_amd.engine import workspace_bytes
    golden = setup.parent()
    for name, _, _, _, _ in setup.MODELS:
        blob = setup.packed(name)[1]
        want = golden["weights"][name]
        assert blob.size == want["floats"] and hashlib.sha256(blob.tobytes()).hexdigest() == want["sha256"], name
    for name, classes, p, enc in setup.WS_MODELS:
        for n, h, w in setup.SHAPES:
            for q in (0, 1, 8):
                assert workspace_bytes(n, h, w, p, q, classes, enc) == golden["workspace"]["%s/%dx%dx%d" % (name, n, h, w)]


def test_partial_planes_fit_tt():
    """20 dense planes of H/8 x W/8 per image against tt's 10 planes of H/4 x W/4 (pitch >= W/4): a quarter of the pixels
    each, so at most half of tt -- restated here for the extreme shapes the workspace tests use."""
    for H, W in ((8, 8), (64, 128), (72, 264), (4096, 4096)):
        H2, W2, H3, W3 = H // 4, W // 4, H // 8, W // 8
        pitch = (W2 + 31) // 32 * 32
        assert 20 * H3 * W3 <= 10 * (H2 * pitch + 96)


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
    eng = EspnetEngine(sd_fold1, classes=5, p=2, q=8, lanes=2)
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
    """test_l3c_side_sums.bound: tau of the stage relative to max(1, max|ref64|); fold-1 weights also within test_gpu_parity's
    absolute bounds"""
    b = TAU[name] * max(1.0, float(np.abs(ref).max()))
    return min(b, LOGIT_TOL if name == "logits" else DEC_STAGE_TOL) if fold1 else b


def check_image(eng, image, logits, ref, j, fold1, what):
    """up_l3 of image `image` of the last forward and its logits against row j of the reference; returns what was read"""
    got = {name: eng.read_stage(name, image=image) for name in STAGES}
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


def tiles_of(seed, n, H, W):
    from glomeruli_segmentation_amd.synth import noise_tile, synth_tile
    return np.stack([(noise_tile if k % 2 else synth_tile)(seed + k, H, W) for k in range(n)])


# 8x8: a 1x1 level-3 map, every dilated tap in the halo.  64x128: 8x16, smaller than the dilations.  64x264: W3 = 33, a run
# boundary and 31 lanes past the row end whose partial sums must not be stored.  72x264: H3 = 9, odd, too.
SHAPES = [(8, 8), (64, 128), (64, 264), (72, 264)]


@pytest.mark.gpu
@pytest.mark.parametrize("H,W", SHAPES, ids=["%dx%d" % s for s in SHAPES])
def test_fold1_stages(torch_mod, engine1, sd_fold1, H, W):
    """up_l3 and the logits of two tiles (a blob tile and a noise tile) with the fold-1 weights, at each of SHAPES."""
    from glomeruli_segmentation_amd.synth import FOLD_MEAN_STD
    torch = torch_mod
    assert cls_in_l3(2, H, W, 2, 8, 5, num_cus(torch))
    mean, std = FOLD_MEAN_STD[1]
    tiles = tiles_of(8100 + H + W, 2, H, W)
    ref = reference64(tiles, sd_fold1, mean, std, 2, 8, STAGES)
    _, _, logits = engine1.segment(torch.from_numpy(tiles).cuda(), mean, std, want_logits=True)
    torch.cuda.synchronize()
    for k in range(2):
        check_image(engine1, k, logits, ref, k, True, "fold 1, %dx%d" % (H, W))
    engine1.check_device_faults()


# (p, q): the shipped depth; q = 1: the down-sampler and the last block are adjacent; q = 2; p = 0 (no lazy b2) with q = 1 and 2
DEPTHS = [(2, 8), (1, 1), (2, 2), (0, 1), (0, 2)]


@pytest.mark.gpu
@pytest.mark.parametrize("p,q", DEPTHS, ids=["p%d_q%d" % d for d in DEPTHS])
def test_random_weights_by_depth(torch_mod, p, q):
    """Seeded random weights at every depth that changes which launches carry the sums, over all of SHAPES in one engine."""
    from glomeruli_segmentation_amd.engine import EspnetEngine
    torch = torch_mod
    sd = random_state_dict(p, q, seed=31 + 10 * p + q)
    mean, std = RANDOM_MEAN_STD
    eng = EspnetEngine(sd, classes=5, p=p, q=q)
    try:
        for H, W in SHAPES:
            assert cls_in_l3(1, H, W, p, q, 5, num_cus(torch))
            tiles = tiles_of(8300 + H + W + q, 1, H, W)
            ref = reference64(tiles, sd, mean, std, p, q, STAGES)
            _, _, logits = eng.segment(torch.from_numpy(tiles).cuda(), mean, std, want_logits=True)
            torch.cuda.synchronize()
            check_image(eng, 0, logits, ref, 0, False, "p=%d q=%d, %dx%d" % (p, q, H, W))
        eng.check_device_faults()
    finally:
        eng.close()


def batch_with(H, W, cus, want_down, want_last):
    """the smallest batch of H x W tiles whose plan runs the two launch classes in the given forms"""
    for k in range(1, 200):
        pl = plan(k, H, W, 2, 8, 5, cus)
        if pl["l3_down"] == want_down and pl["l3_esp_last"] == want_last:
            return k
    raise AssertionError("no batch of %dx%d tiles plans %s / %s" % (H, W, want_down, want_last))


# The forms the planner can pick for l3_down / l3_esp_last with the shipped configuration: the 32-pixel forms (small batches, weights
# through the operand ring), the half-row vector forms (even W/8), the two-run forms (odd W/8).  The four-pixel forms need
# CFG_L3_DOWN_P2 = 0 / CFG_L3_LAST_P2 = 0 builds (test_kernel_forms.UNREACHABLE_AT_DEFAULTS).
@pytest.mark.gpu
@pytest.mark.parametrize("W,down,last", [(128, "CFG_L3_BR_P2R+F_VEC", "CFG_L3_BR_P2R+F_VEC"), (136, "CFG_L3_BR_P2F", "CFG_L3_BR_P2")],
                         ids=["half_row_vec", "two_runs"])
def test_every_form_gives_the_same_bits(torch_mod, engine1, sd_fold1, W, down, last):
    """Tile 0 inside the smallest batch that selects the full-batch forms, against float64; then alone, where both launches
    take their 32-pixel forms: up_l3 and the logits bit for bit -- one summation order in every form."""
    from glomeruli_segmentation_amd.synth import FOLD_MEAN_STD
    torch = torch_mod
    cus = num_cus(torch)
    H = 512
    n = batch_with(H, W, cus, down, last)
    alone = plan(1, H, W, 2, 8, 5, cus)
    assert alone["l3_down"] == "CFG_L3_BR_P1R" and alone["l3_esp_last"] == "CFG_L3_BR_P1R"
    mean, std = FOLD_MEAN_STD[1]
    base = tiles_of(8500 + W, 3, H, W)
    tiles = base[np.arange(n) % 3]
    ref = reference64(tiles[[0, n - 1]], sd_fold1, mean, std, 2, 8, STAGES)
    t = torch.from_numpy(tiles).cuda()
    _, _, logits = engine1.segment(t, mean, std, want_logits=True)
    torch.cuda.synchronize()
    got0 = check_image(engine1, 0, logits, ref, 0, True, "batch of %d x %dx%d" % (n, H, W))
    check_image(engine1, n - 1, logits, ref, 1, True, "batch of %d x %dx%d" % (n, H, W))
    _, _, one = engine1.segment(t[:1], mean, std, want_logits=True)
    torch.cuda.synchronize()
    assert np.array_equal(engine1.read_stage("up_l3", image=0), got0["up_l3"])
    assert torch.equal(one[0], logits[0])
    engine1.check_device_faults()


@pytest.mark.gpu
def test_a_forward_on_lane_1_leaves_lane_0s_up_l3(torch_mod, engine1):
    """The partial planes live in each lane's own workspace: a forward of other tiles on lane 1 right after one on lane 0
    changes nothing of lane 0's up_l3."""
    from glomeruli_segmentation_amd.synth import FOLD_MEAN_STD
    torch = torch_mod
    mean, std = FOLD_MEAN_STD[1]
    H, W = 64, 264
    a = torch.from_numpy(tiles_of(8700, 2, H, W)).cuda()
    b = torch.from_numpy(tiles_of(8800, 2, H, W)).cuda()
    engine1.segment(a, mean, std)
    engine1.quiesce()
    before = [engine1.read_stage("up_l3", image=k) for k in range(2)]
    engine1.segment(a, mean, std)                 # lane 0 again, and lane 1 right behind it
    engine1.segment(b, mean, std, lane=1)
    engine1.quiesce()
    for k in range(2):
        assert np.array_equal(engine1.read_stage("up_l3", image=k), before[k])
    engine1.check_device_faults()


@pytest.mark.gpu
def test_seven_classes_keep_dec1_kernel(torch_mod):
    from glomeruli_segmentation_amd.engine import EspnetEngine
    torch = torch_mod
    H, W = 64, 264
    assert not cls_in_l3(1, H, W, 1, 2, 7, num_cus(torch))
    sd = random_state_dict(1, 2, classes=7, seed=47)
    mean, std = RANDOM_MEAN_STD
    tiles = tiles_of(8900, 1, H, W)
    ref = reference64(tiles, sd, mean, std, 1, 2, STAGES)
    eng = EspnetEngine(sd, classes=7, p=1, q=2)
    try:
        _, _, logits = eng.segment(torch.from_numpy(tiles).cuda(), mean, std, want_logits=True)
        torch.cuda.synchronize()
        check_image(eng, 0, logits, ref, 0, False, "7 classes")
        eng.check_device_faults()
    finally:
        eng.close()


@pytest.mark.gpu
def test_an_encoder_only_handle_keeps_dec1_kernel(torch_mod, sd_fold1):
    """ESPNet-C with the fold-1 encoder: its 1/8-scale logits are dec1_kernel's classifier sums, against the float64 run's
    "enc_classifier" within the bound of the stage they feed in the full network."""
    from glomeruli_segmentation_amd.engine import EspnetEngine
    from glomeruli_segmentation_amd.synth import FOLD_MEAN_STD
    torch = torch_mod
    H, W = 64, 264
    assert not cls_in_l3(1, H, W, 2, 8, 5, num_cus(torch), encoder_only=True)
    mean, std = FOLD_MEAN_STD[1]
    tiles = tiles_of(9000, 1, H, W)
    ref = reference64(tiles, sd_fold1, mean, std, 2, 8, ("enc_classifier",))["enc_classifier"][0]
    eng = EspnetEngine({k[len("encoder."):]: v for k, v in sd_fold1.items() if k.startswith("encoder.")}, classes=5, p=2, q=8,
                       encoder_only=True)
    try:
        _, _, enc = eng.segment(torch.from_numpy(tiles).cuda(), mean, std, want_enc_logits=True)
        torch.cuda.synchronize()
        err = float(np.abs(enc[0].cpu().numpy().astype(np.float64) - ref).max())
        b = min(TAU["up_l3"] * max(1.0, float(np.abs(ref).max())), DEC_STAGE_TOL)
        print("ESPNet-C 1/8-scale logits, error / bound: %.1e/%.1e" % (err, b))
        assert err <= b
        eng.check_device_faults()
    finally:
        eng.close()
