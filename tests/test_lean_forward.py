"""Mask-only ("lean") forwards of the full five-class networks against forwards with logits, bit for bit.

A request without logits (ForwardPlan::lean, csrc/forward_plan.h; the truth table is tests/test_lean_plan.py) runs the network's
last level-3 block without its primary store (F_CLS_ONLY, csrc/conv_mfma.h) and does not launch dec2_br_kernel; either kind
of request runs dec3_cat_kernel (csrc/espnet_kernels.h), which reads the raw cat and applies combine_l2_l3.0's BR on load, four
pixels per thread, and the two-outputs-per-thread pool_kernel.  The float64 tests (tests/test_kernel_forms.py and its
neighbours) hold the path with logits to the reference; equality carries that over to the lean one.

The shapes are the smallest at which each new path can go wrong: 16x24 (H/4 = 4, W/4 = 6: a row is one full thread of dec3 and
a tail of two, every pixel is near an edge, the maps are smaller than the dilations), 64x128 (the golden tile), 64x264 (W/8 = 33:
the non-vector level-3 forms; W/4 = 66 = 4 * 16 + 2).  With the fold-1 weights tiles this small come out as one class (no seed
of synth_tile / noise_tile among 1 900 tried, crops and strided samples of large tiles included, gave three), so the small
shapes run seeded random weights, whose masks hold all five classes (checked on the CPU with oracle/espnet_torch_port.py); the
fold-1 weights run at the sizes of tests/test_kernel_forms.py's case table, where the chosen synth_tile seeds give three and
four classes.  Every case asserts that precondition on the path with logits: at least three classes with at least 1 % of the
pixels each.
"""
import numpy as np
import pytest

from conftest import load_weights, random_state_dict
from test_kernel_forms import CASES, ENC_STAGE_TOL, RANDOM_MEAN_STD, TAU, UNREACHABLE_AT_DEFAULTS, batch_for, plan

SMALL = [(16, 24), (64, 128), (64, 264)]
BATCHES = (1, 2, 5)
RANDOM_SEED = 61          # random_state_dict(2, 8, seed=61): five classes with >= 10 % each on every tile of small_tiles
P, Q = 2, 8


@pytest.fixture(scope="module")
def torch_mod():
    import torch
    assert torch.cuda.is_available(), "the gpu-marked tests need a HIP device"
    return torch


@pytest.fixture(scope="module")
def sd_random():
    return random_state_dict(P, Q, seed=RANDOM_SEED)


@pytest.fixture(scope="module")
def engine_random(torch_mod, sd_random):
    from glomeruli_segmentation_amd.engine import EspnetEngine
    eng = EspnetEngine(sd_random, classes=5, p=P, q=Q, lanes=2)
    yield eng
    eng.close()


@pytest.fixture(scope="module")
def engine1(torch_mod):
    from glomeruli_segmentation_amd.engine import EspnetEngine
    eng = EspnetEngine(load_weights(1), classes=5, p=P, q=Q)
    yield eng
    eng.close()


def num_cus(torch):
    return torch.cuda.get_device_properties(0).multi_processor_count


def is_lean(torch, n, H, W, p=P, q=Q, classes=5, want_logits=False):
    from glomeruli_segmentation_amd.engine import plan_lean
    return plan_lean(n, H, W, p, q, classes, num_cus(torch), want_logits=want_logits)


def small_tiles(n, H, W):
    from glomeruli_segmentation_amd.synth import noise_tile, synth_tile
    return np.stack([(noise_tile if k % 2 else synth_tile)(9300 + H + W + k, H, W) for k in range(n)])


def well_mixed(mask):
    """the precondition: at least three classes with at least 1 % of the pixels of the case's masks each"""
    counts = np.bincount(np.asarray(mask).ravel(), minlength=5)
    return int((counts >= 0.01 * np.asarray(mask).size).sum()) >= 3, counts.tolist()


def full_then_lean(torch, eng, tiles, mean, std, images, what):
    """`tiles` with logits, then mask-only on the same engine: up_l3 and up_l2 of `images`, the masks and the counts are equal; the
    counts sum to the pixel count; the masks of the path with logits are well mixed.  -> {image: {stage: array}} of the former"""
    n, H, W = tiles.shape[:3]
    assert not is_lean(torch, n, H, W, want_logits=True) and is_lean(torch, n, H, W), what
    t = torch.from_numpy(tiles).cuda()
    mask, hist, _ = eng.segment(t, mean, std, want_logits=True)
    torch.cuda.synchronize()
    ok, counts = well_mixed(mask.cpu().numpy())
    assert ok, (what, counts)
    full = {k: {name: eng.read_stage(name, image=k) for name in ("up_l3", "up_l2")} for k in images}
    m2, h2, _ = eng.segment(t, mean, std)
    torch.cuda.synchronize()
    for k in images:
        for name, want in full[k].items():
            assert np.array_equal(eng.read_stage(name, image=k), want), (what, k, name)
    assert torch.equal(m2, mask), what
    assert torch.equal(h2, hist), what
    assert (h2.sum(1) == H * W).all(), what
    eng.check_device_faults()
    return full


@pytest.mark.gpu
@pytest.mark.parametrize("n", BATCHES)
@pytest.mark.parametrize("H,W", SMALL, ids=["%dx%d" % s for s in SMALL])
def test_lean_equals_full_on_small_shapes(torch_mod, engine_random, H, W, n):
    full_then_lean(torch_mod, engine_random, small_tiles(n, H, W), *RANDOM_MEAN_STD, range(n), "%d x %dx%d" % (n, H, W))


# synth_tile seeds whose fold-1 masks hold three or four classes with >= 1 % of the pixels each, per tile
# (oracle/espnet_torch_port.py, float64: 9100 at 512x1024 [295343, 75493, 150045, 3407, 0], 9102 at 264x1000
# [169182, 21911, 65933, 6974, 0], ...)
FORM_SEEDS = {(512, 1024): (9100, 9101, 9102), (264, 1000): (9100, 9102)}


@pytest.mark.gpu
def test_every_form_of_the_last_block_runs_lean(torch_mod, engine1):
    """The batches and sizes of tests/test_kernel_forms.py's cases, fold-1 weights: the first case per form of l3_esp_last runs with
    logits and lean, first and last tile read back -- and the forms that ran are every form of the class the planner can reach
    (the four-pixel one needs a CFG_L3_LAST_P2 = 0 build: UNREACHABLE_AT_DEFAULTS; it is compiled with the flag all the same)."""
    from glomeruli_segmentation_amd.engine import forward_forms
    from glomeruli_segmentation_amd.synth import FOLD_MEAN_STD, synth_tile
    torch = torch_mod
    cus = num_cus(torch)
    mean, std = FOLD_MEAN_STD[1]
    ran = set()
    for case in CASES:
        if (case.weights, case.classes, case.p, case.q) != ("fold1", 5, P, Q):
            continue
        n = batch_for(case, cus)
        form = plan(n, case.H, case.W, P, Q, 5, cus)["l3_esp_last"]
        if form in ran:
            continue
        seeds = FORM_SEEDS[(case.H, case.W)]
        base = np.stack([synth_tile(s, case.H, case.W) for s in seeds])
        full_then_lean(torch, engine1, base[np.arange(n) % len(seeds)], mean, std, sorted({0, n - 1}), "case %s: %d x %s" % (case.name, n, form))
        ran.add(form)
    every = {form for form, _ in dict(forward_forms())["l3_esp_last"]}
    assert len(every) == 4
    unreachable = {form for (cls, form) in UNREACHABLE_AT_DEFAULTS if cls == "l3_esp_last"}
    assert ran == every - unreachable and len(ran) == 3, (sorted(ran), sorted(every))


def reference64(tiles, sd, mean, std, names):
    from oracle import espnet_torch_port as port
    stages = {}
    port.forward64(tiles, sd, mean, std, P, Q, stages)
    return {name: stages[name].numpy() for name in names}


@pytest.mark.gpu
def test_padding_is_zero_after_the_br(torch_mod, sd_random):
    """combine_l2_l3.0's BN with shift 2 and zero running mean: BR(0) = 2, so a tap outside the image that was normalised instead
    of zeroed moves the edge pixels of up_l2 by O(1).  Lean equals full, and up_l2 of the path with logits is within
    tests/test_kernel_forms.py's bound for that stage of the float64 reference."""
    from glomeruli_segmentation_amd.engine import EspnetEngine
    torch = torch_mod
    sd = dict(sd_random)
    sd["combine_l2_l3.0.bn.bias"] = np.full(10, 2.0, dtype=np.float32)
    sd["combine_l2_l3.0.bn.running_mean"] = np.zeros(10, dtype=np.float32)
    mean, std = RANDOM_MEAN_STD
    eng = EspnetEngine(sd, classes=5, p=P, q=Q)
    try:
        for H, W in ((16, 24), (64, 264)):
            tiles = small_tiles(2, H, W)
            ref = reference64(tiles, sd, mean, std, ("up_l2",))["up_l2"]
            full = full_then_lean(torch, eng, tiles, mean, std, range(2), "BR(0) = 2, %dx%d" % (H, W))
            for k in range(2):
                err = float(np.abs(full[k]["up_l2"].astype(np.float64) - ref[k]).max())
                b = TAU["up_l2"] * max(1.0, float(np.abs(ref[k]).max()))
                print("BR(0) = 2, %dx%d image %d: up_l2 error / bound %.1e/%.1e" % (H, W, k, err, b))
                assert err <= b, (H, W, k, err, b)
    finally:
        eng.close()


@pytest.mark.gpu
def test_stage_contract(torch_mod, engine_random):
    """After a lean forward "combine_t" and "level3.<q-1>" are refused with a message that says to request logits, everything else
    reads, and the next forward with logits brings both back.  Models that are never lean keep them after a mask-only forward."""
    from glomeruli_segmentation_amd._lib import GlomsegError
    from glomeruli_segmentation_amd.engine import EspnetEngine
    torch = torch_mod
    mean, std = RANDOM_MEAN_STD
    H, W = 64, 264
    t = torch.from_numpy(small_tiles(2, H, W)).cuda()
    dropped = ("combine_t", "level3.%d" % (Q - 1))
    kept = ("up_l3", "level3_C", "up_l2", "sample2", "b1", "b2", "level3_0", "level3.%d" % (Q - 2))
    engine_random.segment(t, mean, std)
    torch.cuda.synchronize()
    for name in dropped:
        with pytest.raises(GlomsegError, match="request logits"):
            engine_random.read_stage(name)
    for name in kept:
        assert np.isfinite(engine_random.read_stage(name, image=1)).all(), name
    engine_random.segment(t, mean, std, want_logits=True)
    torch.cuda.synchronize()
    for name in dropped + kept + ("conv",):
        assert np.isfinite(engine_random.read_stage(name, image=1)).all(), name
    for classes, p, q in ((20, 2, 3), (5, 1, 0)):
        assert not is_lean(torch, 2, H, W, p, q, classes)
        eng = EspnetEngine(random_state_dict(p, q, classes=classes, seed=67), classes=classes, p=p, q=q)
        try:
            eng.segment(t, mean, std)
            torch.cuda.synchronize()
            names = ["combine_t", "up_l3", "up_l2", "sample2", "level3_0"] + (["level3.%d" % (q - 1)] if q else [])
            for name in names:
                assert np.isfinite(eng.read_stage(name, image=1)).all(), (classes, q, name)
            eng.check_device_faults()
        finally:
            eng.close()


@pytest.mark.gpu
def test_a_lean_forward_on_lane_1_leaves_lane_0s_up_l2(torch_mod, engine_random):
    """The shape of test_l3_classifier_sums.test_a_forward_on_lane_1_leaves_lane_0s_up_l3, for lean forwards and up_l2."""
    torch = torch_mod
    mean, std = RANDOM_MEAN_STD
    H, W = 64, 264
    a = torch.from_numpy(small_tiles(2, H, W)).cuda()
    b = torch.from_numpy(small_tiles(2, H, W)[::-1].copy()).cuda()
    engine_random.segment(a, mean, std)
    engine_random.quiesce()
    before = [engine_random.read_stage("up_l2", image=k) for k in range(2)]
    engine_random.segment(a, mean, std)                 # lane 0 again, and lane 1 right behind it
    engine_random.segment(b, mean, std, lane=1)
    engine_random.quiesce()
    for k in range(2):
        assert np.array_equal(engine_random.read_stage("up_l2", image=k), before[k])
    engine_random.check_device_faults()


# ---------------------------------------------------------------------------------------------- the pool
def emulate_sample2(tile, mean, std):
    """sample2 = AvgPool2d(3, 2, 1) twice over the normalised input (Model.py:232-239,346-348) as the kernels compute it, in float32:
    the stem's table with the reference's three roundings (x - mean, / std, / 255), then per pool the nine taps added one after
    the other from 0.0f in (ky, kx) order, padding taps as zeros, and / 9."""
    f = np.float32
    x = tile.astype(f)                                   # [H, W, 3] BGR
    x = ((x - np.asarray(mean, f)) / np.asarray(std, f)) / f(255.0)
    x = np.ascontiguousarray(x.transpose(2, 0, 1))

    def pool(v):
        c, h, w = v.shape
        padded = np.zeros((c, h + 1, w + 1), f)
        padded[:, 1:, 1:] = v
        s = np.zeros((c, h // 2, w // 2), f)
        for ky in range(3):
            for kx in range(3):
                s = s + padded[:, ky:ky + h - 1:2, kx:kx + w - 1:2]
        return s / f(9.0)
    return pool(pool(x))


POOL_SHAPES = [(16, 24), (64, 264), (24, 16)]


@pytest.mark.gpu
@pytest.mark.parametrize("H,W", POOL_SHAPES, ids=["%dx%d" % s for s in POOL_SHAPES])
def test_sample2_is_the_float32_emulation(torch_mod, engine_random, H, W):
    """pool_kernel's stage against the numpy emulation of its own arithmetic, bit for bit (the emulation was first confirmed exact
    on the build before the two-outputs-per-thread kernel: profiles/lean_forward_ab.txt), and within the bound the float64 tests
    hold the stage to."""
    torch = torch_mod
    mean, std = RANDOM_MEAN_STD
    tiles = small_tiles(2, H, W)
    engine_random.segment(torch.from_numpy(tiles).cuda(), mean, std)
    torch.cuda.synchronize()
    for k in range(2):
        got = engine_random.read_stage("sample2", image=k)
        want = emulate_sample2(tiles[k], mean, std)
        assert got.shape == want.shape == (3, H // 4, W // 4)
        err = float(np.abs(got.astype(np.float64) - want).max())
        print("sample2 %dx%d image %d: max |got - emulation| %.1e" % (H, W, k, err))
        assert err <= ENC_STAGE_TOL
        assert np.array_equal(got, want), (H, W, k, err)
    engine_random.check_device_faults()
