"""Ensembles whose members are full ESPNets: every member's decoder tail turns its logits into ens_w * softmax and stores or adds them
into ONE fp32 accumulator, the last member takes the first-max argmax of the sum and counts the classes -- MODE 2 of dec_tail_kernel
(csrc/dec_tail.h) at five classes, dec4_kernel<CLS, true> (csrc/espnet_kernels.h) at every other class count; roles and weights
from run_ensemble (EnsRole, csrc/gs_internal.h).

The definition is restated here in float64 numpy (ens_ref).  With l_k member k's full-resolution logits [C, H, W]:

    P[c] = sum_k softmax_c(l_k) * (1 / K)        class = first maximum of P        counts = bincount of the class map per image

MARGIN RULE of every GPU case: the mask equals ens_ref(...).argmax(0) wherever the float64 top-2 margin of P exceeds TAU; the counts
equal the bincount of the GPU mask over `classes` bins and sum to n * H * W.  On the GPU the truth's inputs are every member's OWN
logits from its own single-model pass (engine.segment(..., want_logits=True): trunk and logits are held against float64 by
tests/test_kernel_forms.py), so the rule isolates softmax, accumulation, argmax and counts.

TAU = 1e-5, the value of tests/test_espnet_c_ensemble.py, justified by measurement on the CPU and not by the code under test
(test_fp32_restatement_within_tau): the same definition evaluated in fp32 in the kernels' order (ens_ref32: expf(l - max), the sum
over ascending classes, e / sum * w with w = 1.0f / K, old + new over ascending members) differs from float64 in P by at most
3.1e-7 (13 classes, K = 1; 2.1e-7 on the folds; asserted <= MEASURED_WORST = 3.2e-7) over the logits (CPU oracle) of every GPU case
below, the crop cases and the five folds on both ensemble.npz tiles -- far below TAU / 2, so TAU stays 1e-5.  The other half of TAU
covers what that measurement cannot see: the device's expf against numpy's (a couple of ulp on values <= 1: ~2.4e-7 per term, at
most that on P, a convex mean) and one multiply-add of the logits rounded differently by the DBG and ENS instantiations (a logit
change d moves a softmax value by at most d / 4; an ulp of a logit of magnitude 8 is 9.5e-7).

Conditions on a case, asserted from the truth alone (on the CPU from the oracle's logits, again on the GPU from the members'): the
margin set holds at most 1e-3 of the case's pixels; the truth shows three classes where classes >= 5 and both classes below.

MEMBERS are conftest.random_state_dict(1, 1, classes, seed) with classifier.weight (the final deconvolution) multiplied by a gain,
each with its own mean/std: seed 5000 + 37 * classes + k and gain 1.0 up to eight classes (mean logit spread 0.6 .. 1.2 at five
classes, 3.7 .. 5.3 at seven), 0.3 above (spread 1.8 .. 5.5; at gain 1.0 the softmax of twelve and more classes is nearly one-hot, P
a vote with near-ties); two classes take seed 5300 + k, for which the truth shows both classes (5000 + 37 * 2 + k showed one only).
Tiles are noise tiles seeded by the case (300000 + 7 h + 3 w + 1009 classes + image: of four bases tried the one whose worst
margin-set share, 4.9e-4 on 8 x 2056, leaves every case a factor of two under the cap).  Chosen with the CPU oracle's logits so that
the truth alone meets the conditions; test_fp32_restatement_within_tau prints and asserts them.  On the GPU the worst share seen is
the same 4.9e-4 (8 x 2056), and no pixel differed from the float64 argmax, inside the margin set or outside.

The shifted-band cases run with K = 2 and K = 3: with two members FIRST only stores and LAST only reads, so a row that two bands both
take shows in the counts alone; a MIDDLE member (K >= 3) reads AND writes the accumulator, the one role for which such a row is a
probability added twice.
"""
import ctypes

import numpy as np
import pytest

from conftest import load_golden, load_weights, random_state_dict

TAU = 1e-5
MEASURED_WORST = 3.2e-7       # max |ens_ref32 - ens_ref| (test_fp32_restatement_within_tau asserts that it is not exceeded)
MAX_EXCLUDED = 1e-3
P_Q = (1, 1)

# (height, width, n, classes, K).  W1 = width / 2 decides the tail form (launch_dec_tail).
FIVE_CASES = [
    (16, 16, 3, 5, 2),       # packed, NRUN 1: eight images per task, a short group of three
    (16, 48, 5, 5, 3),       # packed, NRUN 2: groups of 4 + 1
    (24, 96, 3, 5, 1),       # packed, NRUN 4: groups of 2 + 1; SOLE
    (16, 128, 2, 5, 2),      # packed, NRUN 8
    (16, 136, 3, 5, 5),      # exchange, team 1
    (32, 392, 2, 5, 2),      # exchange, team 2, partial last strip
    (40, 520, 3, 5, 3),      # exchange, team 4, one wave idle
    (16, 776, 1, 5, 1),      # exchange, team 4, 4-pixel last strip; SOLE
    (24, 1208, 2, 5, 2),     # exchange, team 8, three waves idle
    (16, 2048, 1, 5, 3),     # exchange, team 8, full
    (8, 2056, 3, 5, 3),      # overlapping strips plus a rest launch (NRUN 2, images packed)
]
# dec4_kernel<CLS, true> at every padded width (cp) and pixels-per-thread setting: 24 x 104 = 624 half-resolution pixels, ragged
# against the 1 024, 512 and 256 a workgroup takes
CLASS_CASES = [
    (24, 104, 2, 2, 2),      # cp 4
    (24, 104, 2, 7, 3),      # cp 8
    (24, 104, 2, 12, 2),     # cp 12
    (24, 104, 2, 13, 1),     # cp 16; SOLE
    (24, 104, 2, 13, 2),     # cp 16 again with two members: under K = 1 a padding plane inside the softmax sum cannot move the argmax
    (24, 104, 2, 20, 8),     # cp 20
    (40, 264, 3, 7, 2),      # more than one workgroup per image
]
BAND_WIDE = (56, 1024, 128, 5, 2)          # exchange form, 128 images: bands of 8 rows over 28 on 256 CUs
BAND_WIDE_IMAGES = (0, 77, 127)            # the margin rule on these (counts on all)
# K = 2: FIRST stores and LAST only reads, so a row taken twice shows in the counts alone; K = 3 has a MIDDLE member, the only role
# that reads AND writes the accumulator -- the one for which a row taken twice is a probability added twice
BAND_KS = (2, 3)
BAND_TALL_WIDTH = 16                       # packed form, one image, height from tall_height(CUs): 8208 on 256 CUs
DEFAULT_CUS = 256
# the crop entries: five crops at net size 64 x 128 -- one network-sized, four not, one of them 21 wide -- with three five-class
# and with two seven-class members
NET_H, NET_W = 64, 128
CROP_SIZES = [(64, 128), (150, 99), (33, 21), (301, 420), (40, 56)]
CROP_MEMBERS = [(5, 3), (7, 2)]
# members at trained-range PReLU / BatchNorm parameters (helpers/edge_weights.edge_state_dict: negative slopes, slopes above 1, negative and
# zero BN weights; test_kernel_forms_edge.py): one row of FIVE_CASES and one of CLASS_CASES, under the same margin rule
EDGE_MEMBER_CASES = [FIVE_CASES[6], CLASS_CASES[1]]


def gain(classes):
    return 1.0 if classes <= 8 else 0.3


def member(classes, k):
    """(state dict, mean, std) of member k of the random-weight ensemble with `classes` classes"""
    sd = random_state_dict(P_Q[0], P_Q[1], classes=classes, seed=(5300 + k) if classes == 2 else (5000 + 37 * classes + k))
    sd["classifier.weight"] = (sd["classifier.weight"] * np.float32(gain(classes))).astype(np.float32)
    return sd, (120.0 + 5 * k, 130.0 - 3 * k, 110.0 + 2 * k), (60.0 + k, 55.0 + 2 * k, 70.0 - k)


def edge_member(classes, k):
    """member(classes, k) with the edge rewrite of its PReLU slopes and BatchNorm weights"""
    from helpers.edge_weights import edge_state_dict
    sd, mean, std = member(classes, k)
    return edge_state_dict(sd), mean, std


def case_tiles(h, w, n, classes, images=None):
    """the case's noise tiles; `images`: only these (every tile has its own seed)"""
    from glomeruli_segmentation_amd.synth import noise_tile
    return np.stack([noise_tile(300000 + 7 * h + 3 * w + 1009 * classes + i, h, w) for i in (range(n) if images is None else images)])


def crop_inputs(classes):
    from glomeruli_segmentation_amd.synth import noise_tile
    return [noise_tile(200000 + 1009 * classes + i, h, w) for i, (h, w) in enumerate(CROP_SIZES)]


def softmax64(lg):
    v = np.asarray(lg, dtype=np.float64)
    e = np.exp(v - v.max(0, keepdims=True))
    return e / e.sum(0, keepdims=True)


def ens_ref(logits):
    """K x [C, H, W] fp32 -> P float64 [C, H, W]: the definition in float64 (max-shifted exp)"""
    P = 0.0
    for lg in logits:
        P = P + softmax64(lg) * (1.0 / len(logits))
    return P


def ens_ref32(logits):
    """the same with every operation in fp32, in the kernels' order (what an fp32 implementation of the definition computes)"""
    w = np.float32(1.0) / np.float32(len(logits))
    P = None
    for lg in logits:
        lg = np.asarray(lg, dtype=np.float32)
        e = np.exp(lg - lg.max(0, keepdims=True))
        s = e[0].copy()
        for c in range(1, e.shape[0]):
            s = s + e[c]
        new = e / s * w
        P = new if P is None else P + new
        assert P.dtype == np.float32
    return P


def margin_set(P):
    t = np.sort(P, axis=0)[-2:]
    return (t[1] - t[0]) <= TAU


def truth(logits):
    """(first-max class map, excluded set: float64 top-2 margin of P <= TAU)"""
    P = ens_ref(logits)
    return P.argmax(0).astype(np.uint8), margin_set(P)


def check_conditions(seen, excluded, pixels, classes, what):
    assert excluded <= MAX_EXCLUDED * pixels, "%s: the margin set holds %d of %d pixels" % (what, excluded, pixels)
    assert len(seen) >= (3 if classes >= 5 else classes), "%s: the truth shows classes %s only" % (what, sorted(seen))


def check_margin_rule(mask, hist, logits, classes, what, images=None):
    """mask [n, H, W], hist [n, classes] | None, logits: K x [n', C, H, W], every member's own logits of images `images` (all n)"""
    n, H, W = mask.shape
    images = list(range(n)) if images is None else list(images)
    seen, excluded = set(), 0
    for j, i in enumerate(images):
        ref, excl = truth([lg[j] for lg in logits])
        diff = mask[i] != ref
        bad = diff & ~excl
        print("%s image %d: %d pixels differ, %d outside the margin set (%d pixels)" % (what, i, int(diff.sum()), int(bad.sum()), int(excl.sum())))
        assert not bad.any(), "%s image %d: %d pixels differ from the float64 argmax outside the margin set" % (what, i, int(bad.sum()))
        seen |= set(np.unique(ref).tolist())
        excluded += int(excl.sum())
    if hist is not None:
        assert hist.shape == (n, classes) and int(hist.sum()) == n * H * W, what
        for i in range(n):
            assert np.array_equal(hist[i], np.bincount(mask[i].ravel(), minlength=classes)), (what, i)
    check_conditions(seen, excluded, len(images) * H * W, classes, what)


def cdiv(a, b):
    return -(-a // b)


def tail_band_plan(H1, W1, n, cus):
    """(R, bands) of the fused tail's first launch: launch_dec_tail / launch_dec_tail_exch / launch_dec_tail_p (csrc/dec_tail.h)
    restated.  Bands have R = 3k + 2 rows, about one round of tasks over the resident waves; the last band is shifted up to end
    at the image bottom, so R * bands > H1 means rows that two bands share."""
    if 64 < W1 <= 1024:                       # exchanging strips: a task is (image, band), taken by a team of waves
        nstrips = cdiv(W1, 128)
        team = 1 if nstrips <= 1 else 2 if nstrips <= 2 else 4 if nstrips <= 4 else 8
        slots, cols = cus * (8 // team), n
    else:
        full = W1 // 126
        if full:                              # overlapping 126-pixel strips, one image per task
            slots, cols = cus * 8, n * full
        else:                                 # a narrow row: 8 / NRUN images side by side
            nrun = cdiv(W1 + 2, 16)
            nrun = 1 if nrun <= 1 else 2 if nrun <= 2 else 4 if nrun <= 4 else 8
            slots, cols = cus * 8, cdiv(n, 8 // nrun)
    bands = max(1, slots // cols)
    k3 = max(0, cdiv(H1, bands) // 3)
    while k3 > 0 and 3 * k3 + 2 > H1:
        k3 -= 1
    k3 = min(k3, 169)
    R = 3 * k3 + 2
    return R, cdiv(H1, R)


def tall_height(cus):
    """the height of a 16-wide single tile whose packed tail works in bands of five rows with the last one shifted: a little over
    two rows per wave slot (8 waves per CU), not a multiple of five; 8208 on 256 CUs (4104 rows in 821 bands, one row shared)"""
    H1 = 2 * cus * 8 + 8
    while H1 % 5 == 0:
        H1 += 4
    return 2 * H1


# ------------------------------------------------------------------------------------------ CPU
def oracle_logits(tiles, classes, K):
    """K x [n, C, H, W]: every member's logits of the tiles from the CPU oracle"""
    from oracle import espnet_oracle as orc
    out = []
    for k in range(K):
        sd, mean, std = member(classes, k)
        out.append(np.stack([orc.segment_tile(t, sd, mean, std, *P_Q)[0] for t in tiles]))
    return out


@pytest.fixture(scope="module")
def fold_logits():
    """the five folds' logits of the two ensemble.npz tiles from the CPU oracle (each fold with its own mean/std): 5 x [2, 5, H, W]"""
    from glomeruli_segmentation_amd.synth import FOLD_MEAN_STD
    from oracle import espnet_oracle as orc
    z = load_golden("ensemble.npz")
    return [np.stack([orc.segment_tile(z["tile_%d" % s], load_weights(f), *FOLD_MEAN_STD[f])[0] for s in range(2)]) for f in range(1, 6)]


@pytest.fixture(scope="module")
def case_logits():
    """oracle logits by case, computed on first use and shared (never modified) by the CPU tests"""
    cache = {}

    def get(h, w, n, classes, K, images=None):
        key = (h, w, n, classes, K, images)
        if key not in cache:
            cache[key] = oracle_logits(case_tiles(h, w, n, classes, images), classes, K)
        return cache[key]
    return get


def test_restatement_reproduces_the_golden_masks(fold_logits):
    """ens_ref on the oracle's fold logits gives ensemble.npz's two masks (written from the reference models) outside their edge sets"""
    z = load_golden("ensemble.npz")
    for s in range(2):
        ref = z["mask_%d" % s]
        edge = np.unpackbits(z["edge_%d" % s]).reshape(ref.shape).astype(bool)
        diff = ens_ref([lg[s] for lg in fold_logits]).argmax(0) != ref
        print("tile %d: %d pixels differ from the fixture, %d outside its edge set (%d pixels)" % (s, int(diff.sum()), int((diff & ~edge).sum()), int(edge.sum())))
        assert not (diff & ~edge).any(), s


def test_band_plan_restatement():
    """the two shifted-band shapes on the 256 CUs of an MI355X: 8 rows over 28 in four bands; 5 rows over 4104 in 821 bands"""
    h, w, n, _, _ = BAND_WIDE
    assert tail_band_plan(h // 2, w // 2, n, DEFAULT_CUS) == (8, 4)
    assert tall_height(DEFAULT_CUS) == 8208 and tail_band_plan(4104, BAND_TALL_WIDTH // 2, 1, DEFAULT_CUS) == (5, 821)
    for cus in (64, 80, 104, 228, 256, 304):
        H1 = tall_height(cus) // 2
        R, bands = tail_band_plan(H1, BAND_TALL_WIDTH // 2, 1, cus)
        assert R == 5 and 0 < R * bands - H1 < R and tall_height(cus) % 8 == 0, cus


def cpu_cases():
    """every GPU case the CPU can afford: all of them, with the 128-image case on the three images the margin rule looks at"""
    cases = [c + (None,) for c in FIVE_CASES + CLASS_CASES]
    for K in BAND_KS:
        cases.append(BAND_WIDE[:4] + (K, BAND_WIDE_IMAGES))
        cases.append((tall_height(DEFAULT_CUS), BAND_TALL_WIDTH, 1, 5, K, None))
    return cases


def test_fp32_restatement_within_tau(fold_logits, case_logits):
    """TAU's justification, measured: the definition in fp32 in the kernels' order against float64 on the oracle's logits of every
    GPU case and of the five folds on both fixture tiles.  Also the conditions on the cases, from the oracle's logits alone."""
    worst = 0.0
    for s in range(2):
        lgs = [lg[s] for lg in fold_logits]
        worst = max(worst, float(np.abs(ens_ref32(lgs).astype(np.float64) - ens_ref(lgs)).max()))
    print("five folds, two tiles: worst |P32 - P64| = %.3g" % worst)
    for h, w, n, classes, K, images in cpu_cases():
        lgs = case_logits(h, w, n, classes, K, images)
        seen, excluded, case_worst, spread = set(), 0, 0.0, 0.0
        m = lgs[0].shape[0]
        for i in range(m):
            li = [lg[i] for lg in lgs]
            P = ens_ref(li)
            case_worst = max(case_worst, float(np.abs(ens_ref32(li).astype(np.float64) - P).max()))
            spread = max(spread, float(np.mean([np.ptp(l, axis=0).mean() for l in li])))
            seen |= set(np.unique(P.argmax(0)).tolist())
            excluded += int(margin_set(P).sum())
        print("%dx%d n=%d classes=%d K=%d: |P32 - P64| <= %.3g, mean logit spread %.2f, classes in the truth %s, margin set %d of %d pixels"
              % (h, w, n, classes, K, case_worst, spread, sorted(seen), excluded, m * h * w))
        check_conditions(seen, excluded, m * h * w, classes, "%dx%d c%d K%d" % (h, w, classes, K))
        worst = max(worst, case_worst)
    # the crop cases: the oracle's chain normalise -> bilinear resize to the network size -> forward
    from oracle import espnet_oracle as orc
    from oracle import image_oracle as io
    for classes, K in CROP_MEMBERS:
        seen, excluded, case_worst = set(), 0, 0.0
        for c in crop_inputs(classes):
            li = []
            for k in range(K):
                sd, mean, std = member(classes, k)
                li.append(orc.espnet_forward(io.normalise_then_resize(c, mean, std, NET_W, NET_H), sd, *P_Q))
            P = ens_ref(li)
            case_worst = max(case_worst, float(np.abs(ens_ref32(li).astype(np.float64) - P).max()))
            seen |= set(np.unique(P.argmax(0)).tolist())
            excluded += int(margin_set(P).sum())
        pixels = len(CROP_SIZES) * NET_H * NET_W
        print("crops classes=%d K=%d: |P32 - P64| <= %.3g, classes in the truth %s, margin set %d of %d pixels"
              % (classes, K, case_worst, sorted(seen), excluded, pixels))
        check_conditions(seen, excluded, pixels, classes, "crops c%d K%d" % (classes, K))
        worst = max(worst, case_worst)
    print("fp32 restatement vs float64: worst |P32 - P64| = %.3g" % worst)
    assert worst <= MEASURED_WORST, "the docstring's and DESIGN.md's figure is out of date"
    assert worst <= TAU / 2


@pytest.mark.parametrize("h,w,n,classes,K", EDGE_MEMBER_CASES)
def test_edge_member_conditions(h, w, n, classes, K):
    """the edge-weight members' cases meet the conditions of the margin rule, and TAU's measurement holds for their logits too: from
    the CPU oracle's logits alone"""
    from oracle import espnet_oracle as orc
    assert (h, w, n, classes, K) in FIVE_CASES + CLASS_CASES
    lgs = []
    for k in range(K):
        sd, mean, std = edge_member(classes, k)
        lgs.append(np.stack([orc.segment_tile(t, sd, mean, std, *P_Q)[0] for t in case_tiles(h, w, n, classes)]))
    seen, excluded, worst = set(), 0, 0.0
    for i in range(n):
        li = [lg[i] for lg in lgs]
        P = ens_ref(li)
        worst = max(worst, float(np.abs(ens_ref32(li).astype(np.float64) - P).max()))
        seen |= set(np.unique(P.argmax(0)).tolist())
        excluded += int(margin_set(P).sum())
    print("edge members %dx%d n=%d classes=%d K=%d: |P32 - P64| <= %.3g, classes in the truth %s, margin set %d of %d pixels"
          % (h, w, n, classes, K, worst, sorted(seen), excluded, n * h * w))
    check_conditions(seen, excluded, n * h * w, classes, "edge members %dx%d c%d K%d" % (h, w, classes, K))
    assert worst <= MEASURED_WORST


def mutated(logits, weight=None, own_last=False, pad_plane=False):
    """P float64 of a WRONG ensemble: weight [K, H, W] multiplies member k's probabilities per pixel (2: added twice, 0: left out);
    own_last: the last member's softmax alone; pad_plane: a zero logit of a padding plane takes part in every softmax"""
    K = len(logits)
    if own_last:
        return softmax64(logits[-1])
    P = 0.0
    for k, lg in enumerate(logits):
        if pad_plane:
            sm = softmax64(np.concatenate([lg, np.zeros_like(lg[:1])]))[:-1]
        else:
            sm = softmax64(lg)
        P = P + sm * (1.0 / K) * (1.0 if weight is None else weight[k][None])
    return P


def test_rule_rejects_what_the_kernels_can_get_wrong(case_logits):
    """each mutation of the ensemble, applied to the oracle's logits of one image of a case, leaves differing pixels OUTSIDE the
    margin set, so the margin rule would fail on it: (a) a member added twice on one pair of output rows (the shifted band);
    (b) a member left out on one 256-pixel column strip (a 128-column strip at half resolution); (c) seven classes: the zero
    logit of the eighth, padding, plane in every member's softmax sum; (d) the last tail's argmax of its own softmax"""
    h, w, n, classes, K = FIVE_CASES[6]
    assert (h, w, K) == (40, 520, 3)
    lgs = [lg[0] for lg in case_logits(h, w, n, classes, K)]
    ref, excl = truth(lgs)

    def outside(P, what, region=None):
        bad = (P.argmax(0) != ref) & ~excl
        if region is not None:
            assert not bad[~region].any()
        print("%s: %d pixels differ outside the margin set" % (what, int(bad.sum())))
        return int(bad.sum())
    twice = np.ones((K, h, w))
    twice[1, h - 2:h] = 2.0
    rows = np.zeros((h, w), bool)
    rows[h - 2:h] = True
    assert outside(mutated(lgs, weight=twice), "(a) member 1 twice on the last row pair", rows) >= 1
    left_out = np.ones((K, h, w))
    left_out[1, :, 256:512] = 0.0
    strip = np.zeros((h, w), bool)
    strip[:, 256:512] = True
    assert outside(mutated(lgs, weight=left_out), "(b) member 1 left out on columns 256..511", strip) >= 1
    assert outside(mutated(lgs, own_last=True), "(d) the last member's own argmax") >= 1
    h, w, n, classes, K = CLASS_CASES[1]
    assert (classes, K) == (7, 3)
    lgs = [lg[0] for lg in case_logits(h, w, n, classes, K)]
    ref, excl = truth(lgs)
    assert outside(mutated(lgs, pad_plane=True), "(c) seven classes, the padding plane's zero logit in the softmax sums") >= 1


# ------------------------------------------------------------------------------------------ GPU
@pytest.fixture(scope="module")
def torch_mod():
    import torch
    assert torch.cuda.is_available(), "the gpu-marked tests need a HIP device"
    return torch


@pytest.fixture(scope="module")
def members(torch_mod):
    """random-weight full-network members by (classes, k), built on first use and shared by the cases: get(classes, K) -> (engines, mean_stds)"""
    from glomeruli_segmentation_amd.engine import EspnetEngine
    cache = {}

    def get(classes, K):
        for k in range(K):
            if (classes, k) not in cache:
                sd, mean, std = member(classes, k)
                cache[classes, k] = (EspnetEngine(sd, classes=classes, p=P_Q[0], q=P_Q[1]), (mean, std))
        return [cache[classes, k][0] for k in range(K)], [cache[classes, k][1] for k in range(K)]
    yield get
    for e, _ in cache.values():
        e.close()


def member_logits(torch, engs, mean_stds, tiles_gpu, images=None):
    """every member's full-resolution logits from its OWN single-model pass over the same tiles (of `images` only, if given)"""
    out = []
    for e, (mean, std) in zip(engs, mean_stds):
        _, _, lg = e.segment(tiles_gpu, mean, std, want_logits=True)
        out.append((lg if images is None else lg[list(images)]).cpu().numpy())
    torch.cuda.synchronize()
    return out


def run_ensemble(torch, engs, mean_stds, tiles_gpu):
    from glomeruli_segmentation_amd.engine import ensemble_segment
    mask, hist = ensemble_segment(engs, tiles_gpu, mean_stds)
    torch.cuda.synchronize()
    return mask.cpu().numpy(), hist.cpu().numpy()


def run_case(torch, members, h, w, n, classes, K, images=None):
    engs, mean_stds = members(classes, K)
    t = torch.from_numpy(case_tiles(h, w, n, classes)).cuda()
    mask, hist = run_ensemble(torch, engs, mean_stds, t)
    check_margin_rule(mask, hist, member_logits(torch, engs, mean_stds, t, images), classes, "%dx%d n%d c%d K%d" % (h, w, n, classes, K), images)
    engs[0].check_device_faults()


@pytest.mark.gpu
@pytest.mark.parametrize("h,w,n,classes,K", FIVE_CASES)
def test_fused_tail_forms(torch_mod, members, h, w, n, classes, K):
    """five classes, dec_tail_kernel in MODE 2 at every launch form: images packed side by side (NRUN 1, 2, 4, 8, short last groups),
    exchanging strip teams of 1 / 2 / 4 / 8 waves with partial and idle strips, overlapping strips plus a rest launch; K = 1 (SOLE),
    2 (FIRST, LAST) and 3, 5 (MIDDLE).  (The forward accepts every size from 8 x 8 in steps of 8: none had to be replaced.)"""
    run_case(torch_mod, members, h, w, n, classes, K)


@pytest.mark.gpu
@pytest.mark.parametrize("h,w,n,classes,K", CLASS_CASES)
def test_other_class_counts(torch_mod, members, h, w, n, classes, K):
    """dec4_kernel<CLS, true> at every padded class count (4, 8, 12, 16, 20: four, two and one half-resolution pixels per thread),
    with a ragged last workgroup; the padding planes stay out of the softmax; K = 1, 2, 3 and 8"""
    run_case(torch_mod, members, h, w, n, classes, K)


@pytest.mark.gpu
@pytest.mark.parametrize("h,w,n,classes,K", EDGE_MEMBER_CASES)
def test_edge_weight_members(torch_mod, h, w, n, classes, K):
    """the exchanging five-class tail and dec4_kernel<8, true> with members whose PReLU slopes run from -1 to 1.7 and whose BatchNorm
    weights are negative or zero on a third of the channels: the same margin rule against the members' own logits"""
    from glomeruli_segmentation_amd.engine import EspnetEngine
    ms = [edge_member(classes, k) for k in range(K)]
    engs = [EspnetEngine(sd, classes=classes, p=P_Q[0], q=P_Q[1]) for sd, _, _ in ms]
    try:
        run_case(torch_mod, lambda c, k: (engs, [(mean, std) for _, mean, std in ms]), h, w, n, classes, K)
    finally:
        for e in engs:
            e.close()


def device_cus(torch):
    return int(torch.cuda.get_device_properties(0).multi_processor_count)


@pytest.mark.gpu
@pytest.mark.parametrize("K", BAND_KS)
def test_shifted_last_band_exchange_form(torch_mod, members, K):
    """128 tiles of 56 x 1024: bands of 8 rows over 28, the last one shifted up by four rows that it shares with its neighbour --
    rows whose probabilities must be added once.  The margin rule on three images, the counts on all."""
    h, w, n, classes, _ = BAND_WIDE
    R, bands = tail_band_plan(h // 2, w // 2, n, device_cus(torch_mod))
    print("bands of %d rows x %d over %d" % (R, bands, h // 2))
    assert R * bands > h // 2, "premise: on this device no two bands share a row (R = %d, %d bands, %d rows)" % (R, bands, h // 2)
    run_case(torch_mod, members, h, w, n, classes, K, BAND_WIDE_IMAGES)


@pytest.mark.gpu
@pytest.mark.parametrize("K", BAND_KS)
def test_shifted_last_band_packed_form(torch_mod, members, K):
    """one tall 16-wide tile in the packed form (NRUN 1): bands of five rows, the last one shifted (8208 rows on 256 CUs: 821 bands
    over 4104, one row shared)"""
    h = tall_height(device_cus(torch_mod))
    R, bands = tail_band_plan(h // 2, BAND_TALL_WIDTH // 2, 1, device_cus(torch_mod))
    print("height %d: bands of %d rows x %d over %d" % (h, R, bands, h // 2))
    assert R * bands > h // 2, "premise: no two bands share a row (R = %d, %d bands, %d rows)" % (R, bands, h // 2)
    run_case(torch_mod, members, h, BAND_TALL_WIDTH, 1, 5, K)


@pytest.mark.gpu
@pytest.mark.parametrize("h,w,n,classes", [(40, 520, 3, 5), (24, 104, 2, 7)])
def test_one_member_equals_the_single_model(torch_mod, members, h, w, n, classes):
    """K = 1 runs the ensemble tail (SOLE); its mask equals the same engine's single-model mask outside the margin set of
    truth([its logits]) -- softmax is monotone, so only ties within TAU may fall differently"""
    torch = torch_mod
    engs, mean_stds = members(classes, 1)
    t = torch.from_numpy(case_tiles(h, w, n, classes)).cuda()
    mask, hist = run_ensemble(torch, engs, mean_stds, t)
    single, shist, lg = engs[0].segment(t, *mean_stds[0], want_logits=True)
    torch.cuda.synchronize()
    single, lg = single.cpu().numpy(), lg.cpu().numpy()
    excluded = 0
    for i in range(n):
        _, excl = truth([lg[i]])
        diff = mask[i] != single[i]
        print("c%d image %d: %d pixels differ from the single model, %d outside the margin set (%d pixels)"
              % (classes, i, int(diff.sum()), int((diff & ~excl).sum()), int(excl.sum())))
        assert not (diff & ~excl).any(), i
        assert np.array_equal(hist[i], np.bincount(mask[i].ravel(), minlength=classes))
        excluded += int(excl.sum())
    assert excluded <= MAX_EXCLUDED * n * h * w and int(hist.sum()) == n * h * w
    engs[0].check_device_faults()


@pytest.mark.gpu
@pytest.mark.parametrize("classes,K", CROP_MEMBERS)
def test_crop_entries(torch_mod, members, classes, K):
    """the crop entries with full-network members, net size 64 x 128: the network maps follow the margin rule against the per-crop
    chain crop_preprocess per member (its mean/std) -> forward_logits -> ens_ref; crop-size maps are mask_resize_nearest of the network
    maps and the counts their bincount, exactly; the host pipeline with pageable and with pinned inputs and the device-resident entry
    (gs_espnet_ensemble_segment_crops) agree bit for bit"""
    torch = torch_mod
    from glomeruli_segmentation_amd import _lib
    from glomeruli_segmentation_amd.engine import crop_preprocess, mask_resize_nearest, segment_crops_host
    engs, mean_stds = members(classes, K)
    NH, NW = NET_H, NET_W
    crops = crop_inputs(classes)
    r = segment_crops_host(engs, mean_stds, crops, NH, NW, 2, want_net_maps=True)
    lgs = [[] for _ in engs]
    for c in crops:
        for k, (e, (mean, std)) in enumerate(zip(engs, mean_stds)):
            x = crop_preprocess(torch.from_numpy(c).cuda(), mean, std, NH, NW)
            lgs[k].append(e.forward_logits(x[None])[0].cpu().numpy())
    check_margin_rule(r["net_maps"], None, [np.stack(l) for l in lgs], classes, "crops c%d K%d" % (classes, K))
    for i, c in enumerate(crops):
        h, w = c.shape[:2]
        back = mask_resize_nearest(torch.from_numpy(r["net_maps"][i]).cuda(), h, w).cpu().numpy()
        assert np.array_equal(back, r["masks"][i]), i
        assert np.array_equal(np.bincount(back.ravel(), minlength=classes), r["counts"][i]), i
    # pinned inputs, one batch
    r2 = segment_crops_host(engs, mean_stds, [torch.from_numpy(c).pin_memory() for c in crops], NH, NW, 64, want_net_maps=True)
    assert np.array_equal(r["net_maps"], r2["net_maps"]) and np.array_equal(r["counts"], r2["counts"])
    assert all(np.array_equal(a, b) for a, b in zip(r["masks"], r2["masks"]))
    # the device-resident entry
    descs, ioff, ooff = [], 0, 0
    for c in crops:
        d = _lib.CropDesc()
        d.in_off, d.out_off, d.h, d.w = ioff, ooff, c.shape[0], c.shape[1]
        descs.append(d)
        ioff += c.size
        ooff += (c.shape[0] * c.shape[1] + 3) // 4 * 4
    packed = torch.from_numpy(np.concatenate([c.ravel() for c in crops])).cuda()
    out = torch.zeros(ooff, dtype=torch.uint8, device="cuda")
    net = torch.empty((len(crops), NH, NW), dtype=torch.uint8, device="cuda")
    hist = torch.empty((len(crops), classes), dtype=torch.int64, device="cuda")
    handles = (ctypes.c_void_p * K)(*[e.handle for e in engs])
    means = (ctypes.c_float * (3 * K))(*[float(v) for ms in mean_stds for v in ms[0]])
    stds = (ctypes.c_float * (3 * K))(*[float(v) for ms in mean_stds for v in ms[1]])
    for e in engs:
        e.quiesce()
    _lib.check(engs[0].lib.gs_espnet_ensemble_segment_crops(
        handles, K, packed.data_ptr(), (_lib.CropDesc * len(descs))(*descs), len(descs), means, stds, NH, NW, net.data_ptr(),
        out.data_ptr(), hist.data_ptr(), None, ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)))
    torch.cuda.synchronize()
    assert np.array_equal(net.cpu().numpy(), r["net_maps"]) and np.array_equal(hist.cpu().numpy(), r["counts"])
    o = out.cpu().numpy()
    for d, m in zip(descs, r["masks"]):
        assert np.array_equal(o[d.out_off:d.out_off + d.h * d.w].reshape(d.h, d.w), m)
    engs[0].check_device_faults()
