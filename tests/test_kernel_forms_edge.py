"""The kernel forms of test_kernel_forms_small.py at trained-range PReLU / BatchNorm parameters, and exact logit ties.

Every case of test_kernel_forms.py that is not fold 1 takes conftest.random_state_dict: slopes from uniform(0.05, 0.4), BatchNorm
weights from uniform(0.5, 1.5).  The trained folds hold mostly negative slopes, one to three above 1 (all in conv.act) and a hundred
or two negative BatchNorm weights each -- and exist at ESPNet(5, 2, 8) only.  So of all the copies of the PReLU pin
(`alpha <= 1 ? +inf : -inf`: prelu() of espnet_kernels.h, prelu_med3 / prelu_pin of conv_mfma.h, the packed cls_prelu, the select of
bn_prelu_sel) only dec_tail_kernel's epilogue ever took the -inf side on a card, and the forms that only random weights reach never
saw a negative slope, a slope of 0 or 1, or a negative or zero folded BN scale.  With random weights no two logits are bit-equal
either, so "first maximum wins" (dec_tail.h, dec4_kernel, enc_head.h) was never put to a tie; the ensemble tests exclude near-ties
by their margin rule.  (tests/test_espnet_c_ensemble.py's "P is a vote with exact ties" describes the UNSCALED random members that
file avoids by its GAIN: its cases hold no exact tie outside the excluded margin set, so enc_head_ens.h's argmax gets a tie case
here too.)

The cases are SMALL_CASES with helpers/edge_weights.edge_state_dict applied to the weights (lower-case names: fresh seeds), under
test_kernel_forms.py's unchanged machinery and bounds.  On the CPU: the generator's properties; the fp32 C oracle against float64
at these weights, printed and held to TAU / 4 per stage family (TAU's rule: about four times that error); per PReLU site, the float64
reference with that one PReLU pinned at +inf (max(v, a v): wrong only where a > 1) and with |a| (wrong only where a < 0) breaks a
stage bound -- so a site whose pin were fixed at +inf fails the GPU case; and the tie condition: with tied_state_dict three planes are
bit-equal in float64 and in fp32, the group is the maximum on at least 5 % (and 8) of the pixels of every checked image, and np.argmax
shows class 0 there and the two copies nowhere.

Two wrong builds were tried once each on an MI355X and not kept.  prelu() of espnet_kernels.h with the pin at +inf whatever the
slope: test_kernel_forms.py, test_kernel_forms_small.py, test_gpu_parity.py, test_espnet_c.py and test_ensemble_full.py pass
(163 tests); every case of test_edge_parameters_against_float64 fails from b2 on (s1: b2 off by 1.3 against a bound of 1.1e-4,
logits by 81 against 1.7e-3), as do test_espnet_c_at_edge_parameters and the float64 part of test_exact_ties_single_model.
`>=` in place of `>` at all six argmax sites (dec_tail.h twice, dec4_kernel twice, enc_head.h, enc_head_ens.h): the same files and
test_espnet_c_ensemble.py pass but for test_gpu_parity.test_full_batch_properties (full-size fold-1 tiles hold a few chance ties
at dec_tail_kernel's single-model site); every test_exact_ties_* case here fails, thirteen of thirteen, and nothing else.
"""
from functools import lru_cache

import numpy as np
import pytest

from conftest import random_state_dict
from helpers.edge_weights import SLOPES, act_keys, bn_keys, edge_state_dict, tied_state_dict
from test_kernel_forms import (RANDOM_MEAN_STD, TAU, Case, DeviceCase, batch_for, bounds_discriminate, case_tile, case_weights,
                               plan, reference, stage_errors)
from test_kernel_forms_small import LARGE_CASES, SMALL_CASES, checked_images, planted_errors

EDGE_CASES = [c._replace(name=c.name.lower(), weights="edge") for c in SMALL_CASES]
LARGE_NAMES = {c.name.lower() for c in LARGE_CASES}
# the single-model tie cases: (case, site).  n256 is the batch here, every image of it is checked; p = q = 1
TIE_CASES = [
    Case("x1", "edge", 5, 1, 1, 16, 16, 3, {"dec_conv": "dec_tail_kernel"}, set()),        # dec_tail, images packed side by side
    Case("x2", "edge", 5, 1, 1, 16, 136, 2, {"dec_conv": "dec_tail_kernel"}, set()),       # dec_tail, exchanging strips (W/2 = 68)
    Case("x3", "edge", 7, 1, 1, 24, 104, 2, {"dec3": "dec3_kernel", "dec_conv": "MFMA MT16"}, set()),        # dec4_kernel<8>
    Case("x4", "edge", 20, 1, 1, 8, 32, 2, {"dec3": "MFMA MT32+F_VEC", "dec_conv": "MFMA MT32+F_VEC"}, set()),   # dec4_kernel<20>
]
MIN_TIED_SHARE, MIN_TIED_PIXELS = 0.05, 8


def ids(c):
    return c.name


# ---------------------------------------------------------------------------------------------- the generator
def test_edge_cases_are_the_small_cases():
    assert len(EDGE_CASES) == len(SMALL_CASES) == 16 and len({c.name for c in EDGE_CASES + TIE_CASES + SMALL_CASES}) == 2 * 16 + 4
    for c, s in zip(EDGE_CASES, SMALL_CASES):
        assert c[2:] == s[2:] and c.weights == "edge"
        assert plan(c.n256, c.H, c.W, c.p, c.q, c.classes, 256) == c.targets, c.name
    for c in TIE_CASES:
        hit = plan(c.n256, c.H, c.W, c.p, c.q, c.classes, 256)
        assert all(hit[k] == v for k, v in c.targets.items()), (c.name, hit)


@pytest.mark.parametrize("case", EDGE_CASES + TIE_CASES, ids=ids)
def test_generator_properties(case):
    """every act tensor of seven channels or more holds all seven kinds of slope, a smaller one a slope above 1 and one below 0;
    every BatchNorm weight holds negative and zero entries; nothing else changed; the rewrite is deterministic"""
    plain = random_state_dict(case.p, case.q, classes=case.classes, seed=7)
    sd = edge_state_dict(plain)
    again = edge_state_dict(random_state_dict(case.p, case.q, classes=case.classes, seed=7))
    assert list(sd) == list(plain) and all(np.array_equal(sd[k], again[k]) and sd[k].dtype == plain[k].dtype for k in sd)
    acts, bns = act_keys(sd), bn_keys(sd)
    assert len(acts) == 10 + case.p + case.q and len(bns) == len(acts) + 1           # (br has no activation)
    assert SLOPES.dtype == np.float32 and SLOPES[4] > 1 and SLOPES[4] - np.float32(1) == np.float32(2.0 ** -23)
    for k in acts:
        a = sd[k]
        assert a.dtype == np.float32 and set(a.tolist()) <= set(SLOPES.tolist()), k
        if len(a) >= 7:
            assert set(a.tolist()) == set(SLOPES.tolist()), k
            for group in (4, 16, 64):       # every kind on every lane position of the kernels' channel groupings
                if len(a) >= 7 * group:
                    for lane in range(group):
                        assert set(a[lane::group].tolist()) == set(SLOPES.tolist()), (k, group, lane)
        else:
            assert (a > 1.5).any() and (a < 0).any(), k
    for k in bns:
        w = sd[k]
        assert (w < 0).any() and (w == 0).any() and (w > 0).any() or len(w) == 2, k
        assert (w < 0).any() and (w == 0).any(), k
        assert np.array_equal(np.abs(w)[w != 0], np.abs(plain[k])[w != 0]), k
        if len(w) >= 33:
            assert 0.2 <= (w < 0).mean() <= 0.4 and 0.05 <= (w == 0).mean() <= 0.13, k
    for k in sd:
        if k not in acts and k not in bns:
            assert sd[k] is plain[k], k


# ---------------------------------------------------------------------------------------------- bounds
@pytest.mark.parametrize("case", EDGE_CASES, ids=ids)
def test_bounds_discriminate_at_edge_parameters(case):
    """test_bounds_discriminate_on_small_maps with the edge weights, under the same TAU.  TAU's rule is "about four times the fp32
    oracle's own worst error against float64": the fp32 C oracle's error on the case's first synthetic and first noise tile is
    printed per stage and held to TAU / 4 (relative to max(1, max|ref64|), as the bound is), so TAU stands for these weights.
    (Measured over the sixteen cases, two tiles each: at most 0.21 of the bound -- logits of one case; b2, level3 and combine_t
    reach 0.20, level2 0.16, up_l3, up_l2 and conv 0.15, level2_0 0.13, level3_0 0.11, sample2 and b1 0.07 -- so no family gets
    a bound of its own.)"""
    bounds_discriminate(case, planted_errors(case))
    from oracle import espnet_oracle as orc
    sd, mean, std = case_weights(case)
    for k in (0, 1):
        tile = case_tile(case, k)
        ref = {name: v[0] for name, v in reference(case, sd, mean, std, tile[None]).items()}
        st = {}
        st["logits"] = orc.espnet_forward(orc.preprocess(tile, mean, std), sd, case.p, case.q, st)
        st["combine_t"] = orc.br(np.concatenate([st["level3_C"], st["up_l3"]], 0), sd, "combine_l2_l3.0")
        errors = stage_errors(case, {name: st[name] for name in ref}, ref)
        print("case %s tile %d, fp32 C oracle vs float64 at edge weights, error / TAU bound: %s; max|activation| %.3g" % (
            case.name, k, ", ".join("%s %.2f" % (n, e / b) for n, (e, b) in errors.items()),
            max(float(np.abs(v).max()) for v in ref.values())))
        for name, (e, b) in errors.items():
            assert e <= ORACLE_SHARE_OF_TAU * b, (case.name, k, name, e / b)


# what the fp32 C oracle's own error may take of a TAU bound for TAU to stand ("about four times" that error); measured 0.21
ORACLE_SHARE_OF_TAU = 0.25


# ---------------------------------------------------------------------------------------------- every PReLU site is driven
class PinnedPrelu:
    """torch.nn.functional with prelu at ONE weight tensor replaced by max(v, a v): the kernels' median form with the pin at
    +inf whatever the slope, wrong only where a > 1"""

    def __init__(self, target):
        import torch
        self.torch, self.target = torch, target

    def __getattr__(self, name):
        return getattr(self.torch.nn.functional, name)

    def prelu(self, x, w):
        if w is self.target:
            return self.torch.maximum(x, w.view(1, -1, 1, 1) * x)
        return self.torch.nn.functional.prelu(x, w)


def worst_ratio(case, wrong, ref):
    return max(e / b for e, b in stage_errors(case, wrong, ref).values())


@pytest.mark.parametrize("case", EDGE_CASES + TIE_CASES, ids=ids)
def test_every_prelu_site_is_driven(case, monkeypatch):
    """Per act tensor, the float64 reference of the case's first two tiles with that one PReLU computed as max(v, a v) -- the +inf
    pin for every slope -- and with the slope |a|: each breaks the bound of a stage the engine holds or of the logits.  So a kernel
    that took the wrong side at slopes above 1, or lost a slope's sign, at ANY site fails the case on the GPU."""
    from oracle import espnet_torch_port as port
    sd, mean, std = case_weights(case)
    tiles = np.stack([case_tile(case, 0), case_tile(case, 1)])
    ref = reference(case, sd, mean, std, tiles)
    sd64 = port.cast_state_dict(sd)
    assert port.cast_state_dict(sd64)["conv.act.weight"] is sd64["conv.act.weight"]      # (PinnedPrelu finds its tensor by identity)
    lines = []
    for key in act_keys(sd):
        assert (sd[key] > 1).any() and (sd[key] < 0).any(), key
        with monkeypatch.context() as mp:
            mp.setattr(port, "F", PinnedPrelu(sd64[key]))
            pinned = worst_ratio(case, reference(case, sd64, mean, std, tiles), ref)
        unsigned = worst_ratio(case, reference(case, dict(sd, **{key: np.abs(sd[key])}), mean, std, tiles), ref)
        lines.append("%s %.1e %.1e" % (key[:-len(".act.weight")], pinned, unsigned))
        assert pinned > 1 and unsigned > 1, (case.name, key, pinned, unsigned)
    same = reference(case, sd64, mean, std, tiles)
    assert all(np.array_equal(same[k], ref[k]) for k in ref)
    print("case %s, worst error / bound with the pin at +inf and with |a|: %s" % (case.name, "; ".join(lines)))


# ---------------------------------------------------------------------------------------------- ties
def most_frequent_inner_class(planes, classes):
    """planes: per image [C, h, w] of a float64 reference.  The most frequent class other than 0 and classes - 1: the first
    maximum over the inner classes' planes, counted over all images (the two outer planes are about to be overwritten)"""
    best = np.concatenate([1 + np.asarray(lg)[1:classes - 1].argmax(0).ravel() for lg in planes])
    return int(np.bincount(best, minlength=classes).argmax())


def bit_equal(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes()


def check_tie_condition(planes, winner, what):
    """planes [n, C, h, w] of a reference: 0, winner and C - 1 bit-equal; the group the maximum on >= 5 % and >= 8 pixels of every
    image; np.argmax (first maximum) 0 there and never winner or C - 1.  -> the share per image"""
    last = planes.shape[1] - 1
    assert bit_equal(planes[:, 0], planes[:, winner]) and bit_equal(planes[:, 0], planes[:, last]), what
    shares = []
    for i, lg in enumerate(planes):
        tied = lg[0] >= lg.max(0)
        cls = lg.argmax(0)
        assert tied.sum() >= max(MIN_TIED_PIXELS, MIN_TIED_SHARE * tied.size), (what, i, int(tied.sum()), tied.size)
        assert (cls[tied] == 0).all() and not np.isin(cls, (winner, last)).any(), (what, i)
        shares.append(float(tied.mean()))
    return shares


@lru_cache(maxsize=None)
def tied_weights(name):
    """((tied state dict, mean, std), winner) of a tie case: the edge weights plus the tie at the float64 reference's most
    frequent inner class over the case's images"""
    case = {c.name: c for c in TIE_CASES}[name]
    sd, mean, std = case_weights(case)
    tiles = np.stack([case_tile(case, k) for k in range(case.n256)])
    winner = most_frequent_inner_class(reference(case, sd, mean, std, tiles)["logits"], case.classes)
    return (tied_state_dict(sd, "classifier.weight", winner), mean, std), winner


@pytest.mark.parametrize("case", TIE_CASES, ids=ids)
def test_tie_condition(case):
    from oracle import espnet_oracle as orc
    (sd, mean, std), winner = tied_weights(case.name)
    tiles = np.stack([case_tile(case, k) for k in range(case.n256)])
    ref64 = reference(case, sd, mean, std, tiles)["logits"]
    ref32 = np.stack([orc.espnet_forward(orc.preprocess(t, mean, std), sd, case.p, case.q) for t in tiles])
    assert ref64.dtype == np.float64 and ref32.dtype == np.float32
    s64 = check_tie_condition(ref64, winner, case.name + " float64")
    s32 = check_tie_condition(ref32, winner, case.name + " fp32")
    print("case %s: classes 0, %d and %d tied; the group is the maximum on %s (float64), %s (fp32) of the pixels" % (
        case.name, winner, case.classes - 1, ["%.2f" % s for s in s64], ["%.2f" % s for s in s32]))


# ESPNet-C: (classes, p, q, seed) at 8 x 8 and 136 x 264, the sizes tests/test_espnet_c.py uses; two noise tiles each
ENC_EDGE = [(5, 2, 3, 6105), (7, 2, 3, 6107), (20, 2, 3, 6120)]
ENC_SIZES = [(8, 8), (136, 264)]
ENC_TIE_CLASSES = (5, 20)
ENC_N = 2
# the 1/8 logits follow b3 and a 1x1 convolution: test_kernel_forms.py's bound of the level-3 family, whose rule (four times the
# fp32 C oracle's error) test_espnet_c_edge_reference holds at these weights
ENC_TAU = TAU["level3"]


def enc_full_sd(classes, p, q, seed):
    return edge_state_dict(random_state_dict(p, q, classes=classes, seed=seed))


def enc_tiles(classes, h, w):
    from glomeruli_segmentation_amd.synth import noise_tile
    return np.stack([noise_tile(61000 + 101 * classes + 7 * h + k, h, w) for k in range(ENC_N)])


def enc_reference(sd, p, q, tiles):
    """float64 1/8 logits [n, C, h/8, w/8] of the encoder of a full state dict"""
    from oracle import espnet_torch_port as port
    stages = {}
    port.forward64(tiles, sd, *RANDOM_MEAN_STD, p, q, stages)
    return stages["enc_classifier"].numpy()


@lru_cache(maxsize=None)
def enc_tied(classes, h, w):
    """(full tied state dict, winner, p, q): the winner is the most frequent inner class of the float64 x8-upsampled planes"""
    from test_espnet_c import upsample64
    _, p, q, seed = [e for e in ENC_EDGE if e[0] == classes][0]
    sd = enc_full_sd(classes, p, q, seed)
    winner = most_frequent_inner_class([upsample64(lg) for lg in enc_reference(sd, p, q, enc_tiles(classes, h, w))], classes)
    return tied_state_dict(sd, "encoder.classifier.conv.weight", winner), winner, p, q


@pytest.mark.parametrize("classes,p,q,seed", ENC_EDGE)
def test_espnet_c_edge_reference(classes, p, q, seed):
    """the fp32 C oracle's 1/8 logits against float64 at the edge weights: at most a quarter of ENC_TAU's bound; and at the tie
    sizes the tie condition on the x8-upsampled planes (float64 of the float64 logits, head_ref of the fp32 ones)"""
    from oracle import espnet_oracle as orc
    from test_espnet_c import encoder_sd, head_ref, upsample64
    for h, w in ENC_SIZES:
        tiles = enc_tiles(classes, h, w)
        versions = [("edge", enc_full_sd(classes, p, q, seed), None)]
        if classes in ENC_TIE_CLASSES:
            sd, winner, _, _ = enc_tied(classes, h, w)
            versions.append(("tied", sd, winner))
        for what, sd, winner in versions:
            ref = enc_reference(sd, p, q, tiles)
            got = np.stack([orc.espnet_encoder_forward(orc.preprocess(t, *RANDOM_MEAN_STD), encoder_sd(sd), p, q) for t in tiles])
            err, scale = float(np.abs(got - ref).max()), max(1.0, float(np.abs(ref).max()))
            print("ESPNet-C c%d %dx%d %s: fp32 C oracle vs float64 %.2e, bound %.2e (max|logit| %.3g)" % (classes, h, w, what, err, ENC_TAU * scale, scale))
            assert err <= ENC_TAU * scale / 4
            if winner is not None:
                s64 = check_tie_condition(np.stack([upsample64(lg) for lg in ref]), winner, "c%d %dx%d float64" % (classes, h, w))
                s32 = check_tie_condition(np.stack([head_ref(lg) for lg in got]), winner, "c%d %dx%d fp32" % (classes, h, w))
                print("    classes 0, %d and %d tied; the group is the maximum on %s (float64), %s (fp32)" % (winner, classes - 1, s64, s32))


# ensembles of tied members: (height, width, n, classes, K); members are test_ensemble_full.member's with the edge rewrite
ENS_TIE_CASES = [(16, 16, 3, 5, 2), (16, 16, 3, 5, 3), (16, 136, 2, 5, 3), (24, 104, 2, 7, 2), (24, 104, 2, 7, 3)]
ENC_ENS_TIE_CASES = [(136, 264, 2, 5, 2), (64, 64, 1, 5, 3)]


def ens_members(classes, K, winner=None):
    """K x (state dict, mean, std): test_ensemble_full.member with the edge rewrite, tied at `winner` if given"""
    from test_ensemble_full import member
    out = []
    for k in range(K):
        sd, mean, std = member(classes, k)
        sd = edge_state_dict(sd)
        out.append((sd if winner is None else tied_state_dict(sd, "classifier.weight", winner), mean, std))
    return out


@lru_cache(maxsize=None)
def ens_oracle_logits(h, w, n, classes, K, winner=None):
    from oracle import espnet_oracle as orc
    from test_ensemble_full import P_Q, case_tiles
    tiles = case_tiles(h, w, n, classes)
    return [np.stack([orc.espnet_forward(orc.preprocess(t, mean, std), sd, *P_Q) for t in tiles]) for sd, mean, std in ens_members(classes, K, winner)]


def ens_winner(h, w, n, classes, K):
    """the most frequent inner class of the float64 ensemble of the UNTIED members' (fp32 C oracle) logits"""
    from test_ensemble_full import ens_ref
    lgs = ens_oracle_logits(h, w, n, classes, K)
    return most_frequent_inner_class([ens_ref([lg[i] for lg in lgs]) for i in range(n)], classes)


def enc_ens_members(classes, K, winner=None):
    """K x (encoder state dict, mean, std): test_espnet_c_ensemble.member (its GAIN keeps the softmax soft) with the edge rewrite"""
    from test_espnet_c_ensemble import member
    out = []
    for k in range(K):
        sd, mean, std = member(classes, k)
        sd = edge_state_dict(sd)
        out.append((sd if winner is None else tied_state_dict(sd, "classifier.conv.weight", winner), mean, std))
    return out


@lru_cache(maxsize=None)
def enc_ens_oracle_logits(h, w, n, classes, K, winner=None):
    from oracle import espnet_oracle as orc
    from test_espnet_c_ensemble import P_Q, case_tiles
    tiles = case_tiles(h, w, n, classes)
    return [np.stack([orc.espnet_encoder_forward(orc.preprocess(t, mean, std), sd, *P_Q) for t in tiles])
            for sd, mean, std in enc_ens_members(classes, K, winner)]


def enc_ens_winner(h, w, n, classes, K):
    from test_espnet_c_ensemble import ens_head_ref
    lgs = enc_ens_oracle_logits(h, w, n, classes, K)
    return most_frequent_inner_class([ens_head_ref([lg[i] for lg in lgs]) for i in range(n)], classes)


def check_ensemble_tie(P, mask, winner, tau, what):
    """P float64 [C, H, W] from tied members: where planes 0, winner and C - 1 tie exactly and exceed every other class by more than
    tau the mask (if given: else P's first maximum) shows class 0; nowhere does it show the two copies.  -> pixels of that set"""
    last = P.shape[0] - 1
    others = np.delete(P, (0, winner, last), axis=0).max(0)
    sure = (P[0] == P[winner]) & (P[0] == P[last]) & (P[0] - others > tau)
    m = P.argmax(0) if mask is None else mask
    assert (m[sure] == 0).all(), (what, int((m[sure] != 0).sum()))
    assert not np.isin(m, (winner, last)).any(), (what, np.bincount(m.ravel(), minlength=last + 1))
    return int(sure.sum())


@pytest.mark.parametrize("h,w,n,classes,K", ENS_TIE_CASES)
def test_ensemble_tie_condition(h, w, n, classes, K):
    """from the fp32 C oracle's logits of the tied members: every member's three planes are bit-equal, and the float64 ensemble
    ties exactly, more than TAU above the rest, on at least 5 % and 8 of the pixels of every image"""
    from test_ensemble_full import TAU as ENS_TAU, ens_ref
    winner = ens_winner(h, w, n, classes, K)
    lgs = ens_oracle_logits(h, w, n, classes, K, winner)
    for lg in lgs:
        assert bit_equal(lg[:, 0], lg[:, winner]) and bit_equal(lg[:, 0], lg[:, classes - 1])
    for i in range(n):
        sure = check_ensemble_tie(ens_ref([lg[i] for lg in lgs]), None, winner, ENS_TAU, (h, w, classes, K, i))
        print("%dx%d c%d K%d image %d: classes 0, %d, %d tie exactly and lead by > TAU on %d of %d pixels" % (h, w, classes, K, i, winner, classes - 1, sure, h * w))
        assert sure >= max(MIN_TIED_PIXELS, MIN_TIED_SHARE * h * w)


@pytest.mark.parametrize("h,w,n,classes,K", ENC_ENS_TIE_CASES)
def test_espnet_c_ensemble_tie_condition(h, w, n, classes, K):
    """the same for the ESPNet-C members, through ens_head_ref (head_ref's fp32 upsampling, then float64)"""
    from test_espnet_c_ensemble import TAU as ENS_TAU, ens_head_ref
    winner = enc_ens_winner(h, w, n, classes, K)
    lgs = enc_ens_oracle_logits(h, w, n, classes, K, winner)
    for lg in lgs:
        assert bit_equal(lg[:, 0], lg[:, winner]) and bit_equal(lg[:, 0], lg[:, classes - 1])
    for i in range(n):
        sure = check_ensemble_tie(ens_head_ref([lg[i] for lg in lgs]), None, winner, ENS_TAU, (h, w, classes, K, i))
        print("%dx%d c%d K%d image %d: classes 0, %d, %d tie exactly and lead by > TAU on %d of %d pixels" % (h, w, classes, K, i, winner, classes - 1, sure, h * w))
        assert sure >= max(MIN_TIED_PIXELS, MIN_TIED_SHARE * h * w)


# ---------------------------------------------------------------------------------------------- the GPU cases
@pytest.mark.gpu
@pytest.mark.parametrize("case", EDGE_CASES, ids=ids)
def test_edge_parameters_against_float64(case):
    """Every small-map case at the edge weights through DeviceCase.forward: the batch that takes the case's forms on this device,
    the checked images' stages and logits within TAU's bounds of float64, the mask the first-max argmax of the returned logits,
    the counts its bincount, the mask-only kernels the same, no device fault.
    (Tried once with a build whose prelu() pins +inf whatever the slope -- `fmed3f(v, alpha * v, +inf)`: all sixteen cases fail,
    from b2 on -- the first stage a prelu() caller writes; the module docstring has the figures.)"""
    with DeviceCase(case) as dev:
        n = batch_for(case, dev.num_cus)
        assert (n > 1) == (case.name in LARGE_NAMES)
        dev.forward(n, checked_images(n))


def as_bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


@pytest.mark.gpu
@pytest.mark.parametrize("case", TIE_CASES, ids=ids)
def test_exact_ties_single_model(case):
    """Three bit-equal logit planes -- 0, the winner and the last class -- at the edge weights: dec_tail_kernel's argmax in the packed
    and in the exchanging form, dec4_kernel<8> and dec4_kernel<20>.  DeviceCase.forward holds stages and logits to float64 and the
    mask to np.argmax (first maximum) of the returned logits, the counts to its bincount and the mask-only run to the same bytes;
    here: the three returned planes are bit-equal, the group is the maximum on at least 5 % of every image, and the two copies
    appear nowhere in masks or counts.  A `>=` in place of `>` shows the last class on every such pixel."""
    weights, winner = tied_weights(case.name)
    last, n = case.classes - 1, case.n256
    with DeviceCase(case, weights) as dev:
        mask, hist, logits = dev.forward(n, list(range(n)))
    lg, m, hist = logits.numpy(), mask.numpy(), hist.numpy()
    assert np.array_equal(as_bits(lg[:, 0]), as_bits(lg[:, winner])) and np.array_equal(as_bits(lg[:, 0]), as_bits(lg[:, last]))
    assert np.array_equal(m, lg.argmax(1).astype(np.uint8))
    for i in range(n):
        tied = lg[i, 0] >= lg[i].max(0)
        assert tied.sum() >= max(MIN_TIED_PIXELS, MIN_TIED_SHARE * tied.size), (case.name, i, int(tied.sum()))
        assert (m[i][tied] == 0).all(), (case.name, i)
    assert not np.isin(m, (winner, last)).any(), np.bincount(m.ravel(), minlength=case.classes)
    assert not hist[:, winner].any() and not hist[:, last].any()


@pytest.fixture(scope="module")
def torch_mod():
    import torch
    assert torch.cuda.is_available(), "the gpu-marked tests need a HIP device"
    return torch


def run_encoder(torch, sd, classes, p, q, tiles):
    """an ESPNet-C engine of the encoder of `sd` over the tiles -> (mask, hist, 1/8 logits), the equalities of test_espnet_c.py
    asserted (check_head: the mask IS the first max of head_ref(logits), the counts its bincount) and the mask-only run the same"""
    from glomeruli_segmentation_amd.engine import EspnetEngine
    from test_espnet_c import check_head, encoder_sd
    eng = EspnetEngine(encoder_sd(sd), classes=classes, p=p, q=q, encoder_only=True)
    try:
        t = torch.from_numpy(tiles).cuda()
        mask, hist, logits = eng.segment(t, *RANDOM_MEAN_STD, want_enc_logits=True)
        torch.cuda.synchronize()
        mask, hist, logits = mask.cpu().numpy(), hist.cpu().numpy(), logits.cpu().numpy()
        check_head(mask, hist, logits, classes, "c%d %dx%d" % ((classes,) + tiles.shape[1:3]))
        m2, h2, _ = eng.segment(t, *RANDOM_MEAN_STD)
        torch.cuda.synchronize()
        assert np.array_equal(m2.cpu().numpy(), mask) and np.array_equal(h2.cpu().numpy(), hist)
        eng.check_device_faults()
    finally:
        eng.close()
    return mask, hist, logits


@pytest.mark.gpu
@pytest.mark.parametrize("classes,p,q,seed", ENC_EDGE)
def test_espnet_c_at_edge_parameters(torch_mod, classes, p, q, seed):
    """ESPNet-C heads at 5, 7 and 20 classes with the edge weights, 8 x 8 and 136 x 264: test_espnet_c.py's equalities, and the 1/8
    logits within ENC_TAU of float64 (b3's PReLU and the classifier run in the encoder-only forms here)"""
    sd = enc_full_sd(classes, p, q, seed)
    for h, w in ENC_SIZES:
        tiles = enc_tiles(classes, h, w)
        _, _, logits = run_encoder(torch_mod, sd, classes, p, q, tiles)
        ref = enc_reference(sd, p, q, tiles)
        err, scale = float(np.abs(logits - ref).max()), max(1.0, float(np.abs(ref).max()))
        print("ESPNet-C c%d %dx%d: 1/8 logits vs float64 %.2e, bound %.2e" % (classes, h, w, err, ENC_TAU * scale))
        assert err <= ENC_TAU * scale


@pytest.mark.gpu
@pytest.mark.parametrize("classes", ENC_TIE_CLASSES)
def test_exact_ties_espnet_c(torch_mod, classes):
    """enc_head_kernel's argmax: the 1/8 logit planes 0, winner and last bit-equal (rows of the classifier copied), so their x8
    upsampled values are; the mask is the first max of head_ref(logits) (check_head), never one of the copies; their counts are 0"""
    from test_espnet_c import head_ref
    for h, w in ENC_SIZES:
        sd, winner, p, q = enc_tied(classes, h, w)
        mask, hist, logits = run_encoder(torch_mod, sd, classes, p, q, enc_tiles(classes, h, w))
        last = classes - 1
        assert np.array_equal(as_bits(logits[:, 0]), as_bits(logits[:, winner])) and np.array_equal(as_bits(logits[:, 0]), as_bits(logits[:, last]))
        for i in range(ENC_N):
            v = head_ref(logits[i])
            tied = v[0] >= v.max(0)
            assert tied.sum() >= max(MIN_TIED_PIXELS, MIN_TIED_SHARE * tied.size), (classes, h, w, i, int(tied.sum()))
            assert (mask[i][tied] == 0).all()
        assert not np.isin(mask, (winner, last)).any() and not hist[:, winner].any() and not hist[:, last].any()


@pytest.mark.gpu
@pytest.mark.parametrize("h,w,n,classes,K", ENS_TIE_CASES)
def test_exact_ties_ensemble(torch_mod, h, w, n, classes, K):
    """K members, all tied on classes 0, winner and last: dec_tail_kernel MODE 2 (packed and exchanging) and dec4_kernel<8, true>.
    With every member's own logits (bit-equal planes) the float64 ens_ref ties exactly; where the group leads by more than
    test_ensemble_full.TAU the mask shows class 0, and nowhere the copies; counts are the mask's."""
    torch = torch_mod
    from glomeruli_segmentation_amd.engine import EspnetEngine
    from test_ensemble_full import P_Q, TAU as ENS_TAU, case_tiles, ens_ref, member_logits, run_ensemble
    winner = ens_winner(h, w, n, classes, K)
    ms = ens_members(classes, K, winner)
    engs = [EspnetEngine(sd, classes=classes, p=P_Q[0], q=P_Q[1]) for sd, _, _ in ms]
    try:
        mean_stds = [(mean, std) for _, mean, std in ms]
        t = torch.from_numpy(case_tiles(h, w, n, classes)).cuda()
        mask, hist = run_ensemble(torch, engs, mean_stds, t)
        lgs = member_logits(torch, engs, mean_stds, t)
        engs[0].check_device_faults()
    finally:
        for e in engs:
            e.close()
    last = classes - 1
    for lg in lgs:
        assert np.array_equal(as_bits(lg[:, 0]), as_bits(lg[:, winner])) and np.array_equal(as_bits(lg[:, 0]), as_bits(lg[:, last]))
    for i in range(n):
        sure = check_ensemble_tie(ens_ref([lg[i] for lg in lgs]), mask[i], winner, ENS_TAU, (h, w, classes, K, i))
        assert sure >= max(MIN_TIED_PIXELS, MIN_TIED_SHARE * h * w), (i, sure)
        assert np.array_equal(hist[i], np.bincount(mask[i].ravel(), minlength=classes))
    assert not hist[:, winner].any() and not hist[:, last].any()


@pytest.mark.gpu
@pytest.mark.parametrize("h,w,n,classes,K", ENC_ENS_TIE_CASES)
def test_exact_ties_espnet_c_ensemble(torch_mod, h, w, n, classes, K):
    """enc_head_ens.h's argmax: K ESPNet-C members, all tied on the same three classes.  ens_head_ref of the members' own 1/8 logits
    ties exactly; the mask shows class 0 where the group leads by more than test_espnet_c_ensemble.TAU, and the copies nowhere."""
    torch = torch_mod
    from glomeruli_segmentation_amd.engine import EspnetEngine
    from test_espnet_c_ensemble import P_Q, TAU as ENS_TAU, case_tiles, ens_head_ref, member_logits, run_ensemble
    winner = enc_ens_winner(h, w, n, classes, K)
    ms = enc_ens_members(classes, K, winner)
    engs = [EspnetEngine(sd, classes=classes, p=P_Q[0], q=P_Q[1], encoder_only=True) for sd, _, _ in ms]
    try:
        mean_stds = [(mean, std) for _, mean, std in ms]
        t = torch.from_numpy(case_tiles(h, w, n, classes)).cuda()
        mask, hist = run_ensemble(torch, engs, mean_stds, t)
        lgs = member_logits(torch, engs, mean_stds, t)
        engs[0].check_device_faults()
    finally:
        for e in engs:
            e.close()
    last = classes - 1
    for lg in lgs:
        assert np.array_equal(as_bits(lg[:, 0]), as_bits(lg[:, winner])) and np.array_equal(as_bits(lg[:, 0]), as_bits(lg[:, last]))
    for i in range(n):
        sure = check_ensemble_tie(ens_head_ref([lg[i] for lg in lgs]), mask[i], winner, ENS_TAU, (h, w, classes, K, i))
        assert sure >= max(MIN_TIED_PIXELS, MIN_TIED_SHARE * h * w), (i, sure)
        assert np.array_equal(hist[i], np.bincount(mask[i].ravel(), minlength=classes))
    assert not hist[:, winner].any() and not hist[:, last].any()
