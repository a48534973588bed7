"""Hostile PReLU / BatchNorm parameters and exact logit ties for the kernel-form tests (numpy only).

conftest.random_state_dict draws PReLU slopes from uniform(0.05, 0.4) and BatchNorm weights from uniform(0.5, 1.5).  The trained
folds (tests/golden/weights_fold*.npz) hold mostly negative slopes (down to -0.33), a few above 1 (up to 1.68) and a hundred or two
negative BatchNorm weights each.  edge_state_dict rewrites a random state dict so that every PReLU site sees every kind of slope on
every lane position, and every BatchNorm fold sees a negative and a zero scale; tied_state_dict makes three logit planes bit-equal.
"""
import numpy as np

# the seven kinds of slope: trained-range negative, zero (a ReLU), ordinary, exactly 1 (the identity; the last slope that takes the
# +inf side of the kernels' `alpha <= 1` pin), the first fp32 value above 1 (the first that takes the -inf side), the trained
# maximum rounded up, and -1 (|v|)
SLOPES = np.array([-0.33, 0.0, 0.25, 1.0, np.nextafter(np.float32(1.0), np.float32(2.0)), 1.7, -1.0], dtype=np.float32)
# Tensors of fewer than seven channels (the decoder's at five classes and below) start at kind 4: the five channels take
# nextafter(1), 1.7, -1.0, -0.33 and 0.  Of the windows of five consecutive kinds, those starting at 2, 3, 4 and 5 hold 1.7 and a
# negative slope.  Measured on the CPU over the ten five-class cases of tests/test_kernel_forms_edge.py (float64 reference, the +inf
# pin and |a| at combine_l2_l3.1, up_l2.1 and conv): 4 is the only start at which every wrong site breaks a stage bound, by a factor
# of 1e2 at the least; at 5 the pin at up_l2.1 reaches 0.6 of the bound on one case, at 3 the one at conv.act 5.2, and at 2 |a| at
# combine_l2_l3.1 changes nothing on four.  test_every_prelu_site_is_driven holds the choice to its purpose.  (A two-channel tensor
# starts at 5: 1.7 and -1.0.)
SMALL_OFFSET = 4


def act_keys(sd):
    return [k for k in sd if k.endswith(".act.weight")]


def bn_keys(sd):
    """the `weight` keys of the BatchNorm layers"""
    return [k for k in sd if k.endswith(".weight") and k[:-len("weight")] + "running_var" in sd]


def slope_offset(t, channels):
    """offset_t of act tensor number t"""
    return t if channels >= len(SLOPES) else SMALL_OFFSET if channels >= 3 else 5


def edge_state_dict(sd):
    """A deterministic rewrite of a random_state_dict result; running_var, running_mean, bias and the convolutions stay.
    Slopes: channel c of act tensor number t takes kind (c + offset_t) % 7 -- consecutive channels take consecutive kinds, so on the
    4-, 16- and 64-wide channel groupings of the kernels (none a multiple of 7) every kind falls on every lane position.
    BatchNorm weight: channel c of BN tensor number t keeps its magnitude and changes sign where (c + t) % 3 == 1, and becomes
    exactly 0 where (c + t) % 11 == 0 (tensors of fewer than eleven channels: at c = t % channels, and if that leaves no
    negative weight the next channel takes the sign)."""
    out = dict(sd)
    for t, key in enumerate(act_keys(sd)):
        c = np.arange(sd[key].shape[0])
        out[key] = SLOPES[(c + slope_offset(t, len(c))) % len(SLOPES)].copy()
    for t, key in enumerate(bn_keys(sd)):
        w = np.array(sd[key], dtype=np.float32)
        c = np.arange(w.shape[0])
        zero = (c + t) % 11 == 0 if len(c) >= 11 else c == t % len(c)
        flip = ((c + t) % 3 == 1) & ~zero
        if not flip.any():
            flip = c == (int(np.flatnonzero(zero)[0]) + 1) % len(c)
        w[flip] = -w[flip]
        w[zero] = 0.0
        out[key] = w
    return out


def tie_axis(key):
    """the class axis of the last class projection: the deconvolution's weight is [in, out, 2, 2], the 1x1 convolution's [out, in, 1, 1]"""
    return {"classifier.weight": 1, "encoder.classifier.conv.weight": 0, "classifier.conv.weight": 0}[key]


def tied_state_dict(sd, key, winner):
    """`winner`'s slice of the last class projection copied into class 0 and into the last class: three bit-equal logit planes, one
    candidate below the winner and one above it.  First maximum wins: wherever the group is the maximum, the class is 0."""
    w = np.array(sd[key])
    classes = w.shape[tie_axis(key)]
    assert 0 < winner < classes - 1
    w = np.moveaxis(w, tie_axis(key), 0)
    w[0] = w[winner]
    w[classes - 1] = w[winner]
    return dict(sd, **{key: np.ascontiguousarray(np.moveaxis(w, 0, tie_axis(key)))})
