"""The kernel forms of test_kernel_forms.py on maps smaller than the dilations.

test_kernel_forms.py's cases start at 136 x 1040: H/4 >= 34 and H/8 >= 17, so no output row loses both outer tap rows of a
dilation, every row is at least a strip long, and every launch has more tasks than the device has wave slots.  The forward
accepts any multiple of 8 from 8 up.  The cases here are the shapes that only small tiles reach: level-2 maps of 2 to 26
rows (F_SKIP_PAD drops both d16 tap rows of every output row, so a dead chunk is followed by the dead first chunk of the
next task), level-3 maps of 1 to 13 rows (all of d16's and d8's outer taps in the halo; at 8 x 8 only centre taps read
data), rows of 1 to 20 pixels (most lanes of a strip off the row, also in the +F_VEC forms), a lone last row of the
stride-2 reduce, and at one tile launches of fewer than eight tasks.  The large-batch forms need many tasks, not many
pixels: 205 tiles of 40 x 80 are 2 MB.

Everything is test_kernel_forms.py's own machinery (the planner, the seeds, the float64 reference, the bounds TAU); only the
table of cases, the images checked per batch and the planted weight errors are new.
"""
import numpy as np
import pytest

from test_kernel_forms import (D16_ROW2_AND_K_TAIL, L2_SKIP, L2_SMALL, L2_VEC, L3_SMALL, P2R, SWEEP_BATCHES, Case, DeviceCase,
                               batch_for, bounds_discriminate, edges, form_table, output_width, plan, reachable_forms)

# ---------------------------------------------------------------------------------------------- the cases
# n256: the smallest batch that takes the targets at 256 CUs, by hand from plan_forward's inequalities --
#   small2: n * H/4 * cdiv(W/4, 64) * 2 <= 4 * cus      small3: n * H/8 * cdiv(W/8, 64) * 2 <= 8 * cus
#   (the stride-2 reduce leaves its 32-pixel form earlier: n * H/8 * cdiv(W/8, 128) * 4 <= 8 * cus)
# so the large-batch forms start past small3: S1 2048 / (5 * 2) = 204.8, S2 2048 / (9 * 2) = 113.8, S3 2048 / (13 * 2) = 78.8,
# S4 2048 / 2 = 1024.  test_small_case_batches_at_256_cus holds them to the planner.
P4, P2F = "CFG_L2_BR_P4", "CFG_L3_BR_P2F"
LARGE_VEC = {"l2_down": L2_SKIP, "l2_esp_fused": L2_VEC, "l2_esp_last": L2_VEC, "l3_reduce": "CFG_L3_C1S_BNL",
             "l3_down": P2R, "l3_esp_fused": P2R, "l3_esp_last": P2R, "dec3": "dec3_kernel", "dec_conv": "dec_tail_kernel"}
LARGE_ODD = {"l2_down": P4, "l2_esp_fused": P4, "l2_esp_last": P4, "l3_reduce": "CFG_L3_C1S_BNL",
             "l3_down": P2F, "l3_esp_fused": P2F, "l3_esp_last": "CFG_L3_BR_P2", "dec3": "dec3_kernel", "dec_conv": "dec_tail_kernel"}
SMALL = {"l2_down": L2_SMALL, "l2_esp_fused": L2_SMALL, "l2_esp_last": L2_SMALL, "l3_reduce": "CFG_L3_C1S_BNL_P1",
         "l3_down": L3_SMALL, "l3_esp_fused": L3_SMALL, "l3_esp_last": L3_SMALL, "dec3": "dec3_kernel", "dec_conv": "dec_tail_kernel"}
UNFUSED = {"l2_down": "unfused CFG_L2_BR_P4", "cat_b2": "cat_b2_kernel", "l3_reduce": "CFG_L3_C1S"}
# the large-batch forms (classes 5: the fused tail and the reduce's side sums run too)
LARGE_CASES = [
    # H/4 = 10: both d16 tap rows of every output row are dead.  H/8 = 5, W/8 = 10
    Case("S1", "random", 5, 2, 3, 40, 80, 205, LARGE_VEC, {"lone_row", "ragged_task"}),
    # H/4 = 18: d16's tap row 0 is live only for y = 16, 17 and its row 2 only for y = 0, 1.  Odd W/8 = 9 and H/8 = 9
    Case("S2", "random", 5, 2, 3, 72, 72, 114, LARGE_ODD, {"lone_row", "ragged_task"}),
    # H/4 = 26.  Rows of 4 pixels at level 2 and of 2 at level 3; H/8 = 13
    Case("S3", "random", 5, 2, 3, 104, 16, 79, LARGE_VEC, {"lone_row", "ragged_task"}),
    # a 2 x 2 level-2 map and a 1 x 1 level-3 map: only centre taps read data
    Case("S4", "random", 5, 2, 3, 8, 8, 1025, LARGE_ODD, {"lone_row", "ragged_task"}),
]
# the small-batch forms at one tile: 1, 5, 9 or 2 level-3 tasks of 32 pixels in a launch, fewer than the eight XCDs or barely more
FEW_TASK_CASES = [
    Case("T1", "random", 5, 2, 3, 8, 8, 1, SMALL, {"lone_row", "ragged_task"}),
    Case("T2", "random", 5, 2, 3, 40, 80, 1, SMALL, {"lone_row", "ragged_task"}),
    Case("T3", "random", 5, 2, 3, 72, 72, 1, SMALL, {"lone_row", "ragged_task"}),
    Case("T4", "random", 5, 2, 3, 8, 264, 1, SMALL, {"lone_row", "ragged_task"}),
]
# the forms no batch size gates, at one tile; the targets are the planner's whole answer, written down
UNGATED_CASES = [
    # the unfused down-samplers, cat_b2_kernel, CFG_L3_C1S, MT 32 dec3 and dec_conv
    Case("U1", "random", 20, 0, 0, 8, 8, 1,
         dict(UNFUSED, l3_down="unfused CFG_L3_BR", dec3="MFMA MT32", dec_conv="MFMA MT32+F_VEC"), {"lone_row", "ragged_task"}),
    Case("U2", "random", 20, 0, 0, 40, 72, 1,
         dict(UNFUSED, l3_down="unfused CFG_L3_BR", dec3="MFMA MT32", dec_conv="MFMA MT32+F_VEC"), {"lone_row", "ragged_task"}),
    # W/4 = 8 and W/8 = 4, multiples of the four pixels per lane of the unfused down-samplers and of MT 32 dec3: their vector forms
    Case("U3", "random", 20, 0, 0, 8, 32, 1,
         dict(UNFUSED, l2_down="unfused CFG_L2_BR_P4+F_VEC", l3_down="unfused CFG_L3_BR+F_VEC", dec3="MFMA MT32+F_VEC",
              dec_conv="MFMA MT32+F_VEC"), {"lone_row", "ragged_task"}),
    # MT 16 with and without +F_VEC; the only level-3 block is the last
    Case("V1", "random", 12, 1, 1, 40, 80, 1,
         {"l2_down": L2_SMALL, "l2_esp_last": L2_SMALL, "l3_reduce": "CFG_L3_C1S_BNL_P1", "l3_down": L3_SMALL,
          "l3_esp_last": L3_SMALL, "dec3": "MFMA MT16", "dec_conv": "MFMA MT16+F_VEC"}, {"lone_row", "ragged_task"}),
    Case("V2", "random", 12, 1, 1, 8, 16, 1,
         {"l2_down": L2_SMALL, "l2_esp_last": L2_SMALL, "l3_reduce": "CFG_L3_C1S_BNL_P1", "l3_down": L3_SMALL,
          "l3_esp_last": L3_SMALL, "dec3": "MFMA MT16", "dec_conv": "MFMA MT16+F_VEC"}, {"lone_row", "ragged_task"}),
    # W/4 = 8: dec3's MT 16 vector form, on a 2 x 8 map
    Case("V3", "random", 12, 1, 1, 8, 32, 1,
         {"l2_down": L2_SMALL, "l2_esp_last": L2_SMALL, "l3_reduce": "CFG_L3_C1S_BNL_P1", "l3_down": L3_SMALL,
          "l3_esp_last": L3_SMALL, "dec3": "MFMA MT16+F_VEC", "dec_conv": "MFMA MT16+F_VEC"}, {"lone_row", "ragged_task"}),
    # dec3_kernel and dec4_kernel on a 2 x 2 and an 18 x 18 map
    Case("W1", "random", 7, 0, 1, 8, 8, 1,
         dict(UNFUSED, l3_down=L3_SMALL, l3_esp_last=L3_SMALL, dec3="dec3_kernel", dec_conv="MFMA MT16"), {"lone_row", "ragged_task"}),
    Case("W2", "random", 7, 0, 1, 72, 72, 1,
         dict(UNFUSED, l3_down=L3_SMALL, l3_esp_last=L3_SMALL, dec3="dec3_kernel", dec_conv="MFMA MT16"), {"lone_row", "ragged_task"}),
]
SMALL_CASES = LARGE_CASES + FEW_TASK_CASES + UNGATED_CASES
# the forms the planner returns at H <= 104 that no case above takes, each with the reason
NOT_RUN_ON_SMALL_MAPS = {}
# the heights and batches the planner is swept over for that statement: 1, 2, 5, 9 and 13 level-3 rows, and batches on both
# sides of every threshold above
SMALL_SWEEP_HEIGHTS = (8, 16, 40, 72, 104)
SMALL_SWEEP_BATCHES = SWEEP_BATCHES + (79, 114, 205, 1025)


def second_batch(n):
    """the larger batch of a large-batch case: more than twice the tiles, an odd count"""
    return 2 * n + 3


def checked_images(n):
    """the first, the last and 14 evenly spaced in between; all of them up to 16"""
    return sorted({(k * (n - 1) + 7) // 15 for k in range(16)}) if n > 16 else list(range(n))


def test_checked_images():
    assert checked_images(1) == [0] and checked_images(16) == list(range(16))
    for n in (17, 79, 205, 1025, 2053):
        picks = checked_images(n)
        assert len(picks) == 16 and picks[0] == 0 and picks[-1] == n - 1
        assert max(np.diff(picks)) - min(np.diff(picks)) <= 1


# ---------------------------------------------------------------------------------------------- the plan
def test_small_case_batches_at_256_cus():
    assert len({c.name for c in SMALL_CASES}) == len(SMALL_CASES)
    assert {c.name: batch_for(c, 256) for c in SMALL_CASES} == {c.name: c.n256 for c in SMALL_CASES}
    for c in SMALL_CASES:
        assert c.weights == "random"
        assert c.edges == edges(c.H, c.W), c.name
        # the targets are the planner's whole answer, not a part of it
        assert plan(c.n256, c.H, c.W, c.p, c.q, c.classes, 256) == c.targets, c.name
    for c in LARGE_CASES:   # the larger batch runs the same forms
        assert plan(second_batch(c.n256), c.H, c.W, c.p, c.q, c.classes, 256) == c.targets, c.name
        assert plan(c.n256 - 1, c.H, c.W, c.p, c.q, c.classes, 256) != c.targets, c.name
    for c in FEW_TASK_CASES:   # fewer level-3 tasks of 32 pixels than twice the eight XCDs, or than the XCDs themselves
        assert (c.H // 8) * -(-(c.W // 8) // 32) <= 9


def test_small_cases_reach_what_they_are_for():
    """From the planner, over the whole table: the skip form on maps whose every row loses a d16 tap row; vector forms only
    where their pixels per lane divide the output width; and every form the planner returns at H <= 104 has a case."""
    skip = [c for c in SMALL_CASES if c.targets.get("l2_down") == L2_SKIP]
    assert {c.name for c in skip} == {"S1", "S3"} and all(c.H // 4 <= 32 for c in skip)
    assert any(c.H // 4 <= 16 for c in skip)        # both d16 tap rows of every row dead
    table = form_table()
    vector = 0
    for c in SMALL_CASES:
        for cls, form in c.targets.items():
            P = table[cls][form]
            assert (P > 0) == ("+F_VEC" in form)
            if P:
                vector += 1
                assert output_width(cls, c.W) % P == 0, (c.name, cls, form, P)
    assert vector >= 20
    hit = set()
    for c in SMALL_CASES:
        hit.update(c.targets.items())
    every = reachable_forms(256, SMALL_SWEEP_HEIGHTS, SMALL_SWEEP_BATCHES)
    assert every == reachable_forms(256)            # small maps take every form large ones do, and no other
    assert hit <= every, sorted(hit - every)
    assert every - hit == set(NOT_RUN_ON_SMALL_MAPS), sorted((every - hit) ^ set(NOT_RUN_ON_SMALL_MAPS))


# ---------------------------------------------------------------------------------------------- bounds
def planted_errors(case):
    """The weight errors the bounds must reject, in the first level-3 block (bounds_discriminate): test_kernel_forms.py
    zeroes the bottom tap row of d16, but a map of H/8 <= 16 rows never reads it (y + 16 < H/8 for no row).  Here it is the
    bottom tap row of the widest dilation that some row still reads, d < H/8 -- the row a wrong tap-row decision would drop --
    and on the 1 x 1 map, where no dilation reads anything but its centre tap, d16's centre tap.  The K-tail error stays."""
    H3 = case.H // 8
    live = [d for d in (1, 2, 4, 8, 16) if d < H3]
    first = ("d%d.conv.weight" % live[-1], (slice(None), slice(None), 2)) if live else \
        ("d16.conv.weight", (slice(None), slice(None), 1, 1))
    return (first, D16_ROW2_AND_K_TAIL[1])


@pytest.mark.parametrize("case", SMALL_CASES, ids=lambda c: c.name)
def test_bounds_discriminate_on_small_maps(case):
    """test_bounds_discriminate on the small shapes: the fp32 C oracle passes every stage bound, and the bounds reject the
    1e-4 bump in a stage's last column, a zeroed tap row (planted_errors) and the dropped last input channel of the level-3
    reduce."""
    bounds_discriminate(case, planted_errors(case))


# ---------------------------------------------------------------------------------------------- the GPU cases
@pytest.mark.gpu
@pytest.mark.parametrize("case", LARGE_CASES, ids=lambda c: c.name)
def test_large_batch_forms_on_small_maps(case):
    """The smallest batch that takes the large-batch forms, 16 images of it held to float64 (DeviceCase.forward); then more
    than twice the batch, whose first tiles are the same: their logits, masks and counts are the same bits (what
    test_small_batch_task_shapes_give_the_same_bits states), and its last image is held to float64.  The skip form rotates
    the rows of every other group of images, and where the groups begin depends on the grid: two batches put images on both
    sides of it under a check without the test knowing the grid.
    (Tried once with a build whose F_SKIP_PAD refill steps over one dead chunk instead of all of them: every level-2 stage of
    test_kernel_forms.py's cases still passes -- from H/4 = 34 on no two dead chunks are neighbours -- and S1 fails from
    level2_0 on, error 0.2 against a bound of 6e-6.)"""
    import torch
    with DeviceCase(case) as dev:
        n = batch_for(case, dev.num_cus)
        mask, hist, logits = dev.forward(n, checked_images(n))
        n2 = second_batch(n)
        mask2, hist2, logits2 = dev.forward(n2, [n2 - 1])
        assert torch.equal(logits2[:n], logits), case.name
        assert torch.equal(mask2[:n], mask) and torch.equal(hist2[:n], hist), case.name


@pytest.mark.gpu
@pytest.mark.parametrize("case", FEW_TASK_CASES + UNGATED_CASES, ids=lambda c: c.name)
def test_one_tile_forms_on_small_maps(case):
    """One tile: launches of fewer tasks than the device has XCDs or wave slots, in the small-batch forms and in the forms no
    batch size gates."""
    with DeviceCase(case) as dev:
        assert batch_for(case, dev.num_cus) == 1
        dev.forward(1, [0])
