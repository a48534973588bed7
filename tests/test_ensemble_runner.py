"""What the one ensemble runner (csrc/espnet.hip run_ensemble) and the per-lane probability accumulator must keep doing: the
same bits whichever lane a batch runs on, an accumulator that grows under a call without changing an earlier call's answer, lanes
that can be dropped and made again, and -- on the CPU -- the role predicates and the role a member gets (csrc/gs_internal.h).

Two full five-class networks (folds 1 and 2), net size 64 x 128, five crops of which three are network-sized."""
import os
import shutil
import subprocess

import numpy as np
import pytest

from conftest import REPO, load_weights

NH, NW = 64, 128
CROP_SHAPES = [(64, 128), (64, 128), (150, 99), (40, 52), (64, 128)]
FOLDS = (1, 2)


def make_engines(lanes):
    from glomeruli_segmentation_amd.engine import EspnetEngine
    return [EspnetEngine(load_weights(f), lanes=lanes) for f in FOLDS]


def run_crops(engs, case, batch):
    from glomeruli_segmentation_amd.engine import segment_crops_host
    return segment_crops_host(engs, case["ms"], case["crops"], NH, NW, batch=batch, want_net_maps=True)


def assert_same(a, b):
    assert len(a["masks"]) == len(b["masks"])
    for i, (x, y) in enumerate(zip(a["masks"], b["masks"])):
        assert np.array_equal(x, y), i
    assert np.array_equal(a["net_maps"], b["net_maps"]) and np.array_equal(a["counts"], b["counts"])


@pytest.fixture(scope="module")
def case():
    """the inputs, two-lane engines, and their answer with batch = 1 (five batches that alternate lanes): computed once"""
    import torch
    assert torch.cuda.is_available(), "the gpu-marked tests need a HIP device"
    from glomeruli_segmentation_amd.synth import FOLD_MEAN_STD, synth_tile
    c = {"ms": [FOLD_MEAN_STD[f] for f in FOLDS],
         "crops": [synth_tile(700 + k, h, w, blobs=3) for k, (h, w) in enumerate(CROP_SHAPES)]}
    c["engs"] = make_engines(2)
    c["two_lanes"] = run_crops(c["engs"], c, batch=1)
    yield c
    for e in c["engs"]:
        e.close()


@pytest.mark.gpu
def test_per_lane_accumulator(case):
    """lane 0 and lane 1 accumulate in allocations of their own: the batches that ran on alternating lanes (two compute streams) give
    the bits of the same engines with one lane, and the network-sized crops give gs_espnet_ensemble_forward's masks and counts"""
    import torch
    from glomeruli_segmentation_amd.engine import ensemble_segment
    engs, two = case["engs"], case["two_lanes"]
    for e in engs:
        e.set_lanes(1)
    try:
        one = run_crops(engs, case, batch=1)
    finally:
        for e in engs:
            e.set_lanes(2)
    assert_same(two, one)
    same = [i for i, s in enumerate(CROP_SHAPES) if s == (NH, NW)]
    assert len(same) == 3
    mask, hist = ensemble_segment(engs, torch.from_numpy(np.stack([case["crops"][i] for i in same])).cuda(), case["ms"])
    for j, i in enumerate(same):
        assert np.array_equal(mask[j].cpu().numpy(), two["net_maps"][i]), i
        assert np.array_equal(mask[j].cpu().numpy(), two["masks"][i]), i
        assert np.array_equal(hist[j].cpu().numpy(), two["counts"][i]), i


@pytest.mark.gpu
def test_accumulator_growth_across_entries(case):
    """one engine list, one lane: gs_espnet_ensemble_forward on 1 tile, then the crop entry with batches of 3 (lane 0's accumulator
    has to grow), then the tile again -- the tile's answer does not change, and the crops' is a fresh engine list's"""
    import torch
    from glomeruli_segmentation_amd.engine import ensemble_segment
    tile = torch.from_numpy(case["crops"][0][None]).cuda()
    engs, fresh = make_engines(1), make_engines(1)
    try:
        m1, h1 = ensemble_segment(engs, tile, case["ms"])
        r = run_crops(engs, case, batch=3)
        m3, h3 = ensemble_segment(engs, tile, case["ms"])
        assert torch.equal(m1, m3) and torch.equal(h1, h3)
        assert_same(r, run_crops(fresh, case, batch=3))
    finally:
        for e in engs + fresh:
            e.close()


@pytest.mark.gpu
def test_lane_teardown(case):
    """lanes that held an accumulator are dropped (set_lanes(1)) and made again: the same answer before and after, and close() returns"""
    engs = make_engines(2)
    try:
        before = run_crops(engs, case, batch=1)
        assert_same(before, case["two_lanes"])
        for n in (1, 2):
            for e in engs:
                e.set_lanes(n)
        assert_same(run_crops(engs, case, batch=1), before)
    finally:
        for e in engs:
            e.close()
    assert all(e.handle is None for e in engs)


ROLE_CHECK = r"""
// the role predicates and the runner's role assignment against the literal tests and formulas they replaced
#include <cstdio>
#include "gs_internal.h"
using namespace gs;
int main()
{
    int bad = 0;
    static_assert((int)EnsRole::NONE == 0 && (int)EnsRole::FIRST == 1 && (int)EnsRole::MIDDLE == 2 && (int)EnsRole::LAST == 3 &&
                  (int)EnsRole::SOLE == 4, "the kernels receive these values");
    // rows NONE, FIRST, MIDDLE, LAST, SOLE; columns reads, writes, finishes
    const bool table[5][3] = {{false, false, true}, {false, true, false}, {true, true, false}, {true, false, true}, {false, false, true}};
    for (int m = 0; m <= 4; ++m) {
        const bool reads = m == 2 || m == 3, writes = m == 1 || m == 2;
        const bool zeroes_hist = m == 0 || m >= 3, counts = !(m == 1 || m == 2), dec4_finishes = m == 0 || m >= 3;
        bad += ens_reads(m) != reads || ens_reads(m) != table[m][0];
        bad += ens_writes(m) != writes || ens_writes(m) != table[m][1];
        bad += ens_finishes(m) != zeroes_hist || ens_finishes(m) != counts || ens_finishes(m) != dec4_finishes || ens_finishes(m) != table[m][2];
    }
    for (int K = 1; K <= 8; ++K)
        for (int k = 0; k < K; ++k) {
            const int tiles = K == 1 ? 4 : k == 0 ? 1 : k == K - 1 ? 3 : 2;   // gs_espnet_ensemble_forward's formula
            const int crops = K == 1 ? 0 : k == 0 ? 1 : k == K - 1 ? 3 : 2;   // the crop entries' (they call the runner for K > 1 only)
            bad += (int)ens_role(k, K) != tiles;
            bad += K > 1 && (int)ens_role(k, K) != crops;
        }
    std::printf("role check: %d bad\n", bad);
    return bad ? 1 : 0;
}
"""


def test_role_predicates_on_the_cpu(tmp_path):
    """host only: ens_reads / ens_writes / ens_finishes have, for 0..4, the truth table of the literal tests they replaced, and
    ens_role(k, K) is the formula the two member loops used, K = 1..8.  A stand-alone program, built with the host compiler (for which
    the HIP headers define __host__ / __device__ away)"""
    cxx = shutil.which("g++") or shutil.which("c++") or shutil.which("clang++")
    assert cxx, "no host C++ compiler"
    src, exe = tmp_path / "role_check.cpp", tmp_path / "role_check"
    src.write_text(ROLE_CHECK)
    built = subprocess.run([cxx, "-std=c++17", "-O1", "-Wall", "-D__HIP_PLATFORM_AMD__", "-I/opt/rocm/include",
                            "-I" + os.path.join(REPO, "glomeruli_segmentation_amd", "csrc"), str(src), "-o", str(exe)],
                           capture_output=True, text=True)
    assert built.returncode == 0, built.stderr[-3000:]
    res = subprocess.run([str(exe)], capture_output=True, text=True, timeout=60)
    assert res.returncode == 0 and "role check: 0 bad" in res.stdout, (res.returncode, res.stdout, res.stderr[-1000:])
