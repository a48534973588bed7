#!/usr/bin/env python3
"""Resident rate of a five-member ESPNet-C ensemble (K trunks + ONE enc_head_ens_kernel launch, csrc/enc_head_ens.h), beside a
single ESPNet-C pass and beside the five-member full-ESPNet ensemble -- interleaved in one process, the five folds' weights, each
with its own mean/std, 32 resident 1024x512 uint8 synth tiles -> masks + counts:

  (a) espnet_c_ensemble   engine.ensemble_segment over five ESPNet-C engines            model passes = 5 per tile
  (b) espnet_c            one ESPNet-C engine's segment (stem .. dec1 + enc_head_kernel)  model passes = 1 per tile
  (c) espnet_ensemble     engine.ensemble_segment over five full engines (fp32 probability accumulator, decoder tails)

Every leg: `--repeats` timed repeats of `--iters` calls, the legs taking turns repeat by repeat; the JSON holds every repeat and the
median, in model passes per second.  The relation it states: (a) passes/s / (b) passes/s -- what a member costs inside the ensemble
against alone -- beside the same ratio of the full network, (c) passes/s / the full network's single pass rate.  The ensemble head's
own time comes from the library's per-kernel HIP events (gs_espnet_profile_read on the first member), beside the single-model
head's and the members' trunk kernels.

    python tools/espnet_c_ensemble_rate.py [--out profiles/espnet_c_ensemble_rate.json]
"""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
from glomeruli_segmentation_amd.engine import EspnetEngine, ensemble_segment  # noqa: E402
from glomeruli_segmentation_amd.synth import FOLD_MEAN_STD, synth_tile  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--tiles", type=int, default=32)
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--iters", type=int, default=5)
    a = ap.parse_args()
    n, K = a.tiles, 5
    sds = []
    for k in range(1, K + 1):
        z = np.load(os.path.join(REPO, "tests", "golden", "weights_fold%d.npz" % k))
        sds.append({name: z[name] for name in z.files})
    mean_stds = [FOLD_MEAN_STD[k] for k in range(1, K + 1)]
    encs = [EspnetEngine({k[len("encoder."):]: v for k, v in sd.items() if k.startswith("encoder.")}, encoder_only=True) for sd in sds]
    fulls = [EspnetEngine(sd) for sd in sds]
    tiles = torch.from_numpy(np.stack([synth_tile(k) for k in range(n)])).cuda()
    out_m = torch.empty((n, 512, 1024), dtype=torch.uint8, device="cuda")
    out_h = torch.empty((n, 5), dtype=torch.int64, device="cuda")
    last = {}

    def ens(engs, tag):
        def run():
            for _ in range(a.iters):
                last[tag] = ensemble_segment(engs, tiles, mean_stds)
            return a.iters * n * K
        return run

    def single(eng):
        def run():
            for _ in range(a.iters * K):          # as many model passes as an ensemble repeat
                eng.segment(tiles, *mean_stds[0], out_mask=out_m, out_hist=out_h)
            return a.iters * n * K
        return run

    legs = [("espnet_c_ensemble", ens(encs, "c")), ("espnet_c", single(encs[0])), ("espnet_ensemble", ens(fulls, "f")),
            ("espnet", single(fulls[0]))]
    for _, run in legs:      # warm-up: workspaces, the accumulator, torch's allocator
        run()
    torch.cuda.synchronize()
    assert int(last["c"][1].sum()) == n * 512 * 1024 and int(last["f"][1].sum()) == n * 512 * 1024
    times = {name: [] for name, _ in legs}
    for _ in range(a.repeats):
        for name, run in legs:
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            passes = run()
            torch.cuda.synchronize()
            times[name].append((time.perf_counter() - t0) / passes)
    result = {"what": __doc__.split("\n\n")[0], "device": torch.cuda.get_device_name(0), "tiles": n, "members": K,
              "iters_per_repeat": a.iters, "rows": []}
    med = {}
    for name, _ in legs:
        rates = [1.0 / t for t in times[name]]
        med[name] = statistics.median(rates)
        row = {"leg": name, "tiles": n, "model_passes_per_s_median": round(med[name], 1),
               "model_passes_per_s_repeats": [round(r, 1) for r in rates]}
        result["rows"].append(row)
        print(row, flush=True)
    # per-kernel HIP events: the first member times its trunk and the ensemble head; then the same engine alone (its own head)
    encs[0].profile(True)
    for _ in range(a.iters):
        ensemble_segment(encs, tiles, mean_stds)
    kern_ens = {k["name"]: round(k["total_ms"] / k["launches"] * 1e3, 2) for k in encs[0].profile_read() if k["launches"]}
    for _ in range(a.iters):
        encs[0].segment(tiles, *mean_stds[0], out_mask=out_m, out_hist=out_h)
    kern_one = {k["name"]: round(k["total_ms"] / k["launches"] * 1e3, 2) for k in encs[0].profile_read() if k["launches"]}
    encs[0].profile(False)
    trunk_us = sum(v for k, v in kern_ens.items() if k != "enc_head_ens_kernel")
    result["kernels_us"] = {"member_0_in_the_ensemble": kern_ens, "member_0_alone": kern_one,
                            "ensemble_head_us": kern_ens.get("enc_head_ens_kernel"), "single_head_us": kern_one.get("enc_head_kernel"),
                            "member_trunk_us": round(trunk_us, 2),
                            "head_share_of_ensemble_kernel_time": round(kern_ens.get("enc_head_ens_kernel", 0.0) / (K * trunk_us + kern_ens.get("enc_head_ens_kernel", 0.0)), 4)}
    print(result["kernels_us"], flush=True)
    result["relations"] = {
        "espnet_c_ensemble_over_single_espnet_c": round(med["espnet_c_ensemble"] / med["espnet_c"], 4),
        "espnet_ensemble_over_single_espnet": round(med["espnet_ensemble"] / med["espnet"], 4),
        "espnet_c_ensemble_over_espnet_ensemble": round(med["espnet_c_ensemble"] / med["espnet_ensemble"], 4)}
    print(result["relations"], flush=True)
    encs[0].check_device_faults()
    for e in encs + fulls:
        e.close()
    if a.out:
        with open(a.out, "w") as f:
            json.dump(result, f, indent=1)
    return 0


if __name__ == "__main__":
    sys.exit(main())
