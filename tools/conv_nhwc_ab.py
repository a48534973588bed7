#!/usr/bin/env python3
"""Interleaved A/B of the detector half on one MI355X: the cfg-3 legs of tools/bench_aux.py (per-layer gs_conv2d_nhwc at batch 16,
gs_roialign, gs_detector_forward on sixteen 1000x1000 windows) for another build of the library and the shipped one, in turn
(A B A B ...), one fresh process per run.  Prints every round, both medians and A's own max - min spread per leg:
    python tools/conv_nhwc_ab.py variants_so/libglomseg_parent.so [rounds] > profiles/conv_nhwc_ab.json
Across an ABI change the binding refuses the parent's library: pass the parent's built checkout (a directory) instead, and its
own tools/bench_aux.py runs on its own library.
The bar is A: B's median has to lie within A's spread of A's median."""
import json
import os
import statistics
import subprocess
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def legs(j):
    out = {"conv2d_nhwc " + c["shape"]: c["ms"] for c in j["cfg3_conv2d_nhwc_batch16"]}
    out["roialign 300x14x14x128"] = round(j["cfg3_roialign_300x14x14x128"]["us"] / 1e3, 4)
    out["detector_forward batch16 1000x1000"] = j["cfg3_detector_forward_batch16_1000x1000"]["ms_per_batch"]
    return out


def main():
    libs = {"parent": sys.argv[1], "new": os.path.join(REPO, "glomeruli_segmentation_amd", "libglomseg.so")}
    rounds = int(sys.argv[2]) if len(sys.argv) > 2 else 5
    runs = {name: [] for name in libs}
    for _ in range(rounds):
        for name, lib in libs.items():
            tree = lib if os.path.isdir(lib) else REPO
            env = dict(os.environ) if os.path.isdir(lib) else dict(os.environ, GLOMSEG_EXPERIMENT="1", GLOMSEG_LIB=lib)
            p = subprocess.run([sys.executable, os.path.join(tree, "tools", "bench_aux.py"), "--cfg3"], env=env, capture_output=True,
                               text=True, timeout=240)
            if p.returncode != 0:                      # nothing more on the GPU after a failure
                sys.exit("%s failed (%d):\n%s" % (name, p.returncode, p.stderr[-2000:]))
            runs[name].append(legs(json.loads(p.stdout)))
            print(name, runs[name][-1], file=sys.stderr, flush=True)
    table = {}
    for leg in runs["parent"][0]:
        a, b = [r[leg] for r in runs["parent"]], [r[leg] for r in runs["new"]]
        spread = max(a) - min(a)
        table[leg] = {"unit": "ms", "parent": a, "new": b, "parent_median": statistics.median(a), "new_median": statistics.median(b),
                      "parent_spread": round(spread, 4), "within_parent_spread": abs(statistics.median(b) - statistics.median(a)) <= spread}
    print(json.dumps({"libs": {k: os.path.relpath(v, REPO) for k, v in libs.items()}, "rounds": rounds, "legs": table}, indent=1))


if __name__ == "__main__":
    main()
