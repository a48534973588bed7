"""One process with a variant build of the library loaded: python variant_forms_child.py <variant> <plan|gpu>

Started by tests/test_variant_forms.py (helpers/variant_builds.py, run_child) with GLOMSEG_LIB / GLOMSEG_EXPERIMENT and the
variant's own environment set, because the process that runs pytest has loaded the shipped library.  Everything it does is
test_kernel_forms.py's machinery on the variant's cases; it prints one JSON line per answer.

plan (no device): {"lib", "build_flags", "reached": the forms a planner sweep returns}, then per case {"case", "n256":
    batch_for(case, 256), "plan": the plan at that batch, "plan_at_tiles": the plan at the batch a run takes on 256 CUs}.
gpu: per case {"case", "ok", "n", "num_cus", "forms": the planned forms of that batch, "worst": {stage: [error, bound]},
    "ratio": the worst error / bound, "error"}.  DeviceCase.forward holds every stage the engine keeps and the logits of
    checked_images(n) to float64 under bound(), the mask to the first-max argmax with flips below the margin only, the counts,
    the mask-only kernels and the device fault word.  A failed assertion is the case's answer and the next case runs; any other
    error (a HIP error, a refusal of the library) ends the process with status 70 and nothing more goes to the card.
"""
import json
import os
import sys
import traceback

HERE = os.path.dirname(os.path.abspath(__file__))
TESTS = os.path.dirname(HERE)
REPO = os.path.dirname(TESTS)
for path in (TESTS, REPO):
    if path not in sys.path:
        sys.path.insert(0, path)


def say(**answer):
    print(json.dumps(answer), flush=True)


def main(variant, mode):
    from glomeruli_segmentation_amd import _lib
    from helpers.variant_builds import CHILD_GAVE_UP, lib_path, variant_cases
    import test_kernel_forms as tkf
    assert os.path.samefile(_lib.LIB_PATH, lib_path(variant)), (_lib.LIB_PATH, lib_path(variant))
    lib = _lib.load()
    cases = variant_cases(variant)
    if mode == "plan":
        say(lib=_lib.LIB_PATH, build_flags=lib.gs_build_flags(), reached=sorted(tkf.reachable_forms(256)))
        for vc in cases:
            c = vc.case
            n = tkf.batch_for(c, 256)
            say(case=c.name, n256=n, plan=tkf.plan(n, c.H, c.W, c.p, c.q, c.classes, 256),
                plan_at_tiles=tkf.plan(max(n, vc.tiles), c.H, c.W, c.p, c.q, c.classes, 256))
        return 0
    assert mode == "gpu", mode
    for vc in cases:
        c = vc.case
        answer = {"case": c.name, "ok": False, "lib": _lib.LIB_PATH}
        dev, gave_up = None, False
        try:
            dev = tkf.DeviceCase(c)
            n = max(tkf.batch_for(c, dev.num_cus), vc.tiles)
            answer.update(n=n, num_cus=dev.num_cus, forms=tkf.plan(n, c.H, c.W, c.p, c.q, c.classes, dev.num_cus))
            dev.forward(n, tkf.checked_images(n))
            answer["ok"] = True
        except AssertionError:
            answer["error"] = traceback.format_exc()[-1500:]
        except BaseException:
            answer["error"] = traceback.format_exc()[-1500:]
            gave_up = True
        worst = getattr(dev, "worst", None) or {}
        answer["worst"] = {k: list(eb) for k, eb in worst.items()}
        answer["ratio"] = max([e / b for e, b in worst.values()], default=None)
        say(**answer)
        if gave_up:
            return CHILD_GAVE_UP
        if dev is not None:
            dev.eng.close()
    return 0


if __name__ == "__main__":
    sys.exit(main(sys.argv[1], sys.argv[2]))
