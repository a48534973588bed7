"""ctypes binding of libglomseg.so (the headers under include/: HEADERS).  No fallback: if the HIP library is
missing or fails to load this raises, so a GPU box can never pass on a silent CPU path."""
import ctypes
import os

_PKG = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(_PKG, "libglomseg.so")
# Experiments only (tools/ab.sh): GLOMSEG_LIB names an alternative build of the same sources.  It is honoured only together
# with the explicit opt-in GLOMSEG_EXPERIMENT=1, and a library that reports a diagnostic build (gs_build_flags() &
# GS_BUILD_DIAG: timing variants that return wrong results by construction) is refused unless GLOMSEG_ALLOW_DIAG=1 as well,
# so that no stray environment variable can swap the product library under a test or a benchmark.
if os.environ.get("GLOMSEG_LIB") and os.environ.get("GLOMSEG_EXPERIMENT") == "1":
    LIB_PATH = os.environ["GLOMSEG_LIB"]

GS_OK = 0
GS_IN_U8_BGR_NHWC = 0
GS_IN_F32_NCHW = 1
ABI_VERSION = 10
GS_BUILD_DIAG = 1
GS_BUILD_NO_ODD_2B = 2      # a -DCFG_L3_ODD_2B=0 build: the A/B side of the two-block step of the level-3 branch kernels
GS_FORM_ODD_2B_LEGAL, GS_FORM_ODD_2B_BUILT = 1, 2
GS_FORM_NONE = -1
GS_MAX_ENSEMBLE_C = 8      # most ESPNet-C members of an ensemble (include/glomseg.h)
MAX_CROPS_PER_CALL = 64

STATUS_NAMES = {0: "GS_OK", 1: "GS_ERR_INVALID", 2: "GS_ERR_HIP", 3: "GS_ERR_NOMEM", 4: "GS_ERR_UNSUPPORTED",
                5: "GS_ERR_NODEVICE", 6: "GS_ERR_DEVICE_FAULT"}


class GlomsegError(RuntimeError):
    def __init__(self, status, message):
        super().__init__("%s: %s" % (STATUS_NAMES.get(status, status), message))
        self.status = status


class LayerDesc(ctypes.Structure):
    _fields_ = [("name", ctypes.c_char * 96), ("offset", ctypes.c_int64), ("ndim", ctypes.c_int32),
                ("shape", ctypes.c_int32 * 4)]


class CropDesc(ctypes.Structure):
    _fields_ = [("in_off", ctypes.c_int64), ("out_off", ctypes.c_int64), ("h", ctypes.c_int32), ("w", ctypes.c_int32),
                ("x1", ctypes.c_int32), ("y1", ctypes.c_int32)]


class PasteTarget(ctypes.Structure):
    _fields_ = [("slide_map", ctypes.c_void_p), ("map_h", ctypes.c_int32), ("map_w", ctypes.c_int32), ("ds", ctypes.c_int32),
                ("sx_lut", ctypes.c_void_p), ("sy_lut", ctypes.c_void_p)]


class CropOverlay(ctypes.Structure):
    _fields_ = [("palette_rgb", ctypes.c_void_p), ("n_colours", ctypes.c_int32), ("wa", ctypes.c_float), ("wb", ctypes.c_float),
                ("out_bgr", ctypes.POINTER(ctypes.c_void_p))]


class CropScoring(ctypes.Structure):
    _fields_ = [("labels", ctypes.POINTER(ctypes.c_void_p)), ("conf", ctypes.c_void_p), ("seen", ctypes.c_void_p),
                ("gt_overlay_bgr", ctypes.POINTER(ctypes.c_void_p)), ("gt_clamp", ctypes.c_int32)]


class EvalBox(ctypes.Structure):
    _fields_ = [("x0", ctypes.c_int32), ("y0", ctypes.c_int32), ("x1", ctypes.c_int32), ("y1", ctypes.c_int32),
                ("raster_w", ctypes.c_int32), ("raster_h", ctypes.c_int32), ("offset", ctypes.c_int64)]


class EvalSet(ctypes.Structure):
    _fields_ = [("rasters", ctypes.c_void_p), ("raster_bytes", ctypes.c_int64), ("boxes", ctypes.c_void_p),
                ("n_boxes", ctypes.c_int32), ("win_ptr", ctypes.c_void_p), ("win_idx", ctypes.c_void_p), ("n_idx", ctypes.c_int32),
                ("small_map", ctypes.c_void_p)]


class DetectorLayerPlan(ctypes.Structure):
    _fields_ = [("images", ctypes.c_int64), ("in_h", ctypes.c_int32), ("in_w", ctypes.c_int32), ("out_h", ctypes.c_int32),
                ("out_w", ctypes.c_int32), ("form", ctypes.c_int32)]


class DetectorPlan(ctypes.Structure):
    _fields_ = [("hf", ctypes.c_int32), ("wf", ctypes.c_int32), ("workspace_bytes", ctypes.c_int64), ("n_layers", ctypes.c_int32),
                ("layers", DetectorLayerPlan * 16)]


class DetectorStepArgs(ctypes.Structure):
    """gs_detector_step_args (include/glomseg_detector_steps.h)"""
    _fields_ = [("inp", ctypes.c_void_p * 3), ("out", ctypes.c_void_p * 3), ("n", ctypes.c_int64), ("h", ctypes.c_int32),
                ("w", ctypes.c_int32), ("c", ctypes.c_int32), ("k", ctypes.c_int32), ("stride", ctypes.c_int32), ("pad", ctypes.c_int32),
                ("layer", ctypes.c_int32), ("count", ctypes.c_int32), ("crop", ctypes.c_int32), ("win_h", ctypes.c_float),
                ("win_w", ctypes.c_float)]


class WeightPiece(ctypes.Structure):
    _fields_ = [("name", ctypes.c_char * 32), ("offset", ctypes.c_longlong), ("floats", ctypes.c_longlong)]


class WorkspaceReport(ctypes.Structure):
    _fields_ = [("must_be_zero", ctypes.c_longlong), ("offenders", ctypes.c_longlong), ("piece", ctypes.c_char * 16),
                ("image", ctypes.c_int), ("plane", ctypes.c_int), ("row", ctypes.c_int), ("col", ctypes.c_int), ("bits", ctypes.c_uint)]


class WorkspacePiece(ctypes.Structure):
    _fields_ = [("name", ctypes.c_char * 16), ("offset", ctypes.c_ulonglong), ("own_words", ctypes.c_ulonglong),
                ("span_words", ctypes.c_ulonglong), ("padded", ctypes.c_int)] + \
               [(k, ctypes.c_int) for k in ("C", "Cp", "H", "W", "pitch", "sc", "off")]


class KernelTime(ctypes.Structure):
    _fields_ = [("name", ctypes.c_char * 64), ("total_ms", ctypes.c_double), ("launches", ctypes.c_int64),
                ("flops_per_tile", ctypes.c_double)]


_P = ctypes.c_void_p
_FP = ctypes.POINTER(ctypes.c_float)
_I = ctypes.c_int

PROTOTYPES = {
    "gs_last_error": (ctypes.c_char_p, []),
    "gs_abi_version": (_I, []),
    "gs_build_flags": (_I, []),
    "gs_device_fault_check": (_I, []),
    "gs_espnet_create": (_I, [_P, ctypes.POINTER(LayerDesc), _I, _I, _I, _I, _I, ctypes.POINTER(_P)]),
    "gs_espnet_destroy": (None, [_P]),
    "gs_espnet_reserve": (_I, [_P, _I, _I, _I]),
    "gs_espnet_forward": (_I, [_P, _P, _I, _I, _I, _I, _FP, _FP, _P, _P, _P, _P]),
    "gs_espnet_set_lanes": (_I, [_P, _I]),
    "gs_espnet_lanes": (_I, [_P]),
    "gs_espnet_forward_lane": (_I, [_P, _I, _P, _I, _I, _I, _I, _FP, _FP, _P, _P, _P, _P]),
    "gs_espnet_segment_host": (_I, [_P, _P, _I, _I, _I, _FP, _FP, _I, _P, _P]),
    "gs_espnet_segment_crops": (_I, [_P, _I, _P, ctypes.POINTER(CropDesc), _I, _FP, _FP, _I, _I, _P, _P, _P,
                                ctypes.POINTER(PasteTarget), _P]),
    "gs_espnet_ensemble_segment_crops": (_I, [ctypes.POINTER(_P), _I, _P, ctypes.POINTER(CropDesc), _I, _FP, _FP, _I, _I, _P, _P, _P,
                                         ctypes.POINTER(PasteTarget), _P]),
    "gs_espnet_segment_crops_host": (_I, [ctypes.POINTER(_P), _I, ctypes.POINTER(_P), ctypes.POINTER(_I), ctypes.POINTER(_I), _I, _FP, _FP,
                                     _I, _I, _I, ctypes.POINTER(_P), _P, _P, ctypes.POINTER(PasteTarget), ctypes.POINTER(_I),
                                     ctypes.POINTER(_I), ctypes.POINTER(CropOverlay)]),
    "gs_crops_from_masks": (_I, [_P, ctypes.POINTER(CropDesc), _I, _I, _I, _I, _P, _P, ctypes.POINTER(PasteTarget), _P, _P, _I,
                            ctypes.c_float, ctypes.c_float, _I, _P, _P]),
    "gs_plan_crop_batches": (_I, [ctypes.POINTER(_I), ctypes.POINTER(_I), _I, _I, ctypes.POINTER(_I), _I, ctypes.POINTER(_I)]),
    "gs_host_block_is_pinned": (_I, [_P, ctypes.c_size_t]),
    "gs_espnet_ensemble_forward": (_I, [ctypes.POINTER(_P), _I, _P, _I, _I, _I, _FP, _FP, _P, _P, _P]),
    "gs_espnet_read_stage": (_I, [_P, ctypes.c_char_p, _I, _P, ctypes.c_size_t, ctypes.POINTER(_I * 3)]),
    "gs_espnet_block_forward": (_I, [_P, _I, _I, _I, _P, _I, _I, _P]),
    "gs_espnet_plan_forward": (_I, [_I, _I, _I, _I, _I, _I, _I, ctypes.POINTER(_I), _I, ctypes.POINTER(_I)]),
    "gs_espnet_form_info": (_I, [_I, _I, ctypes.POINTER(ctypes.c_char_p), ctypes.POINTER(_I)]),
    "gs_espnet_profile_enable": (_I, [_P, _I]),
    "gs_espnet_profile_read": (_I, [_P, ctypes.POINTER(KernelTime), _I, ctypes.POINTER(_I)]),
    "gs_crop_preprocess": (_I, [_P, _I, _I, _FP, _FP, _I, _I, _P, _P]),
    "gs_mask_resize_nearest": (_I, [_P, _I, _I, _I, _I, _P, _P]),
    "gs_find_contours": (_I, [_P, _I, _I, _I, _P, _I, _P, _I, ctypes.POINTER(_I), ctypes.POINTER(_I)]),
    "gs_arc_length_closed": (ctypes.c_double, [_P, _I]),
    "gs_approx_poly_closed": (_I, [_P, _I, ctypes.c_double, _P]),
    "gs_wsi_paste_max": (_I, [_P, _I, _I, _I, _P, _I, _I, _I, _I, _P]),
    "gs_wsi_paste_max_lut": (_I, [_P, _I, _I, _I, _P, _P, _P, _I, _I, _I, _I, _P]),
    "gs_overlay_classmap": (_I, [_P, _P, _I, _I, _P, _I, ctypes.c_float, ctypes.c_float, _P, _P]),
    "gs_confusion_u8": (_I, [_P, _P, ctypes.c_longlong, _I, _P, _P]),
    "gs_wsi_eval_windows": (_I, [_I, _I, _I, _I, ctypes.POINTER(EvalSet), ctypes.POINTER(EvalSet), _P, _P, _I, _I, _P, _P, _P]),
    "gs_conv2d_nhwc": (_I, [_P, _I, _I, _I, _I, _P, _I, _I, _I, _P, _I, _I, _I, _P, _P]),
    "gs_conv2d_nhwc_form": (_I, [_I] * 10 + [ctypes.POINTER(ctypes.c_char_p)]),
    "gs_roialign": (_I, [_P, _I, _I, _I, _I, _P, _P, _I, _I, _P, _P]),
    "gs_nms": (_I, [_P, _P, _I, ctypes.c_float, ctypes.c_float, _I, _P, _P, _P]),
    "gs_detector_create": (_I, [_P, ctypes.POINTER(LayerDesc), _I, ctypes.POINTER(_P)]),
    "gs_detector_destroy": (None, [_P]),
    "gs_detector_max_detections": (_I, []),
    "gs_detector_num_proposals": (_I, []),
    "gs_detector_layer_info": (_I, [_I, ctypes.POINTER(ctypes.c_char_p)] + [ctypes.POINTER(_I)] * 6),
    "gs_detector_plan": (_I, [_I, _I, _I, ctypes.POINTER(DetectorPlan)]),
    "gs_detector_set_thresholds": (_I, [_P, ctypes.c_float, ctypes.c_float, ctypes.c_float]),
    "gs_detector_forward": (_I, [_P, _P, _I, _I, _I, _P, _P, _P, _P, _P, _P, _P, _P, _P]),
    "gs_detector_detect_host": (_I, [_P, ctypes.POINTER(_P), _I, _I, _I, _I, _P, _P, _P, _P]),
}

SCORING_PROTOTYPES = {
    "gs_espnet_score_crops": (_I, [_P, _P, ctypes.POINTER(CropDesc), _I, _I, _I, _I, _P, _P, _P]),
    "gs_espnet_segment_crops_host_scored": (_I, PROTOTYPES["gs_espnet_segment_crops_host"][1] + [ctypes.POINTER(CropScoring)]),
}

PLAN_PROTOTYPES = {
    "gs_espnet_plan_flags": (_I, [_I, _I, _I, _I, _I, _I, _I, _I, ctypes.POINTER(_I)]),
    "gs_espnet_pack_weights": (_I, [_P, ctypes.POINTER(LayerDesc), _I, _I, _I, _I, _I, _P, ctypes.c_size_t, ctypes.POINTER(ctypes.c_size_t),
                                ctypes.POINTER(WeightPiece), _I, ctypes.POINTER(_I)]),
    "gs_espnet_workspace_plan": (_I, [_I] * 7 + [ctypes.POINTER(ctypes.c_size_t)]),
}
GS_PLAN_LAZY_B2, GS_PLAN_L3C_IN_REDUCE, GS_PLAN_CLS_IN_L3 = 1, 2, 4

LEAN_PROTOTYPES = {
    "gs_espnet_plan_lean": (_I, [_I] * 9 + [ctypes.POINTER(_I)]),
}

FORMS_PROTOTYPES = {
    "gs_espnet_form_odd_2b": (_I, [_I, _I]),
}

DETECTOR_STEPS_PROTOTYPES = {
    "gs_conv2d_nhwc_pack4": (_I, [_P, _I, _I, _I, _I, _P]),
    "gs_conv2d_nhwc_packed": (_I, [_P, _I, _I, _I, _I, _P, _I, _I, _I, _P, _I, _I, _I, _P, _P]),
    "gs_detector_step_name": (ctypes.c_char_p, [_I]),
    "gs_detector_step": (_I, [_P, ctypes.c_char_p, ctypes.POINTER(DetectorStepArgs), _P]),
}

INSTANCE_PROTOTYPES = {
    "gs_instances_plan": (_I, [_I, _I, _I, _I, ctypes.POINTER(ctypes.c_size_t)]),
    "gs_slide_instances": (_I, [_P, _I, _I, _I, _I, _P, ctypes.c_size_t, _I, _P, _P, _P, _P, _P]),
}

MATCH_PROTOTYPES = {
    "gs_instance_match_plan": (_I, [_I, _I, _I, ctypes.POINTER(ctypes.c_size_t)]),
    "gs_instance_overlaps": (_I, [_P, _P, _P, _P, _I, _I, _P, ctypes.c_size_t, _I, _P, _P, _P, _P]),
    "gs_instance_match": (_I, [_P, _P, _P, _I, _P, _I, _P, _I, _I, _I, _I, _P, _P, _P]),
}

BOUNDARY_PROTOTYPES = {
    "gs_boundary_dist_plan": (_I, [_I, _I, ctypes.POINTER(ctypes.c_size_t)]),
    "gs_instance_boundary_dist": (_I, [_P, _P, _P, _I, _P, _I, _I, _I, _P, ctypes.c_size_t, _P, _P, _P, _P]),
}

MORPH_PROTOTYPES = {
    "gs_morphometry_plan": (_I, [_I, _I, ctypes.c_longlong, ctypes.POINTER(ctypes.c_size_t)]),
    "gs_instance_morphometry": (_I, [_P, _P, _I, _I, _I, _P, ctypes.c_size_t, ctypes.c_longlong, _P, _P, _P, _P]),
}

SPLIT_PROTOTYPES = {
    "gs_edt_plan": (_I, [_I, _I, ctypes.POINTER(ctypes.c_size_t)]),
    "gs_label_peaks_plan": (_I, [_I, ctypes.POINTER(ctypes.c_size_t)]),
    "gs_split_plan": (_I, [_I, _I, _I, _I, ctypes.POINTER(ctypes.c_size_t)]),
    "gs_foreground_edt": (_I, [_P, _I, _I, _I, _P, ctypes.c_size_t, _P, _P]),
    "gs_label_peaks": (_I, [_P, _P, _I, _I, _I, _P, ctypes.c_size_t, _P, _P, _P]),
    "gs_split_cut": (_I, [_P, _P, _I, _P, _P, _I, _I, _I, _I, _P, ctypes.c_size_t, _P, _P, _P, _P, _P]),
}

WORKSPACE_PROTOTYPES = {
    "gs_espnet_workspace_classes": (_I, [_I] * 8 + [ctypes.POINTER(WorkspacePiece), _P, ctypes.c_size_t, ctypes.POINTER(_I)]),
    "gs_espnet_workspace_audit_host": (_I, [_I] * 7 + [_P, ctypes.c_size_t, ctypes.POINTER(WorkspaceReport)]),
    "gs_espnet_workspace_audit": (_I, [_P, _I, ctypes.POINTER(WorkspaceReport)]),
    "gs_espnet_workspace_poison": (_I, [_P, _I, ctypes.c_uint]),
}
GS_WS_FREE, GS_WS_INTERIOR, GS_WS_MUST_BE_ZERO = 0, 1, 2

# public header under include/ -> its table: every symbol the header declares, (restype, argtypes).  load() binds them in
# this order.
HEADERS = {
    "glomseg.h": PROTOTYPES,
    "glomseg_scoring.h": SCORING_PROTOTYPES,
    "glomseg_plan.h": PLAN_PROTOTYPES,
    "glomseg_instances.h": INSTANCE_PROTOTYPES,
    "glomseg_instance_match.h": MATCH_PROTOTYPES,
    "glomseg_boundary_dist.h": BOUNDARY_PROTOTYPES,
    "glomseg_lean.h": LEAN_PROTOTYPES,
    "glomseg_morphometry.h": MORPH_PROTOTYPES,
    "glomseg_split.h": SPLIT_PROTOTYPES,
    "glomseg_workspace.h": WORKSPACE_PROTOTYPES,
    "glomseg_forms.h": FORMS_PROTOTYPES,
    "glomseg_detector_steps.h": DETECTOR_STEPS_PROTOTYPES,
}
# the headers whose symbols an older library, loaded for an A/B (GLOMSEG_LIB), may lack; a symbol missing from any other is an
# AttributeError in load()
OPTIONAL_HEADERS = {"glomseg_plan.h", "glomseg_lean.h", "glomseg_workspace.h", "glomseg_forms.h", "glomseg_detector_steps.h"}

_lib = None


def load():
    """Load the library (once).  Import torch first in GPU processes so that libamdhip64.so.7 is
    torch's copy: device pointers and streams are then shared with torch."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise ImportError(
            "%s is missing: build it with `python -m glomeruli_segmentation_amd.build` "
            "(hipcc --offload-arch=gfx950).  There is no CPU fallback." % LIB_PATH)
    lib = ctypes.CDLL(LIB_PATH, mode=ctypes.RTLD_GLOBAL)
    for header, table in HEADERS.items():
        for name, (res, args) in table.items():
            if header in OPTIONAL_HEADERS and not hasattr(lib, name):
                continue   # (a library from before that header, loaded for an A/B: the callers of its entries then raise)
            fn = getattr(lib, name)   # AttributeError if the symbol is not exported
            fn.restype = res
            fn.argtypes = args
    if lib.gs_abi_version() != ABI_VERSION:
        raise ImportError("libglomseg.so ABI %d != binding ABI %d: rebuild" % (lib.gs_abi_version(), ABI_VERSION))
    if (lib.gs_build_flags() & GS_BUILD_DIAG) and os.environ.get("GLOMSEG_ALLOW_DIAG") != "1":
        raise ImportError("%s is a -DGS_DIAG experiment build (its timing variants return wrong results by construction); "
                          "set GLOMSEG_ALLOW_DIAG=1 to load it for an A/B measurement" % LIB_PATH)
    _lib = lib
    return lib


def check(status):
    if status != GS_OK:
        raise GlomsegError(status, load().gs_last_error().decode("utf-8", "replace"))


def fptr3(values):
    arr = (ctypes.c_float * len(values))(*[float(v) for v in values])
    return arr
