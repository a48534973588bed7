#!/usr/bin/env python3
"""The packed weight blob and the workspace size of the commit BEFORE the weight packer and the activation layout became host-only
headers (csrc/espnet_weights.h, csrc/workspace_plan.h), recorded from that commit's own code: tests/test_espnet_setup.py holds
the present code to these values, bit for bit.

The recorder checks PARENT out into a scratch directory, applies PATCH -- an export around the unmodified packing statements
of gs_espnet_create and the unmodified arithmetic of layout_workspace: the device checks, hipMalloc and the upload are skipped
when the export is active, nothing else changes --, builds that tree's library and asks it.  Nothing of the code under test
takes part.

    python tests/golden/make_golden_espnet_setup.py SCRATCH_DIR    ->  tests/golden/espnet_setup.json
"""
import ctypes
import hashlib
import json
import os
import subprocess
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.join(REPO, "tests"))

from glomeruli_segmentation_amd.engine import pack_state_dict  # noqa: E402
from test_espnet_setup import MODELS, SHAPES, WS_MODELS, state_dict  # noqa: E402  (the configurations the test asks for)

PARENT = "0f8c616"

PATCH = r"""--- a/glomeruli_segmentation_amd/csrc/espnet.hip
+++ b/glomeruli_segmentation_amd/csrc/espnet.hip
@@ -274,6 +274,7 @@
     return a;
 }
 
+static size_t *g_export_ws = nullptr;
 static gs_status layout_workspace(Model *m, int n, int H, int W)
 {
     if (m->ws && n <= m->ws_n && H == m->ws_h && W == m->ws_w)
@@ -327,6 +328,7 @@
     size_t total = 0;
     for (Act *a : all)
         total += round_up(a->bytes(n) + slack, 256);
+    if (g_export_ws) { *g_export_ws = total; return GS_OK; }
     void *ws = nullptr;
     if (hipMalloc(&ws, total) != hipSuccess) {
         set_error("workspace allocation of %zu bytes failed (n=%d, %dx%d)", total, n, H, W);
@@ -1120,6 +1122,7 @@
 }
 }  // namespace gs
 
+static std::vector<float> *g_export_blob = nullptr;
 extern "C" {
 
 gs_status gs_espnet_create(const float *blob, const gs_layer_desc *table, int n_layers, int classes, int p, int q,
@@ -1134,7 +1137,7 @@
         return GS_ERR_UNSUPPORTED;
     }
     int ndev = 0;
-    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev == 0) {
+    if (!g_export_blob && (hipGetDeviceCount(&ndev) != hipSuccess || ndev == 0)) {
         set_error("gs_espnet_create: no HIP device visible");
         return GS_ERR_NODEVICE;
     }
@@ -1145,10 +1148,12 @@
     m.p = p;
     m.q = q;
     m.encoder_only = encoder_only != 0;
+    hipDeviceProp_t prop{};
+    if (!g_export_blob) {
     GS_HIP(hipGetDevice(&m.device));
-    hipDeviceProp_t prop;
     GS_HIP(hipGetDeviceProperties(&prop, m.device));
-    if (std::strncmp(prop.gcnArchName, "gfx950", 6) != 0) {
+    }
+    if (!g_export_blob && std::strncmp(prop.gcnArchName, "gfx950", 6) != 0) {
         set_error("gs_espnet_create: device %d is %s; this library is built for gfx950 only", m.device, prop.gcnArchName);
         return GS_ERR_NODEVICE;
     }
@@ -1341,6 +1346,7 @@
         }
     }
     bb.reserve(512);   // tail guard: LDS-DMA staging reads whole 1-KiB pieces
+    if (g_export_blob) { *g_export_blob = bb.data; return GS_OK; }
     GS_HIP(hipMalloc(reinterpret_cast<void **>(&m.dblob), bb.data.size() * sizeof(float)));
     GS_HIP(hipMemcpy(m.dblob, bb.data.data(), bb.data.size() * sizeof(float), hipMemcpyHostToDevice));
     *out = h.release();
@@ -1701,4 +1707,31 @@
     return rc != GS_OK ? rc : gs_device_fault_check();   // (every batch has been drained: a few microseconds)
 }
 
+
+// ---- export of the parent's packing and workspace arithmetic (recording only)
+gs_status gs_export_pack(const float *blob, const gs_layer_desc *table, int n_layers, int classes, int p, int q, int encoder_only,
+                         float *out, size_t cap, size_t *n_floats)
+{
+    std::vector<float> v;
+    gs_espnet *h = nullptr;
+    g_export_blob = &v;
+    const gs_status st = gs_espnet_create(blob, table, n_layers, classes, p, q, encoder_only, &h);
+    g_export_blob = nullptr;
+    if (st != GS_OK) return st;
+    *n_floats = v.size();
+    if (out && cap >= v.size()) std::memcpy(out, v.data(), v.size() * sizeof(float));
+    return GS_OK;
+}
+gs_status gs_export_workspace(int n, int height, int width, int p, int classes, int encoder_only, size_t *bytes)
+{
+    gs_status st = check_shape(n, height, width);
+    if (st != GS_OK) return st;
+    Model m;
+    m.classes = classes, m.cp = padded_classes(classes), m.p = p, m.encoder_only = encoder_only != 0;
+    g_export_ws = bytes;
+    st = layout_workspace(&m, n, height, width);
+    g_export_ws = nullptr;
+    return st;
+}
+
 }  // extern "C"
"""


def main(scratch):
    tree = os.path.join(scratch, "parent")
    lib_path = os.path.join(tree, "glomeruli_segmentation_amd", "libglomseg.so")
    if not os.path.exists(lib_path):
        os.makedirs(tree)
        archive = subprocess.run(["git", "-C", REPO, "archive", PARENT], check=True, capture_output=True).stdout
        subprocess.run(["tar", "-x", "-C", tree], input=archive, check=True)
        subprocess.run(["patch", "-p1"], input=PATCH.encode(), cwd=tree, check=True)
        subprocess.check_call([sys.executable, "-m", "glomeruli_segmentation_amd.build"], cwd=tree)
    lib = ctypes.CDLL(lib_path)
    out = {"parent": PARENT, "weights": {}, "workspace": {}}
    for name, p, q, classes, enc in MODELS:
        blob, table = pack_state_dict(state_dict(name, p, q, classes, enc))
        n = ctypes.c_size_t()
        args = (blob.ctypes.data_as(ctypes.c_void_p), table, len(table), classes, p, q, int(enc))
        assert lib.gs_export_pack(*args, None, ctypes.c_size_t(0), ctypes.byref(n)) == 0, name
        packed = np.zeros(n.value, np.float32)
        assert lib.gs_export_pack(*args, packed.ctypes.data_as(ctypes.c_void_p), ctypes.c_size_t(packed.size), ctypes.byref(n)) == 0
        out["weights"][name] = {"floats": int(n.value), "sha256": hashlib.sha256(packed.tobytes()).hexdigest()}
    for name, classes, p, enc in WS_MODELS:
        for n, h, w in SHAPES:
            b = ctypes.c_size_t()
            assert lib.gs_export_workspace(n, h, w, p, classes, int(enc), ctypes.byref(b)) == 0, (name, n, h, w)
            out["workspace"]["%s/%dx%dx%d" % (name, n, h, w)] = int(b.value)
    # the parent's refusals of a shape (status codes of include/glomseg.h)
    b = ctypes.c_size_t()
    out["workspace_status"] = {"c5_p2/1x8192x8192": lib.gs_export_workspace(1, 8192, 8192, 2, 5, 0, ctypes.byref(b)),
                               "c5_p2/0x64x128": lib.gs_export_workspace(0, 64, 128, 2, 5, 0, ctypes.byref(b)),
                               "c5_p2/1x12x64": lib.gs_export_workspace(1, 12, 64, 2, 5, 0, ctypes.byref(b))}
    with open(os.path.join(HERE, "espnet_setup.json"), "w") as fh:
        json.dump(out, fh, indent=1, sort_keys=True)
        fh.write("\n")
    print(json.dumps(out, indent=1, sort_keys=True))


if __name__ == "__main__":
    main(sys.argv[1])
