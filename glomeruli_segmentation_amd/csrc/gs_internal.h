// Shared internals of libglomseg.so (not part of the ABI).
#pragma once
#include <hip/hip_runtime.h>

#include <cstdarg>
#include <cstdio>
#include <cstring>
#include <functional>
#include <string>

#include "../../include/glomseg.h"
#include "espnet_facts.h"   // set_error, round_up, Act: shared with the host-only set-up headers

namespace gs {

#define GS_HIP(expr)                                                                              \
    do {                                                                                          \
        hipError_t e_ = (expr);                                                                   \
        if (e_ != hipSuccess) {                                                                   \
            gs::set_error("%s failed: %s (%s:%d)", #expr, hipGetErrorString(e_), __FILE__, __LINE__); \
            return GS_ERR_HIP;                                                                    \
        }                                                                                         \
    } while (0)

#define GS_REQUIRE(cond, ...)                                                                     \
    do {                                                                                          \
        if (!(cond)) {                                                                            \
            gs::set_error(__VA_ARGS__);                                                           \
            return GS_ERR_INVALID;                                                                \
        }                                                                                         \
    } while (0)

// a device buffer that only ever grows (scratch kept across calls)
template <typename T>
inline gs_status grow(T *&buf, size_t &have, size_t need, const char *what)
{
    if (have >= need)
        return GS_OK;
    if (buf) {
        GS_HIP(hipDeviceSynchronize());   // work in flight may still use the old buffer
        GS_HIP(hipFree(buf));
        buf = nullptr, have = 0;
    }
    if (hipMalloc(reinterpret_cast<void **>(&buf), need) != hipSuccess) {
        (void)hipGetLastError();
        set_error("%s allocation of %zu bytes failed", what, need);
        return GS_ERR_NOMEM;
    }
    have = need;
    return GS_OK;
}

static inline int cdiv(int a, int b) { return (a + b - 1) / b; }
// p is not NULL and a multiple of a, a power of two
static inline bool aligned(const void *p, uintptr_t a) { return p && ((uintptr_t)p & (a - 1)) == 0; }

// NHWC convolution (csrc/detect_ops.hip); ho / wo are filled in by the launcher.
struct ConvNhwcArgs {
    const float *in, *w, *bias;
    float *out;
    int n, h, w_, cin, kh, kw, cout, stride, pad, relu, ho, wo;
};
void conv2d_nhwc_pack4(const float *w, int kh, int kw, int cin, int cout, float *dst);
// packed: a.w went through conv2d_nhwc_pack4 (handles that own their weights); a shape the packed-weight kernels cannot take
// is GS_ERR_UNSUPPORTED.  The kernel is conv_nhwc_form's choice (detect_plan.h); a caller that has planned already passes it.
struct ConvPlan;
gs_status launch_conv2d_nhwc(const ConvNhwcArgs &a, bool packed, hipStream_t stream);
gs_status launch_conv2d_nhwc(ConvNhwcArgs a, const ConvPlan &plan, bool packed, hipStream_t stream);

// ---- espnet.hip internals that the crop pipeline (crops.hip) builds on
struct CropPipe;                                   // staging state of gs_espnet_segment_crops*, owned by the handle
CropPipe *&espnet_crop_pipe(gs_espnet *h);
void crop_pipe_destroy(CropPipe *p);               // crops.hip; called by gs_espnet_destroy
int espnet_device(gs_espnet *h);
int espnet_is_full_net(gs_espnet *h);
int espnet_lanes(gs_espnet *h);
int espnet_classes(gs_espnet *h);

// The ensemble (BASELINE cfg 5, definition in DESIGN.md): prob [N][classes][H][W] accumulates ens_w * softmax(logits) over the
// member models in the decoder tail.  A member's role is what its tail does with the accumulator: FIRST stores, MIDDLE adds, LAST
// adds, then takes the argmax of the sum -> mask + counts (nothing is written back), SOLE is a single member (softmax -> argmax,
// prob untouched).  NONE: no ensemble, the argmax of the logits.  The kernels receive the value as an `int` (ens_mode).
enum class EnsRole : int { NONE = 0, FIRST = 1, MIDDLE = 2, LAST = 3, SOLE = 4 };
constexpr __host__ __device__ bool ens_reads(int mode) { return mode == 2 || mode == 3; }      // adds to what prob holds
constexpr __host__ __device__ bool ens_writes(int mode) { return mode == 1 || mode == 2; }     // leaves its sum in prob
constexpr __host__ __device__ bool ens_finishes(int mode) { return mode == 0 || mode >= 3; }   // zeroes hist in the stem, writes mask and counts
constexpr EnsRole ens_role(int k, int K) { return K == 1 ? EnsRole::SOLE : k == 0 ? EnsRole::FIRST : k == K - 1 ? EnsRole::LAST : EnsRole::MIDDLE; }   // member k of K

// One forward on one lane of a handle.  The defaults are a plain forward: fill in the input, the shape and the outputs wanted.
struct ForwardReq {
    const void *in = nullptr;
    int in_format = GS_IN_F32_NCHW, n = 0, H = 0, W = 0;
    const float *mean = nullptr, *stdv = nullptr;   // null: 0 / 1 (an input that is normalised already)
    float *logits = nullptr;                        // (ESPNet-C: the 1/8-scale ones)
    // [n][classes], zeroed by the stem, counted into by the last kernel.  ESPNet-C: `hist` without `mask` means "zero it in the
    // stem, run no head" -- an ensemble member's trunk, which stops with its 1/8-scale logits in the workspace (run_ensemble)
    uint8_t *mask = nullptr;
    unsigned long long *hist = nullptr;
    EnsRole role = EnsRole::NONE;
    float *prob = nullptr, ens_w = 1.0f;   // the ensemble's accumulator and this member's weight (roles other than NONE)
    hipStream_t s = nullptr;
};
// arguments are the caller's responsibility beyond the checks of gs_espnet_forward_lane
gs_status espnet_forward(gs_espnet *h, int lane, const ForwardReq &r);
// what a list of members is (all full networks / all ESPNet-C), or its refusal
gs_status ensemble_kind(gs_espnet *const *models, int n_models, bool *enc_only);
// The ensemble of a checked member list on lane `lane`.  `shared` is every member's request; the runner fills in mean / stdv (member
// k's: means + 3 * k, stds + 3 * k; null: none), the role, the weight 1 / K and the accumulator.  `prepare(k)`, when given, runs
// before member k's forward (the crop pipeline resamples its crops with that member's mean / std).
gs_status run_ensemble(gs_espnet *const *models, int n_models, int lane, const ForwardReq &shared, const float *means,
                       const float *stds, const std::function<gs_status(int)> &prepare = nullptr);

}  // namespace gs
