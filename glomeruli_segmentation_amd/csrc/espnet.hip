// gs_espnet_*: model handle, weight packing, HBM workspace and the forward schedule.
// Reference path replaced: module/espnet/test/Model.py ESPNet.forward (:341-378) /
// ESPNet_Encoder.forward (:273-304) called from module/espnet/test/VisualizeResults_iou.py:123.
#include <chrono>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <functional>
#include <map>
#include <memory>
#include <string>
#include <thread>
#include <type_traits>
#include <vector>

#include "../../include/glomseg_plan.h"
#include "../../include/glomseg_lean.h"
#include "../../include/glomseg_forms.h"
#include "../../include/glomseg_workspace.h"
#include "conv_mfma.h"
#include "dec_tail_args.h"
#include "enc_head.h"
#include "enc_head_ens.h"
#include "espnet_config.h"
#include "forward_plan.h"
#include "espnet_kernels.h"
#include "espnet_weights.h"
#include "host_copy.h"
#include "host_pipe.h"
#include "workspace_audit.h"
#include "workspace_plan.h"

namespace gs {

static thread_local std::string g_err;
void set_error(const char *fmt, ...)
{
    char buf[1024];
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(buf, sizeof buf, fmt, ap);
    va_end(ap);
    g_err = buf;
}

#ifdef GS_DIAG
static bool getenv_flag(const char *name)
{
    const char *e = std::getenv(name);
    return e && std::atoi(e) != 0;
}
static bool no_vec() { return getenv_flag("GS_NO_VEC"); }
#else
static constexpr bool no_vec() { return false; }
#endif

enum KernelId {
    K_STEM, K_POOL, K_L2_C1S, K_L2_DOWN, K_L2_C1, K_L2_ESP, K_CAT_B2, K_L3_C1S, K_L3_DOWN, K_L3_C1, K_L3_ESP,
    K_DEC1, K_DEC2, K_DEC3, K_DEC_CONV, K_DEC4, K_DEC_TAIL, K_ENC_HEAD, K_ENC_HEAD_ENS, K_COUNT
};
static const char *kKernelNames[K_COUNT] = {
    "stem_kernel", "pool_kernel", "conv_l2_reduce_s2", "conv_l2_down_branches", "conv_l2_reduce_1x1",
    "conv_l2_esp_branches", "cat_b2_kernel", "conv_l3_reduce_s2", "conv_l3_down_branches", "conv_l3_reduce_1x1",
    "conv_l3_esp_branches", "dec1_kernel", "dec2_kernel", "dec3_kernel", "conv_dec_cbr", "dec4_kernel", "dec_tail_kernel",
    "enc_head_kernel", "enc_head_ens_kernel"};

struct Model : Workspace {   // (the activations: workspace_plan.h)
    int classes = 0, p = 0, q = 0;
    int cp = 0;   // the padded class count the decoder kernels are instantiated for: 5 for the five-class networks (the fast path),
                  // else `classes` rounded up to a multiple of four (espnet_kernels.h, "CLASS COUNTS")
    bool encoder_only = false;
    int device = 0, num_cus = 256;
#ifdef GS_DIAG
    int variant = 0;   // GS_VARIANT env (diagnostic builds only): kernel A/B experiments (0 = shipped configuration)
#else
    static constexpr int variant = 0;
#endif
    float *dblob = nullptr;
    EspnetOffsets w;   // float offsets into dblob, and the stem's parameters: they travel as kernel arguments (espnet_weights.h)

    // workspace
    void *ws = nullptr;
    size_t ws_bytes = 0;
    int ws_n = 0, ws_h = 0, ws_w = 0;
    float *prob = nullptr;   // ensemble scratch of this lane (ensemble_scratch: the first member's handle owns it)
    size_t prob_bytes = 0;
    std::map<std::string, std::pair<Act, int>> stages;   // name -> (activation, channels) of the last forward
    // a ping-pong buffer that is written again no longer holds the stage recorded for it earlier
    void set_stage(const std::string &name, const Act &act, int C)
    {
        for (auto it = stages.begin(); it != stages.end();)
            it = it->second.first.base == act.base ? stages.erase(it) : std::next(it);
        stages[name] = {act, C};
    }
    int last_n = 0;
    bool b2_lazy = false;    // planes 64..127 of the stage "b2" are not materialised by the last forward (read_stage fills them)
    bool lean = false;       // the last forward was lean (ForwardPlan::lean): the stages such a request leaves out (read_stage's message)

    // profiling
    bool profile = false;
    struct Ev { hipEvent_t a, b; int k; };
    std::vector<Ev> events;
    double prof_ms[K_COUNT] = {0};
    long long prof_launches[K_COUNT] = {0};
    double prof_flops[K_COUNT] = {0};
};

// ------------------------------------------------------------------------------------------
static gs_status layout_workspace(Model *m, int n, int H, int W)
{
    if (m->ws && n <= m->ws_n && H == m->ws_h && W == m->ws_w)
        return GS_OK;
    if (m->ws) {
        GS_HIP(hipDeviceSynchronize());
        GS_HIP(hipFree(m->ws));
        m->ws = nullptr;
    }
    WorkspacePlan plan;   // every activation, its place in the allocation and the total: workspace_plan.h
    const gs_status st = plan_workspace(n, H, W, m->cp, m->p, m->encoder_only, plan);
    if (st != GS_OK)
        return st;
    void *ws = nullptr;
    if (hipMalloc(&ws, plan.bytes) != hipSuccess) {
        set_error("workspace allocation of %zu bytes failed (n=%d, %dx%d)", plan.bytes, n, H, W);
        return GS_ERR_NOMEM;
    }
    GS_HIP(hipMemset(ws, 0, plan.bytes));   // halos and padded channel planes are zero from here on
    // (the fill runs on the NULL stream, which non-blocking streams -- the host pipelines' own, torch's side streams -- do not
    // wait for: a forward launched on one of them right after this call must not meet the fill still in flight)
    GS_HIP(hipDeviceSynchronize());
    static_cast<Workspace &>(*m) = plan.acts;
    int i = 0;
    for (Act *a : acts_of(*m))
        a->base = reinterpret_cast<float *>(static_cast<char *>(ws) + plan.at[i++]);
    m->ws = ws;
    m->ws_bytes = plan.bytes;
    m->ws_n = n;
    m->ws_h = H;
    m->ws_w = W;
    return GS_OK;
}

// ------------------------------------------------------------------------------------------
struct Launcher {
    Model *m;
    hipStream_t s;
    gs_status st = GS_OK;
    int n;
    template <typename F>
    void run(int kid, double flops_per_tile, F &&f)
    {
        if (st != GS_OK)
            return;
        Model::Ev ev{nullptr, nullptr, kid};
        if (m->profile) {
            if (hipEventCreate(&ev.a) != hipSuccess || hipEventCreate(&ev.b) != hipSuccess ||
                hipEventRecord(ev.a, s) != hipSuccess) {
                set_error("profiling event setup failed");
                st = GS_ERR_HIP;
                return;
            }
        }
        st = f();
        if (st == GS_OK && hipGetLastError() != hipSuccess) {
            set_error("launch of %s failed", kKernelNames[kid]);
            st = GS_ERR_HIP;
        }
        if (m->profile && st == GS_OK) {
            hipEventRecord(ev.b, s);
            m->events.push_back(ev);
            m->prof_flops[kid] += flops_per_tile;   // summed like the times: launches of one kernel name may differ (fused / plain)
        }
    }
};

static ConvArgs conv_args(const Act &in, const float *wpack, const Act &out, const Act *res, int n)
{
    ConvArgs a{};
    a.in = in.base;
    a.in_sn = in.sn;
    a.in_sc = in.sc;
    a.in_pitch = in.pitch;
    a.in_off = in.off;
    a.in_img_bytes = (unsigned)(in.sn * sizeof(float));
    a.wpack = wpack;
    a.out = out.base;
    a.out_sn = out.sn;
    a.out_sc = out.sc;
    a.out_pitch = out.pitch;
    a.out_off = out.off;
    a.out_img_bytes = (unsigned)(out.sn * sizeof(float));
    if (res) {
        a.res = res->base;
        a.res_sn = res->sn;
        a.res_sc = res->sc;
        a.res_pitch = res->pitch;
        a.res_off = res->off;
        a.res_img_bytes = (unsigned)(res->sn * sizeof(float));
    }
    a.N = n;
    a.H = out.H;
    a.W = out.W;
    return a;
}

// The optional outputs of a conv launch, each added to the arguments conv_args made.
// F_DUAL: the second store, through its own BN + PReLU, into planes coff.. of a concat buffer
static ConvArgs with_dual(ConvArgs a, const Act &cat, int coff)
{
    a.out2 = cat.base;
    a.out2_sn = cat.sn;
    a.out2_sc = cat.sc;
    a.out2_pitch = cat.pitch;
    a.out2_off = cat.off;
    a.out2_coff = coff;
    a.out2_img_bytes = (unsigned)(cat.sn * sizeof(float));
    return a;
}
// F_FUSE1X1: the next block's reduced map is written by this block's epilogue (the two maps alternate)
static ConvArgs with_fused(ConvArgs a, const Act &r, int nout3)
{
    a.out3 = r.base;
    a.out3_sn = r.sn;
    a.out3_sc = r.sc;
    a.out3_pitch = r.pitch;
    a.out3_off = r.off;
    a.out3_img_bytes = (unsigned)(r.sn * sizeof(float));
    a.nout3 = nout3;
    return a;
}
// F_SIDE1X1: the stride-2 reduce also writes level3_C's raw output
static ConvArgs with_side(ConvArgs a, const Act &side)
{
    a.side = side.base;
    a.side_sn = side.sn;
    a.side_sc = side.sc;
    a.side_pitch = side.pitch;
    a.side_off = side.off;
    a.side_img_bytes = (unsigned)(side.sn * sizeof(float));
    return a;
}
// F_CLS1X1: the classifier's partial sums of one producer (0: output2_0, channels 0..127; 1: output2, 128..255; b3: its
// channel records) go to its two groups of class planes in tt, which nothing reads or writes before dec2 (cls_side_sums,
// espnet_facts.h).  `a` is a level-3 launch: a.H x a.W is the 1/8-scale map.
static ConvArgs with_cls(ConvArgs a, const float *b3, const Act &tt, int producer)
{
    a.crec = b3 + (long long)producer * 128 * CLS_REC;
    a.cls_sc = a.H * a.W;
    a.cls_pitch = a.W;
    a.cls = tt.base + (long long)producer * 2 * CLS_N * a.cls_sc;
    a.cls_sn = tt.sn;
    a.cls_img_bytes = (unsigned)((size_t)2 * CLS_N * a.cls_sc * sizeof(float));
    return a;
}

static inline unsigned blocks_for(long long items) { return (unsigned)((items + 255) / 256); }

// Timing / stamp variants of the forward (GS_VARIANT: ablations, per-wave stamps, the kernels a round replaced) live in
// espnet_diag.inc and exist in -DGS_DIAG builds only.  The forward offers them its launch sites through GS_DIAG_TRY; in the
// product build that macro expands to nothing (its arguments are not even evaluated), so what follows is the shipped
// schedule and nothing else.
#ifdef GS_DIAG
#include "espnet_diag.inc"
#define GS_DIAG_TRY(call)     \
    do {                      \
        gs_status dst_;       \
        if (call) return dst_; \
    } while (0)
#else
#define GS_DIAG_TRY(call) \
    do {                  \
    } while (0)
#define GS_DIAG_STAMPED(F, S, block)
#endif

// ------------------------------------------------------------------------------------------
// The switchboard: every conv_mfma_kernel instantiation the forward can run is spelled here once, as the Spec of its form in
// forward_plan.h's table.  The forward (encode / decode) and the single-block hook (gs_espnet_block_forward) launch through
// launch_planned and decide nothing themselves; the caller has put a form's optional outputs into `ca` (with_dual .. with_cls).
static gs_status not_planned(const char *launch_class)
{
    set_error("internal: the forward plan has no form for launch class %s", launch_class);
    return GS_ERR_INVALID;
}

// A form's instantiation: its base mask (F_VEC and F_SKIP_PAD are the form's), the modifier bits a launch may OR onto it (MAY:
// the side sums the plan asks for -- F_SIDE1X1, F_CLS1X1, F_CLS_ONLY) and its CFG_* tuple.  A modifier outside MAY is a pair the
// plan never makes: launch_form refuses it and it is never instantiated.
template <int FLAGS, int MAY, int... C>
struct Inst {
    static constexpr int flags = FLAGS, pixels = cfg_pixels(C...);
    static constexpr bool odd_2b_legal = false;
    static constexpr bool carries(int extra) { return !(extra & ~MAY); }
    template <int EXTRA>
    static gs_status launch(const ConvArgs &ca, int num_cus, hipStream_t s) { return launch_conv_mfma<C..., FLAGS | EXTRA>(ca, num_cus, s); }
};
struct NotConv {   // a row that is no conv launch: a plain kernel, or a decoder shape at a class count of the other MFMA shape
    static constexpr int flags = 0;
    static constexpr bool odd_2b_legal = false;
    static constexpr bool carries(int) { return false; }
};
// A level-3 branch form with its pixel groups in pairs and a tap row per chunk: 25 real input channels of CINP = 26, so it may carry
// F_ODD_2B, and does unless the build says CFG_L3_ODD_2B = 0
template <int FLAGS, int MAY, int... C>
struct OddInst : Inst<FLAGS | ODD_L3, MAY, C...> {
    static_assert(cfg_odd_2b_legal(C...), "F_ODD_2B on a form that cannot pair its pixel groups");
    static constexpr bool odd_2b_legal = true;
};
// Spec<class, form, CLS>: one per row of the table (a row without one does not compile); CLS is the decoder's padded class count
template <typename E, E F, int CLS>
struct Spec;
#define GS_SPEC(id, ...) \
    template <int CLS>   \
    struct Spec<decltype(form::id), form::id, CLS> : __VA_ARGS__ {};

// the level-2 branch kernels.  The down-sampler stores the raw output only, with or without ESP blocks behind it: b2 is applied
// by the consumers (p > 0: the level-3 stride-2 reduce and dec2 on load; p == 0: cat_b2_kernel)
constexpr int L2_DOWN = F_BNACT | (POL_L2_DOWN & F_ST_NT), L2_ESP = F_BNACT | F_RES | POL_L2_ESP;
constexpr int L2_LAST = F_BNACT | F_RES | F_NOSTORE | F_DUAL | POL_L2_LAST;
GS_SPEC(l2_down::P2S_VEC, Inst<L2_DOWN | FUSE_L2 | F_VEC, 0, CFG_L2_BR_P2S>)
GS_SPEC(l2_down::P4S_VEC_SKIP, Inst<L2_DOWN | FUSE_L2 | F_VEC | F_SKIP_PAD, 0, CFG_L2_BR_P4S>)
GS_SPEC(l2_down::P4_VEC, Inst<L2_DOWN | FUSE_L2 | F_VEC, 0, CFG_L2_BR_P4>)
GS_SPEC(l2_down::P4, Inst<L2_DOWN | FUSE_L2, 0, CFG_L2_BR_P4>)
GS_SPEC(l2_down::UNFUSED_P4_VEC, Inst<L2_DOWN | F_VEC, 0, CFG_L2_BR_P4>)
GS_SPEC(l2_down::UNFUSED_P4, Inst<L2_DOWN, 0, CFG_L2_BR_P4>)
GS_SPEC(l2_esp_fused::P2S_VEC, Inst<L2_ESP | FUSE_L2 | F_VEC, 0, CFG_L2_BR_P2S>)
GS_SPEC(l2_esp_fused::P4_VEC, Inst<L2_ESP | FUSE_L2 | F_VEC, 0, CFG_L2_BR_P4>)
GS_SPEC(l2_esp_fused::P4, Inst<L2_ESP | FUSE_L2, 0, CFG_L2_BR_P4>)
GS_SPEC(l2_esp_fused::UNFUSED_P4_VEC, Inst<L2_ESP | F_VEC, 0, CFG_L2_BR_P4>)
GS_SPEC(l2_esp_fused::UNFUSED_P4, Inst<L2_ESP, 0, CFG_L2_BR_P4>)
GS_SPEC(l2_esp_last::P2S_VEC, Inst<L2_LAST | F_VEC, 0, CFG_L2_BR_P2S>)
GS_SPEC(l2_esp_last::P4_VEC, Inst<L2_LAST | F_VEC, 0, CFG_L2_BR_P4>)
GS_SPEC(l2_esp_last::P4, Inst<L2_LAST, 0, CFG_L2_BR_P4>)
GS_SPEC(cat_b2::KERNEL, NotConv)
// the level-3 stride-2 reduce (the F_BNLOAD forms: planes 64..127 of output1_cat hold output1_0 RAW, b2 is applied to the B
// operands on load); every form can also compute the five-class level3_C (F_SIDE1X1)
constexpr int L3_REDUCE = F_S2PAIR | POL_L3_C1S | S2FLIP_L3;
GS_SPEC(l3_reduce::BNL_P1, Inst<L3_REDUCE | F_BNLOAD, F_SIDE1X1(5), CFG_L3_C1S_BNL_P1>)
GS_SPEC(l3_reduce::BNL, Inst<L3_REDUCE | F_BNLOAD, F_SIDE1X1(5), CFG_L3_C1S_BNL>)
GS_SPEC(l3_reduce::C1S, Inst<L3_REDUCE, F_SIDE1X1(5), CFG_L3_C1S>)
// the level-3 branch kernels.  The classifier's side sums (F_CLS1X1) go with every form the plan pairs them with: not the unfused
// forms (cls_side_sums) or the down-sampler's four-pixel one (plan_forward); only the network's last block may drop its map (F_CLS_ONLY)
constexpr int L3_DOWN = F_BNACT | POL_L3_DOWN | FUSE_L3, L3_ESP = F_BNACT | F_RES | POL_L3_ESP;
constexpr int AGL_SMALL = CFG_SMALL_AGL ? F_A_GLOBAL : 0;
GS_SPEC(l3_down::P1R, Inst<L3_DOWN | SKIP_L3 | AGL_SMALL, F_CLS1X1, CFG_L3_BR_P1R>)
GS_SPEC(l3_down::P2R_VEC, OddInst<L3_DOWN | F_VEC | SKIP_L3, F_CLS1X1, CFG_L3_BR_P2R>)
GS_SPEC(l3_down::BR_VEC, Inst<L3_DOWN | F_VEC, 0, CFG_L3_BR>)
GS_SPEC(l3_down::P2F, Inst<L3_DOWN, F_CLS1X1, CFG_L3_BR_P2F>)
GS_SPEC(l3_down::UNFUSED_BR_VEC, Inst<F_BNACT | POL_L3_DOWN | F_VEC, 0, CFG_L3_BR>)
GS_SPEC(l3_down::UNFUSED_BR, Inst<F_BNACT | POL_L3_DOWN, 0, CFG_L3_BR>)
GS_SPEC(l3_esp_fused::P1R, Inst<L3_ESP | FUSE_L3 | SKIP_L3 | AGL_SMALL, 0, CFG_L3_BR_P1R>)
GS_SPEC(l3_esp_fused::P2R_VEC, OddInst<L3_ESP | FUSE_L3 | F_VEC | SKIP_L3, 0, CFG_L3_BR_P2R>)
GS_SPEC(l3_esp_fused::P2F, Inst<F_BNACT | F_RES | FUSE_L3, 0, CFG_L3_BR_P2F>)
GS_SPEC(l3_esp_last::P1R, Inst<L3_ESP | SKIP_L3 | AGL_SMALL, F_CLS1X1 | F_CLS_ONLY, CFG_L3_BR_P1R>)
GS_SPEC(l3_esp_last::P2R_VEC, OddInst<L3_ESP | F_VEC | SKIP_L3, F_CLS1X1 | F_CLS_ONLY, CFG_L3_BR_P2R>)   // tap rows in the halo skipped
GS_SPEC(l3_esp_last::BR_VEC, Inst<L3_ESP | F_VEC, F_CLS1X1 | F_CLS_ONLY, CFG_L3_BR>)
GS_SPEC(l3_esp_last::P2, OddInst<F_BNACT | F_RES, F_CLS1X1 | F_CLS_ONLY, CFG_L3_BR_P2>)
// The decoder's 3x3 convolutions as plain conv_mfma launches (MFMA rows = the padded output channels, BN + PReLU in the
// epilogue).  The shape is a property of the class count: the plan names it from the same CLS = Model::cp (dec_mt), and a form
// of the other shape is no launch at this CLS.
// (Deeper operand rings and four pixels per lane were measured on the conv launch: no gain -- at twenty classes it is at 90 % of
// what its padded matrix work allows, 20 of 32 rows.)
template <int CLS, int MT, int FLAGS, int CINP>
using DecInst = std::conditional_t<dec_mt(CLS) == MT, Inst<FLAGS, 0, MT, 8, CINP, 9, 1, 1, CLS, CLS, dec_pixels(CLS), 3>, NotConv>;
constexpr int dec_conv_cinp(int cls) { return (19 + cls + 3) / 4 * 4; }
GS_SPEC(dec3::KERNEL, NotConv)
GS_SPEC(dec3::MT16, DecInst<CLS, 16, F_BNACT, 2 * CLS>)
GS_SPEC(dec3::MT16_VEC, DecInst<CLS, 16, F_BNACT | F_VEC, 2 * CLS>)
GS_SPEC(dec3::MT32, DecInst<CLS, 32, F_BNACT, 2 * CLS>)
GS_SPEC(dec3::MT32_VEC, DecInst<CLS, 32, F_BNACT | F_VEC, 2 * CLS>)
GS_SPEC(dec_conv::TAIL, NotConv)
GS_SPEC(dec_conv::MT16, DecInst<CLS, 16, F_BNACT | POL_DEC_CONV, dec_conv_cinp(CLS)>)
GS_SPEC(dec_conv::MT16_VEC, DecInst<CLS, 16, F_BNACT | POL_DEC_CONV | F_VEC, dec_conv_cinp(CLS)>)
GS_SPEC(dec_conv::MT32, DecInst<CLS, 32, F_BNACT | POL_DEC_CONV, dec_conv_cinp(CLS)>)
GS_SPEC(dec_conv::MT32_VEC, DecInst<CLS, 32, F_BNACT | POL_DEC_CONV | F_VEC, dec_conv_cinp(CLS)>)
#undef GS_SPEC

// One form's launch: its spec with EXTRA on top (`what`: the launch class, for the refusal; `block`: the ESP block's index, which a
// stamp variant of -DGS_DIAG builds asks for).  The table's vector width is the spec's: vec_fits trusts the one, the kernel runs the other.
template <auto F, int EXTRA, int CLS>
static gs_status launch_form(const Model *m, const ConvArgs &ca, hipStream_t s, int block, const char *what)
{
    using S = Spec<decltype(F), F, CLS>;
    if constexpr (!S::carries(EXTRA)) {
        return not_planned(what);
    } else {
        static_assert((S::flags & F_VEC) ? pixels_per_lane(F) == S::pixels : pixels_per_lane(F) == 0,
                      "forward_plan.h's pixels per lane of a form is not the vector width of its Spec");
        if constexpr (EXTRA == 0) {   // (the side sums refuse every F_X_* flag)
            GS_DIAG_STAMPED(F, S, block)
        }
        return S::template launch<EXTRA>(ca, m->num_cus, s);
    }
}
// launch_planned<EXTRA, CLS>(m, form, ca, s): the one switch of each launch class, a `case` per row of its table
#define GS_FORM_CASE(id, name, ppl) \
    case F::id: return launch_form<F::id, EXTRA, CLS>(m, ca, s, block, what);
#define GS_CLASS_SWITCH(cls, FORMS)                                                                                                \
    template <int EXTRA = 0, int CLS = 0>                                                                                          \
    static gs_status launch_planned(const Model *m, form::cls f, const ConvArgs &ca, hipStream_t s, int block = -1, const char *what = #cls) \
    {                                                                                                                              \
        using F = form::cls;                                                                                                       \
        switch (f) {                                                                                                               \
            FORMS(GS_FORM_CASE)                                                                                                    \
        case F::none: break;                                                                                                       \
        }                                                                                                                          \
        return not_planned(what);                                                                                                  \
    }
GS_LAUNCH_CLASSES(GS_CLASS_SWITCH)
#undef GS_FORM_CASE
#undef GS_CLASS_SWITCH

// the launches that have one form: the level-2 stride-2 reduce and the 1x1 reduces that no epilogue computed
static gs_status launch_l2_reduce(const Model *m, const ConvArgs &ca, hipStream_t s) { return launch_conv_mfma<CFG_L2_C1S, F_S2PAIR | POL_L2_C1S | S2FLIP_L2>(ca, m->num_cus, s); }
static gs_status launch_l2_c1(const Model *m, const ConvArgs &ca, hipStream_t s) { return launch_conv_mfma<CFG_L2_C1, POL_L2_C1>(ca, m->num_cus, s); }   // 1x1: the run mapping measured no slower
static gs_status launch_l3_c1(const Model *m, const ConvArgs &ca, hipStream_t s) { return launch_conv_mfma<CFG_L3_C1, POL_L3_C1>(ca, m->num_cus, s); }

// ... and those whose modifier is the plan's: EXTRA is picked here, once.
// side5: the plan's l3c_in_reduce -- the five-class level3_C goes to ca.side (with_side)
static gs_status launch_l3_reduce(const Model *m, form::l3_reduce f, bool side5, const ConvArgs &ca, hipStream_t s)
{
    return side5 ? launch_planned<F_SIDE1X1(5)>(m, f, ca, s) : launch_planned(m, f, ca, s);
}
// cls5: the plan's cls_in_l3 -- the five-class classifier's channels 0..127 are summed into ca.cls (with_cls)
static gs_status launch_l3_down(const Model *m, form::l3_down f, bool cls5, const ConvArgs &ca, hipStream_t s)
{
    return cls5 ? launch_planned<F_CLS1X1>(m, f, ca, s, -1, "l3_down with the classifier's side sums") : launch_planned(m, f, ca, s);
}
// cls5: as launch_l3_down's, for the network's last block: channels 128..255.  cls_only: the plan's `lean` -- nothing of this forward
// reads that block's map, so it runs without its primary store; a block without the sums has nothing but its map and keeps it
static gs_status launch_l3_esp_last(const Model *m, form::l3_esp_last f, bool cls5, bool cls_only, const ConvArgs &ca, hipStream_t s)
{
    if (!cls5)
        return launch_planned(m, f, ca, s);
    return cls_only ? launch_planned<F_CLS1X1 | F_CLS_ONLY>(m, f, ca, s) : launch_planned<F_CLS1X1>(m, f, ca, s);
}

// The forward is the encoder (stem .. the last level-3 block), the same code for every class count, then the decoder instantiated
// for the padded class count (forward_any).  What the decoder needs of the encoder's run: cc[last] holds the last block's output
struct Encoded { int last; bool lazy_b2; };
static Encoded encode(Model *m, Launcher &L, const ForwardPlan &plan, const ForwardReq &r)
{
    const float *wb = m->dblob;
    const hipStream_t s = r.s;
    const int n = r.n, H = r.H, W = r.W, H1 = H / 2, W1 = W / 2, H2 = H / 4, W2 = W / 4, H3 = H / 8, W3 = W / 8;
    const double px1 = (double)H1 * W1, px2 = (double)H2 * W2, px3 = (double)H3 * W3;
    m->stages.clear();
    m->last_n = n;
    m->lean = plan.lean;
    // ---- stem (Model.py:346-350)
    L.run(K_STEM, px1 * (27 * 16 * 2), [&] {
        StemArgs a{};
        a.in = r.in;
        for (int i = 0; i < 3; ++i) {
            a.mean[i] = r.mean ? r.mean[i] : 0.0f;
            a.std[i] = r.stdv ? r.stdv[i] : 1.0f;
        }
        std::memcpy(a.w1, m->w.stem_params, sizeof(float) * 432);
        std::memcpy(a.bn1, m->w.stem_params + 432, sizeof(float) * 48);
        std::memcpy(a.b1, m->w.stem_params + 480, sizeof(float) * 57);
        a.a0 = view(m->a0);
        a.inp1 = view(m->inp1);
        a.N = n;
        a.H = H;
        a.W = W;
        if (r.hist && ens_finishes((int)r.role)) {   // zeroed by the first kernel of the forward; the last one adds into it
            a.hist_zero = r.hist;
            a.hist_count = n * m->classes;
        }
        hipLaunchKernelGGL(r.in_format == GS_IN_U8_BGR_NHWC ? stem_kernel<true> : stem_kernel<false>,
                           dim3(blocks_for((long long)n * H1 * ((W1 + STEM_PX - 1) / STEM_PX))), dim3(256), 0, s, a);
        return GS_OK;
    });
    L.run(K_POOL, 0, [&] {
        hipLaunchKernelGGL(pool_kernel, dim3(blocks_for((long long)n * 3 * H2 * (W2 / POOL_PX))), dim3(256), 0, s, view(m->inp1),
                           view(m->inp2), n, 3, m->p > 0 ? wb + m->w.b2 : nullptr, view(m->a1), 128, 131);
        return GS_OK;
    });
    m->set_stage("b1", m->a0, 19);
    m->set_stage("sample2", m->inp2, 3);

    // ---- level 2 (Model.py:351-357): DownSamplerB(19,64) then p ESP blocks
    L.run(K_L2_C1S, px2 * (19 * 9 * 12 * 2), [&] {
        GS_DIAG_TRY(diag_reduce_s2(m, 2, conv_args(m->a0, wb + m->w.l2_0.c1, m->r2[0], nullptr, n), s, dst_));
        return launch_l2_reduce(m, conv_args(m->a0, wb + m->w.l2_0.c1, m->r2[0], nullptr, n), s);
    });
    // b2 = BR(131) over cat([output1, output1_0, inp2]) (Model.py:359) never runs as a kernel: the last ESP block stores
    // only its b2-normalised form (planes 0..63 of output1_cat), the pool kernel writes planes 128..130 normalised, and
    // output1_0 is stored RAW into planes 64..127 (lazy b2, espnet_config.h: the consumers normalise on load).  With p == 0
    // the unfused cat kernel runs.
    const bool lazy_b2 = plan.lazy_b2;
    m->b2_lazy = lazy_b2;
    int rd2 = 0;   // index of the reduced map the next level-2 branch kernel reads
    L.run(K_L2_DOWN, px2 * (12 * 9 * 64 * 2) + (m->w.l2_0.fused_next ? px2 * (64 * 12 * 2) : 0), [&] {
        const ConvArgs ca = conv_args(m->r2[rd2], wb + m->w.l2_0.br, m->bb[0], nullptr, n);
        return launch_planned(m, plan.l2_down, m->w.l2_0.fused_next ? with_fused(ca, m->r2[rd2 ^ 1], 12) : ca, s);
    });
    bool have_r2 = m->w.l2_0.fused_next;   // the reduced map of the next block already exists
    rd2 ^= have_r2 ? 1 : 0;
    m->set_stage("level2_0", m->bb[0], 64);
    int cur2 = 0;
    for (int i = 0; i < m->p; ++i) {
        const int nxt = cur2 == 1 ? 2 : 1;
        const bool last = i == m->p - 1;
        const bool fuse_next = m->w.l2[i].fused_next;
        if (!have_r2)
            L.run(K_L2_C1, px2 * (64 * 12 * 2), [&] {
                return launch_l2_c1(m, conv_args(m->bb[cur2], wb + m->w.l2[i].c1, m->r2[rd2], nullptr, n), s);
            });
        L.run(K_L2_ESP, px2 * (12 * 9 * 64 * 2) + (fuse_next ? px2 * (64 * 12 * 2) : 0), [&] {
            const ConvArgs ca = conv_args(m->r2[rd2], wb + m->w.l2[i].br, m->bb[nxt], &m->bb[cur2], n);
            if (last)
                return launch_planned(m, plan.l2_esp_last, with_dual(ca, m->a1, 0), s);
            return launch_planned(m, plan.l2_esp_fused, fuse_next ? with_fused(ca, m->r2[rd2 ^ 1], 12) : ca, s);
        });
        have_r2 = fuse_next;
        rd2 ^= have_r2 ? 1 : 0;
        cur2 = nxt;
        if (!last)
            m->set_stage("level2." + std::to_string(i), m->bb[cur2], 64);
    }
    if (plan.cat_b2 == form::cat_b2::KERNEL) {
        L.run(K_CAT_B2, 0, [&] {
            hipLaunchKernelGGL(cat_b2_kernel, dim3(blocks_for((long long)n * 131 * H2 * W2)), dim3(256), 0, s, view(m->bb[cur2]),
                               view(m->bb[0]), view(m->inp2), wb + m->w.b2, view(m->a1), n);
            return GS_OK;
        });
    }
    m->set_stage("b2", m->a1, 131);

    // ---- level 3 (Model.py:361-366)
    int rd3 = 0;
    L.run(K_L3_C1S, px3 * (131 * 9 * 25 * 2) + (plan.l3c_in_reduce ? px2 * (131 * m->classes * 2) : 0), [&] {
        GS_DIAG_TRY(diag_reduce_s2(m, 3, conv_args(m->a1, wb + m->w.l3_0.c1, m->r3[0], nullptr, n), s, dst_));
        ConvArgs ca = conv_args(m->a1, wb + m->w.l3_0.c1, m->r3[0], nullptr, n);
        if (lazy_b2) {   // planes 64..127 of output1_cat hold output1_0 RAW: b2 is applied to the B operands on load
            ca.bnl_s0 = 64 / 2;      // k-groups of two channels
            ca.bnl_s1 = 128 / 2;
        }
        return launch_l3_reduce(m, plan.l3_reduce, plan.l3c_in_reduce, plan.l3c_in_reduce ? with_side(ca, m->l3c) : ca, s);
    });
    if (plan.l3c_in_reduce)
        m->set_stage("level3_C", m->l3c, m->classes);
    const double cls_flops = plan.cls_in_l3 ? px3 * (128 * m->classes * 2) : 0;   // a producer's half of the classifier (F_CLS1X1)
    L.run(K_L3_DOWN, px3 * (25 * 9 * 128 * 2) + (m->w.l3_0.fused_next ? px3 * (128 * 25 * 2) : 0) + cls_flops, [&] {
        ConvArgs ca = conv_args(m->r3[rd3], wb + m->w.l3_0.br, m->cc[0], nullptr, n);
        if (plan.cls_in_l3) {
            if ((long long)CLS_PART_PLANES * H3 * W3 > m->tt.sn) {
                set_error("internal: the classifier's partial planes do not fit the workspace's tt");
                return GS_ERR_INVALID;
            }
            ca = with_cls(ca, wb + m->w.b3, m->tt, 0);
        }
        return launch_l3_down(m, plan.l3_down, plan.cls_in_l3, m->w.l3_0.fused_next ? with_fused(ca, m->r3[rd3 ^ 1], 25) : ca, s);
    });
    bool have_r3 = m->w.l3_0.fused_next;
    m->set_stage("level3_reduce", m->r3[rd3], 25);      // (debug: valid until the second ESP block overwrites the map)
    rd3 ^= have_r3 ? 1 : 0;
    m->set_stage("level3_0", m->cc[0], 128);
    int cur3 = 0;
    for (int i = 0; i < m->q; ++i) {
        const int nxt = cur3 == 1 ? 2 : 1;
        const bool fuse_next = m->w.l3[i].fused_next;
        if (!have_r3)
            L.run(K_L3_C1, px3 * (128 * 25 * 2), [&] {
                return launch_l3_c1(m, conv_args(m->cc[cur3], wb + m->w.l3[i].c1, m->r3[rd3], nullptr, n), s);
            });
        L.run(K_L3_ESP, px3 * (25 * 9 * 128 * 2) + (fuse_next ? px3 * (128 * 25 * 2) : 0) + (i == m->q - 1 ? cls_flops : 0), [&] {
            const ConvArgs ca = conv_args(m->r3[rd3], wb + m->w.l3[i].br, m->cc[nxt], &m->cc[cur3], n);
            GS_DIAG_TRY(diag_l3_esp(m, ca, i, s, dst_));
            if (fuse_next)
                return launch_planned(m, plan.l3_esp_fused, with_fused(ca, m->r3[rd3 ^ 1], 25), s, i);
            const bool cls5 = plan.cls_in_l3 && i == m->q - 1;   // the network's last block holds output2
            return launch_l3_esp_last(m, plan.l3_esp_last, cls5, plan.lean, cls5 ? with_cls(ca, wb + m->w.b3, m->tt, 1) : ca, s);
        });
        have_r3 = fuse_next;
        rd3 ^= have_r3 ? 1 : 0;
        cur3 = nxt;
        m->set_stage("level3." + std::to_string(i), m->cc[cur3], 128);
        // a lean forward's last block stores no map (F_CLS_ONLY): its buffer holds no stage this forward vouches for -- not
        // output2, and no longer the block before the last one's input either, which the line above has just dropped
        if (plan.lean && i == m->q - 1)
            m->stages.erase("level3." + std::to_string(i));
    }
    return {cur3, lazy_b2};
}

// dec1_kernel .. the class map and the counts (ESPNet-C: dec1_kernel, then the head when a mask is asked for)
template <int CLS>
static gs_status decode(Model *m, Launcher &L, const ForwardPlan &plan, const ForwardReq &r, const Encoded &enc)
{
    const float *wb = m->dblob;
    const hipStream_t s = r.s;
    const int n = r.n, H = r.H, W = r.W, H1 = H / 2, W1 = W / 2, H2 = H / 4, W2 = W / 4, H3 = H / 8, W3 = W / 8;
    const double px1 = (double)H1 * W1, px2 = (double)H2 * W2, px3 = (double)H3 * W3;
    // ---- b3 + classifier (+ br + up_l3)  (Model.py:368-370)
    const int ncls = m->classes;   // real class count (CLS is the padded one): algorithmic FLOPs, output widths
    // ESPNet-C: the 1/8-scale logits are an output of their own and the input of the head; a caller that wants the class map
    // only gets them in the (otherwise unused) up_l3 buffer of the workspace, which is larger than [n][classes][H3][W3]
    float *enc_logits = !m->encoder_only ? nullptr : r.logits ? r.logits : m->o2c.base;
    L.run(K_DEC1, (plan.cls_in_l3 ? 0 : px3 * (256 * ncls * 2)) + px3 * (ncls * ncls * 4 * 2), [&] {
        if constexpr (CLS == CLS_N) {
            if (plan.cls_in_l3) {   // the classifier came out of the level-3 epilogues: add the partial planes, then br + up_l3
                Dec1SumsArgs a{};
                a.part = m->tt.base;
                a.psn = m->tt.sn;
                a.psc = H3 * W3;
                a.br = wb + m->w.br;
                a.wup = wb + m->w.wup3;
                a.out = view(m->o2c);
                a.N = n;
                a.H3 = H3;
                a.W3 = W3;
                a.classes = ncls;
                hipLaunchKernelGGL(dec1_sums_kernel<CLS>, dim3(blocks_for((long long)n * H3 * W3)), dim3(256), 0, s, a);
                return GS_OK;
            }
        }
        Dec1Args a{};
        a.c0 = view(m->cc[0]);
        a.clast = view(m->cc[enc.last]);
        a.b3w = wb + m->w.b3;
        a.br = m->encoder_only ? nullptr : wb + m->w.br;
        a.wup = m->encoder_only ? nullptr : wb + m->w.wup3;
        a.out = view(m->o2c);
        a.enc_logits = enc_logits;
        a.N = n;
        a.classes = ncls;
        // (channel batch: 16 channels x (3 + CLS) scalar constants in flight fit the scalar registers for five classes only)
        constexpr int CB = CLS <= 5 ? 16 : CLS <= 8 ? 8 : 4;
        hipLaunchKernelGGL((dec1_kernel<CLS, CB>), dim3((unsigned)(((long long)n * H3 * W3 + 63) / 64)), dim3(256), 0, s, a);
        return GS_OK;
    });
    if (m->encoder_only) {
        // ---- x8 bilinear upsampling + argmax + counts (VisualizeResults_iou.py:125-128,151-155,258-261), enc_head.h
        if (r.mask)
            L.run(K_ENC_HEAD, (double)H * W * (ncls * 6), [&] {
                EncHeadArgs a{};
                a.logits = enc_logits;
                a.mask = r.mask;
                a.hist = r.hist;
                a.classes = ncls;
                a.H3 = H3;
                a.W3 = W3;
                launch_enc_head(a, n, s);
                return GS_OK;
            });
        return L.st;
    }
    m->set_stage("up_l3", m->o2c, ncls);

    // ---- level3_C + cat + BR (Model.py:372-373)
    // Five classes: level3_C came out of the stride-2 reduce and dec3_cat_kernel applies the cat's BR to both raw halves on load, so
    // the forward itself needs no dec2 launch: there dec2_br_kernel only materialises the 2 * CLS normalised planes as the stage
    // "combine_t", and a lean forward (the plan: no logits asked for) does not run it and has no such stage.
    if constexpr (l3c_side_sums(CLS)) {
        if (!plan.l3c_in_reduce) {
            set_error("internal: a %d-class decoder without level3_C from the stride-2 reduce", CLS);
            return GS_ERR_INVALID;
        }
    }
    const bool cat_on_load = l3c_side_sums(CLS);
    if (!plan.lean) {
        L.run(K_DEC2, cat_on_load ? 0 : px2 * (131 * ncls * 2), [&] {
            Dec2Args a{};
            a.o2c = view(m->o2c);
            a.br = wb + m->w.cbr0;
            a.t = view(m->tt);
            a.N = n;
            a.classes = ncls;
            if constexpr (l3c_side_sums(CLS)) {
                a.a1 = view(m->l3c);
                hipLaunchKernelGGL(dec2_br_kernel<CLS>, dim3(blocks_for((long long)n * H2 * W2)), dim3(256), 0, s, a);
            } else {
                a.a1 = view(m->a1);
                a.raw = view(m->bb[0]);
                a.b2 = wb + m->w.b2;
                a.raw_c0 = 64;
                a.raw_cn = enc.lazy_b2 ? 64 : 0;
                a.w3c = wb + m->w.w3c;
                hipLaunchKernelGGL(dec2_kernel<CLS>, dim3((unsigned)(((long long)n * H2 * W2 + 63) / 64)), dim3(256), 0, s, a);   // 64 pixels x 4 channel quarters
            }
            return GS_OK;
        });
        if (ncls == CLS)   // (with padding planes in between the two halves are not one contiguous stage)
            m->set_stage("combine_t", m->tt, 2 * CLS);
    }
    // ---- CBR(2c,c,3) + up_l2 (Model.py:373)
    if constexpr (dec3_on_mfma(CLS)) {
        // many classes: the 3x3 over 2 * CLS planes is 7 200 FMAs per pixel at twenty classes -- on the matrix cores (a plain
        // conv_mfma launch, BN + PReLU in its epilogue), the deconvolution + BR as a second, small kernel
        L.run(K_DEC3, px2 * (2 * ncls * 9 * ncls * 2), [&] {
            return launch_planned<0, CLS>(m, plan.dec3, conv_args(m->tt, wb + m->w.wcc_mfma, m->t3, nullptr, n), s);
        });
        L.run(K_DEC3, px2 * (ncls * ncls * 4 * 2), [&] {
            Dec3Args a{};
            a.t = view(m->t3);
            a.wup = wb + m->w.wup2;
            a.bnu = wb + m->w.bnu2;
            a.e = view(m->ee);
            a.N = n;
            a.classes = ncls;
            hipLaunchKernelGGL(dec3b_kernel<CLS>, dim3(blocks_for((long long)n * H2 * W2)), dim3(256), 0, s, a);
            return GS_OK;
        });
    } else {
        L.run(K_DEC3, px2 * (2 * ncls * 9 * ncls * 2) + px2 * (ncls * ncls * 4 * 2), [&] {
            if constexpr (l3c_side_sums(CLS)) {   // the raw cat, its BR on load: a 2 x 2 block of pixels per thread
                Dec3CatArgs a{};
                a.l3c = view(m->l3c);
                a.o2c = view(m->o2c);
                a.br = wb + m->w.cbr0;
                a.wc = wb + m->w.wcc;
                a.bnc = wb + m->w.bncc;
                a.wup = wb + m->w.wup2;
                a.bnu = wb + m->w.bnu2;
                a.e = view(m->ee);
                a.N = n;
                hipLaunchKernelGGL(dec3_cat_kernel<CLS>, dim3(blocks_for((long long)n * H2 * W2 / DEC3_PX)), dim3(256), 0, s, a);
            } else {
                Dec3Args a{};
                a.t = view(m->tt);
                a.wc = wb + m->w.wcc;
                a.bnc = wb + m->w.bncc;
                a.wup = wb + m->w.wup2;
                a.bnu = wb + m->w.bnu2;
                a.e = view(m->ee);
                a.N = n;
                a.classes = ncls;
                hipLaunchKernelGGL(dec3_kernel<CLS>, dim3(blocks_for((long long)n * H2 * W2)), dim3(256), 0, s, a);
            }
            return GS_OK;
        });
    }
    m->set_stage("up_l2", m->ee, ncls);
    // ---- conv CBR(19+c,c,3) + classifier deconv + argmax + counts (Model.py:375-377, VisualizeResults_iou.py:128,151-155)
    if constexpr (dec_tail_fused(CLS)) {
        L.run(K_DEC_TAIL, px1 * ((19 + CLS) * 9 * CLS * 2) + px1 * (CLS * CLS * 4 * 2), [&] {
            DecTailArgs a{};
            a.in = m->a0c.base;
            a.in_sn = m->a0c.sn;
            a.in_sc = m->a0c.sc;
            a.in_pitch = m->a0c.pitch;
            a.in_off = m->a0c.off;
            a.in_img_bytes = (unsigned)(m->a0c.sn * sizeof(float));
            a.wpack = wb + m->w.wtail;
            a.logits = r.logits;
            a.mask = r.mask;
            a.hist = ens_finishes((int)r.role) ? r.hist : nullptr;   // only the last member of an ensemble counts
            a.prob = r.prob;
            a.ens_mode = (int)r.role;
            a.ens_w = r.ens_w;
            if (r.logits) {   // debug / test path: the half-resolution CBR output is kept as stage "conv"
                a.ff = m->ff.base;
                a.ff_sn = m->ff.sn;
                a.ff_sc = m->ff.sc;
                a.ff_pitch = m->ff.pitch;
                a.ff_off = m->ff.off;
            }
            a.N = n;
            a.H1 = H1;
            a.W1 = W1;
            return launch_dec_tail(a, m->num_cus, s);
        });
        if (r.logits)
            m->set_stage("conv", m->ff, CLS);
    } else {
        // Any other class count (Model.py:311: `classes` is free, 20 by default): the 3x3 over the 19 + classes planes of the concat
        // buffer as a plain conv_mfma launch (MFMA rows = the padded output channels, BN + PReLU in its epilogue), then the
        // classifier deconvolution + argmax + counts (+ the ensemble's softmax accumulation) as a second kernel.
        L.run(K_DEC_CONV, px1 * ((19 + ncls) * 9 * ncls * 2), [&] {
            return launch_planned<0, CLS>(m, plan.dec_conv, conv_args(m->a0c, wb + m->w.wconv, m->ff, nullptr, n), s);
        });
        m->set_stage("conv", m->ff, ncls);
        L.run(K_DEC4, px1 * (ncls * ncls * 4 * 2), [&] {
            Dec4Args a{};
            a.f = view(m->ff);
            a.wcl = wb + m->w.wclassifier;
            a.logits = r.logits;
            a.mask = r.mask;
            a.hist = r.hist;
            a.prob = r.prob;
            a.ens_mode = (int)r.role;
            a.ens_w = r.ens_w;
            a.N = n;
            a.classes = ncls;
            const dim3 grid(blocks_for(((long long)H1 * W1 + dec4_px<CLS>() - 1) / dec4_px<CLS>()), n);
            hipLaunchKernelGGL((r.role != EnsRole::NONE ? dec4_kernel<CLS, true> : dec4_kernel<CLS, false>), grid, dim3(256), 0, s, a);
            return GS_OK;
        });
    }
    return L.st;
}

// the decoder kernels exist for the padded class counts 4, 5, 8, 12, 16, 20 (Model::cp)
static gs_status forward_any(Model *m, const ForwardReq &r)
{
    Launcher L{m, r.s, GS_OK, r.n};
    const ForwardPlan plan = plan_forward(r.n, r.H, r.W, m->p, m->q, m->cp, m->num_cus, no_vec(), m->encoder_only, r.logits != nullptr);   // every choice of a kernel form
    const Encoded e = encode(m, L, plan, r);
    switch (m->cp) {
    case 5: return decode<5>(m, L, plan, r, e);
    case 4: return decode<4>(m, L, plan, r, e);
    case 8: return decode<8>(m, L, plan, r, e);
    case 12: return decode<12>(m, L, plan, r, e);
    case 16: return decode<16>(m, L, plan, r, e);
    case 20: return decode<20>(m, L, plan, r, e);
    }
    set_error("internal: no decoder instantiation for %d padded classes", m->cp);
    return GS_ERR_UNSUPPORTED;
}

// staging of gs_espnet_segment_host (host_pipe.h): four slots, two per compute stream, kept across calls
struct TileSlot : PipeSlot {
    Staging<uint8_t> in, out;
    Staging<unsigned long long> hist;
    void free_staging() { in.free(), out.free(), hist.free(); }
};

}  // namespace gs

using namespace gs;

// ==========================================================================================
extern "C" {

const char *gs_last_error(void) { return g_err.c_str(); }
int gs_abi_version(void) { return 10; }   // 2: lanes, block hook, detector, compositor LUT; 3: batched crop entries, detector host entry, build flags; 4: any class count 2..20 (hist is [n,classes]), batch planner, pinned-block query, overlays from the crop pipeline; 5: gs_device_fault_check, GS_ERR_DEVICE_FAULT; 6: gs_wsi_eval_windows; 7: ESPNet-C handles give class maps and counts (forward, segment_host, the crop entries with one model); 8: gs_espnet_plan_forward, gs_espnet_form_info; 9: gs_conv2d_nhwc_form, gs_detector_layer_info, gs_detector_plan; 10: gs_crops_from_masks (the crop stage behind the masks, no handle)
gs_status gs_device_fault_check(void)
{
    GS_HIP(hipDeviceSynchronize());
    int flags = 0;
    gs_status st = dec_tail_fault_flags(&flags);
    if (st != GS_OK) return st;
    if (flags) {
        set_error("device fault word %d: a decoder-tail wave gave up its strip-boundary exchange; the results of the calls since the last check are invalid", flags);
        return GS_ERR_DEVICE_FAULT;
    }
    return GS_OK;
}
int gs_build_flags(void)
{
    int flags = CFG_L3_ODD_2B ? 0 : GS_BUILD_NO_ODD_2B;
#ifdef GS_DIAG
    flags |= GS_BUILD_DIAG;
#endif
    return flags;
}

// A handle = the model (weights + lane-0 workspace) plus optional extra LANES: shallow copies of the model that share
// the device weight blob and own a workspace of their own, so that two batches can be in flight on two HIP streams
// (gs_espnet_forward_lane).  Consecutive kernels of one forward cannot overlap (each waits for its predecessor and the
// big ones fill every CU), but the tail of one batch's kernel and the head of another batch's can.
struct gs_espnet {
    Model m;
    std::vector<std::unique_ptr<Model>> lanes;   // lane k >= 1 is lanes[k - 1]
    HostPipe<TileSlot, 4> tile_pipe;             // gs_espnet_segment_host: staging state
    gs::CropPipe *crop_pipe = nullptr;           // gs_espnet_segment_crops*: staging state (csrc/crops.hip)
    Model &lane(int k) { return k == 0 ? m : *lanes[k - 1]; }
};

}  // extern "C"

namespace gs {
CropPipe *&espnet_crop_pipe(gs_espnet *h) { return h->crop_pipe; }
int espnet_device(gs_espnet *h) { return h->m.device; }
int espnet_is_full_net(gs_espnet *h) { return h->m.encoder_only ? 0 : 1; }
int espnet_lanes(gs_espnet *h) { return 1 + (int)h->lanes.size(); }
int espnet_classes(gs_espnet *h) { return h->m.classes; }
// the ensemble's fp32 probability accumulator [n][classes][height][width] of lane `lane`, owned by the first member's handle (one
// per lane: the crop host pipeline has two lanes' batches in flight on two streams)
static gs_status ensemble_scratch(gs_espnet *h, int lane, int n, int height, int width, float **prob)
{
    GS_REQUIRE(lane >= 0 && lane <= (int)h->lanes.size(), "lane %d does not exist (gs_espnet_set_lanes)", lane);
    Model &m0 = h->lane(lane);
    const gs_status st = grow(m0.prob, m0.prob_bytes, (size_t)n * m0.classes * height * width * sizeof(float), "ensemble scratch");
    *prob = m0.prob;
    return st;
}
gs_status espnet_forward(gs_espnet *h, int lane, const ForwardReq &r)
{
    GS_REQUIRE(h && r.in, "forward: null handle or input");
    GS_REQUIRE(lane >= 0 && lane <= (int)h->lanes.size(), "lane %d does not exist (gs_espnet_set_lanes)", lane);
    Model &m = h->lane(lane);
    GS_REQUIRE(!m.encoder_only || r.role == EnsRole::NONE, "an ESPNet-C handle cannot be an ensemble member");
    const gs_status st = layout_workspace(&m, r.n, r.H, r.W);
    return st != GS_OK ? st : forward_any(&m, r);
}

// what a list of members is: GS_OK and *enc_only (all full / all ESPNet-C), or the refusal of a mixed list, of members that
// disagree on the class count, of more than GS_MAX_ENSEMBLE_C ESPNet-C members and of one ESPNet-C handle listed twice (its
// workspace holds ONE set of logits)
gs_status ensemble_kind(gs_espnet *const *models, int n_models, bool *enc_only)
{
    int n_enc = 0;
    for (int k = 0; k < n_models; ++k) {
        GS_REQUIRE(models[k], "ensemble member %d is null", k);
        n_enc += models[k]->m.encoder_only ? 1 : 0;
    }
    *enc_only = n_enc == n_models;
    for (int k = 0; k < n_models; ++k) {
        // a mixed list, full and ESPNet-C members in either order
        GS_REQUIRE(*enc_only || !models[k]->m.encoder_only, "ensemble member %d is not a full ESPNet", k);
        GS_REQUIRE(models[k]->m.classes == models[0]->m.classes, "ensemble member %d has %d classes, member 0 has %d", k,
                   models[k]->m.classes, models[0]->m.classes);
        for (int j = 0; *enc_only && j < k; ++j)
            GS_REQUIRE(models[j] != models[k], "ESPNet-C ensemble members %d and %d are the same handle", j, k);
    }
    if (*enc_only && n_models > GS_MAX_ENSEMBLE_C) {
        set_error("an ESPNet-C ensemble has at most %d members (got %d)", GS_MAX_ENSEMBLE_C, n_models);
        return GS_ERR_UNSUPPORTED;
    }
    return GS_OK;
}

// ESPNet-C ensembles (enc_head_ens.h): the one head launch behind the K trunks of lane `lane`, class map and counts from the
// members' 1/8-scale logits where they lie (the up_l3 buffer of each member's workspace: decode, `enc_logits`); `r`: the ensemble's request
static gs_status espnet_c_ensemble_head(gs_espnet *const *models, int n_models, int lane, const ForwardReq &r)
{
    EncHeadEnsArgs a{};
    for (int k = 0; k < n_models; ++k) {
        const Model &mk = models[k]->lane(lane);
        GS_REQUIRE(mk.encoder_only && mk.ws && r.n <= mk.ws_n && r.H == mk.ws_h && r.W == mk.ws_w,
                   "internal: member %d holds no 1/8-scale logits of this batch", k);
        a.logits[k] = mk.o2c.base;
    }
    a.mask = r.mask;
    a.hist = r.hist;
    a.classes = models[0]->m.classes;
    a.members = n_models;
    a.H3 = r.H / 8;
    a.W3 = r.W / 8;
    a.inv_members = 1.0f / (float)n_models;
    Model &m0 = models[0]->lane(lane);   // (the profiler of the first member times the head)
    Launcher L{&m0, r.s, GS_OK, r.n};
    L.run(K_ENC_HEAD_ENS, (double)r.H * r.W * (a.classes * n_models * 20), [&] {
        launch_ens_head(a, r.n, r.s);
        return GS_OK;
    });
    return L.st;
}

gs_status run_ensemble(gs_espnet *const *models, int n_models, int lane, const ForwardReq &shared, const float *means,
                       const float *stds, const std::function<gs_status(int)> &prepare)
{
    const bool enc_only = models[0]->m.encoder_only;   // (ensemble_kind: then every member is)
    ForwardReq r = shared;
    r.ens_w = 1.0f / (float)n_models;
    // Full networks: every member's decoder tail turns its logits into probabilities in registers and adds 1/K of them into ONE
    // fp32 accumulator (the first member stores, middle members add, the last adds and goes on to the argmax and the counts): the
    // logits are never written, and the accumulator is read K-1 and written K-1 times.
    // ESPNet-C members: the K trunks one after the other on the call's stream -- a trunk is a forward that is asked for no mask
    // (ForwardReq::hist) -- then ONE head over their 1/8-scale logits.  No accumulator; K = 1 runs the same code.
    gs_status st = GS_OK;
    if (!enc_only && (st = ensemble_scratch(models[0], lane, r.n, r.H, r.W, &r.prob)) != GS_OK) return st;
    for (int k = 0; k < n_models; ++k) {
        if (prepare && (st = prepare(k)) != GS_OK) return st;
        r.mean = means ? means + 3 * k : nullptr, r.stdv = stds ? stds + 3 * k : nullptr;
        if (enc_only)   // (the first trunk's stem zeroes what the head counts into)
            r.mask = nullptr, r.hist = k == 0 ? shared.hist : nullptr;
        else
            r.role = ens_role(k, n_models);
        st = espnet_forward(models[k], lane, r);
        if (st != GS_OK) return st;
    }
    return enc_only ? espnet_c_ensemble_head(models, n_models, lane, shared) : GS_OK;
}
}  // namespace gs

extern "C" {

// what gs_espnet_create and gs_espnet_pack_weights (`fn`) ask of their common arguments
static gs_status check_model_args(const char *fn, const float *blob, const gs_layer_desc *table, int n_layers, int classes, int p, int q)
{
    GS_REQUIRE(blob && table && n_layers > 0, "%s: null argument", fn);
    GS_REQUIRE(p >= 0 && q >= 0, "%s: p and q must be non-negative", fn);
    // Model.py:311,246: `classes` is free (20 by default).  The decoder kernels exist for 2..20 (padded to 4, 5, 8, 12, 16, 20
    // planes: Model::cp); class maps are uint8 and a lane's per-class counters are sized for at most 20.
    if (classes < 2 || classes > 20) {
        set_error("%s: classes must be 2..20 (got %d)", fn, classes);
        return GS_ERR_UNSUPPORTED;
    }
    return GS_OK;
}

gs_status gs_espnet_create(const float *blob, const gs_layer_desc *table, int n_layers, int classes, int p, int q,
                           int encoder_only, gs_espnet **out)
{
    GS_REQUIRE(out, "gs_espnet_create: null argument");
    gs_status st = check_model_args("gs_espnet_create", blob, table, n_layers, classes, p, q);
    if (st != GS_OK) return st;
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev == 0) {
        set_error("gs_espnet_create: no HIP device visible");
        return GS_ERR_NODEVICE;
    }
    std::unique_ptr<gs_espnet> h(new gs_espnet());
    Model &m = h->m;
    m.classes = classes;
    m.cp = padded_classes(classes);
    m.p = p;
    m.q = q;
    m.encoder_only = encoder_only != 0;
    GS_HIP(hipGetDevice(&m.device));
    hipDeviceProp_t prop;
    GS_HIP(hipGetDeviceProperties(&prop, m.device));
    if (std::strncmp(prop.gcnArchName, "gfx950", 6) != 0) {
        set_error("gs_espnet_create: device %d is %s; this library is built for gfx950 only", m.device, prop.gcnArchName);
        return GS_ERR_NODEVICE;
    }
    m.num_cus = prop.multiProcessorCount;
#ifdef GS_DIAG
    if (const char *v = std::getenv("GS_VARIANT"))
        m.variant = std::atoi(v);
#endif
    EspnetWeights packed;   // every layout of the weights: espnet_weights.h
    st = pack_espnet_weights(blob, table, n_layers, classes, p, q, m.encoder_only, packed);
    if (st != GS_OK) return st;
    m.w = packed;
    GS_HIP(hipMalloc(reinterpret_cast<void **>(&m.dblob), packed.blob.size() * sizeof(float)));
    GS_HIP(hipMemcpy(m.dblob, packed.blob.data(), packed.blob.size() * sizeof(float), hipMemcpyHostToDevice));
    *out = h.release();
    return GS_OK;
}

gs_status gs_espnet_pack_weights(const float *blob, const gs_layer_desc *table, int n_layers, int classes, int p, int q,
                                 int encoder_only, float *out, size_t cap, size_t *n_floats, gs_weight_piece *pieces, int piece_cap,
                                 int *n_pieces)
{
    GS_REQUIRE(n_floats, "gs_espnet_pack_weights: null argument");
    gs_status st = check_model_args("gs_espnet_pack_weights", blob, table, n_layers, classes, p, q);
    if (st != GS_OK) return st;
    EspnetWeights packed;
    st = pack_espnet_weights(blob, table, n_layers, classes, p, q, encoder_only != 0, packed);
    if (st != GS_OK) return st;
    *n_floats = packed.blob.size();
    if (n_pieces) *n_pieces = (int)packed.pieces.size();
    if (out) {
        GS_REQUIRE(cap >= packed.blob.size(), "gs_espnet_pack_weights: %zu floats needed, room for %zu", packed.blob.size(), cap);
        std::memcpy(out, packed.blob.data(), packed.blob.size() * sizeof(float));
    }
    if (pieces) {
        GS_REQUIRE(piece_cap >= (int)packed.pieces.size(), "gs_espnet_pack_weights: %zu pieces, room for %d", packed.pieces.size(), piece_cap);
        std::memcpy(pieces, packed.pieces.data(), packed.pieces.size() * sizeof(gs_weight_piece));
    }
    return GS_OK;
}

// what a lane owns on the device (the weight blob is the handle's); the caller has synchronised
static void free_lane(Model &l)
{
    for (auto &ev : l.events) {
        hipEventDestroy(ev.a);
        hipEventDestroy(ev.b);
    }
    if (l.ws) hipFree(l.ws);
    if (l.prob) hipFree(l.prob);
}

void gs_espnet_destroy(gs_espnet *h)
{
    if (!h)
        return;
    hipDeviceSynchronize();
    h->tile_pipe.destroy();
    crop_pipe_destroy(h->crop_pipe);
    for (int k = 0; k <= (int)h->lanes.size(); ++k)
        free_lane(h->lane(k));
    if (h->m.dblob) hipFree(h->m.dblob);
    delete h;
}

static gs_status check_shape(int n, int height, int width)
{
    GS_REQUIRE(n > 0, "batch size must be positive (got %d)", n);
    GS_REQUIRE(height >= 8 && width >= 8 && height % 8 == 0 && width % 8 == 0,
               "tile size must be a positive multiple of 8 in both dimensions (got %dx%d)", height, width);
    return GS_OK;
}

gs_status gs_espnet_reserve(gs_espnet *h, int n, int height, int width)
{
    GS_REQUIRE(h, "null handle");
    gs_status st = check_shape(n, height, width);
    if (st != GS_OK) return st;
    for (int k = 0; k <= (int)h->lanes.size(); ++k) {
        st = layout_workspace(&h->lane(k), n, height, width);
        if (st != GS_OK) return st;
    }
    return GS_OK;
}

gs_status gs_espnet_workspace_plan(int n, int height, int width, int p, int q, int classes, int encoder_only, size_t *bytes)
{
    GS_REQUIRE(bytes, "gs_espnet_workspace_plan: null argument");
    gs_status st = check_shape(n, height, width);
    if (st != GS_OK) return st;
    GS_REQUIRE(p >= 0 && q >= 0, "gs_espnet_workspace_plan: p and q must be non-negative");
    if (classes < 2 || classes > 20) {
        set_error("gs_espnet_workspace_plan: classes must be 2..20 (got %d)", classes);
        return GS_ERR_UNSUPPORTED;
    }
    WorkspacePlan plan;
    st = plan_workspace(n, height, width, padded_classes(classes), p, encoder_only != 0, plan);
    *bytes = plan.bytes;
    return st;
}

// ---- include/glomseg_workspace.h: test tools over csrc/workspace_audit.h
static gs_status workspace_plan_checked(const char *fn, int n, int height, int width, int p, int q, int classes, int encoder_only,
                                        gs::WorkspacePlan &plan)
{
    gs_status st = check_shape(n, height, width);
    if (st != GS_OK) return st;
    GS_REQUIRE(p >= 0 && q >= 0, "%s: p and q must be non-negative", fn);
    if (classes < 2 || classes > 20) {
        set_error("%s: classes must be 2..20 (got %d)", fn, classes);
        return GS_ERR_UNSUPPORTED;
    }
    return plan_workspace(n, height, width, padded_classes(classes), p, encoder_only != 0, plan);
}

static void fill_report(const WsReport &rep, gs_workspace_report *out)
{
    static_assert(sizeof(WsReport) == sizeof(gs_workspace_report), "WsReport is gs_workspace_report field for field");
    std::memcpy(out, &rep, sizeof rep);
}

gs_status gs_espnet_workspace_classes(int ws_n, int height, int width, int p, int q, int classes, int encoder_only, int piece,
                                      gs_workspace_piece *info, unsigned char *map, size_t cap, int *n_pieces)
{
    WorkspacePlan plan;
    const gs_status st = workspace_plan_checked("gs_espnet_workspace_classes", ws_n, height, width, p, q, classes, encoder_only, plan);
    if (st != GS_OK) return st;
    if (n_pieces) *n_pieces = WS_PIECES;
    if (!info && !map)
        return GS_OK;
    GS_REQUIRE(piece >= 0 && piece < WS_PIECES, "gs_espnet_workspace_classes: piece %d of %d", piece, WS_PIECES);
    const WsPiece pc = ws_piece(plan, ws_n, piece, classes);
    if (info) {
        *info = gs_workspace_piece{};
        std::strncpy(info->name, pc.name, sizeof info->name - 1);
        info->offset = pc.at, info->own_words = pc.own_words, info->span_words = pc.span_words, info->padded = pc.padded;
        info->C = pc.act.C, info->Cp = pc.act.Cp, info->H = pc.act.H, info->W = pc.act.W;
        info->pitch = pc.act.pitch, info->sc = pc.act.sc, info->off = pc.act.off;
    }
    if (map) {
        GS_REQUIRE(cap >= pc.span_words, "gs_espnet_workspace_classes: %zu bytes needed, room for %zu", pc.span_words, cap);
        ws_class_map(pc, map);
    }
    return GS_OK;
}

gs_status gs_espnet_workspace_audit_host(int ws_n, int height, int width, int p, int q, int classes, int encoder_only,
                                         const void *copy, size_t bytes, gs_workspace_report *report)
{
    GS_REQUIRE(copy && report, "gs_espnet_workspace_audit_host: null argument");
    WorkspacePlan plan;
    const gs_status st = workspace_plan_checked("gs_espnet_workspace_audit_host", ws_n, height, width, p, q, classes, encoder_only, plan);
    if (st != GS_OK) return st;
    GS_REQUIRE(bytes == plan.bytes, "gs_espnet_workspace_audit_host: the workspace has %zu bytes, the copy %zu", plan.bytes, bytes);
    WsReport rep;
    for (int i = 0; i < WS_PIECES; ++i) {
        const WsPiece pc = ws_piece(plan, ws_n, i, classes);
        ws_audit_piece(pc, reinterpret_cast<const uint32_t *>(static_cast<const char *>(copy) + pc.at), rep);
    }
    fill_report(rep, report);
    return GS_OK;
}

// the plan of a lane's workspace as layout_workspace laid it out
static gs_status lane_workspace_plan(const Model &m, WorkspacePlan &plan)
{
    const gs_status st = plan_workspace(m.ws_n, m.ws_h, m.ws_w, m.cp, m.p, m.encoder_only, plan);
    if (st != GS_OK) return st;
    GS_REQUIRE(plan.bytes == m.ws_bytes, "internal: the workspace has %zu bytes, its plan %zu", m.ws_bytes, plan.bytes);
    return GS_OK;
}

gs_status gs_espnet_workspace_audit(gs_espnet *h, int lane, gs_workspace_report *report)
{
    GS_REQUIRE(h && report, "gs_espnet_workspace_audit: null argument");
    GS_REQUIRE(lane >= 0 && lane <= (int)h->lanes.size(), "lane %d does not exist (gs_espnet_set_lanes)", lane);
    const Model &m = h->lane(lane);
    WsReport rep;
    GS_HIP(hipDeviceSynchronize());
    if (m.ws) {
        WorkspacePlan plan;
        const gs_status st = lane_workspace_plan(m, plan);
        if (st != GS_OK) return st;
        std::vector<uint32_t> host;
        for (int i = 0; i < WS_PIECES; ++i) {
            const WsPiece pc = ws_piece(plan, m.ws_n, i, m.classes);
            host.resize(pc.span_words);
            GS_HIP(hipMemcpy(host.data(), static_cast<const char *>(m.ws) + pc.at, pc.span_words * sizeof(uint32_t), hipMemcpyDeviceToHost));
            ws_audit_piece(pc, host.data(), rep);
        }
    }
    fill_report(rep, report);
    return GS_OK;
}

gs_status gs_espnet_workspace_poison(gs_espnet *h, int lane, unsigned int pattern)
{
    GS_REQUIRE(h, "gs_espnet_workspace_poison: null handle");
    GS_REQUIRE(lane >= 0 && lane <= (int)h->lanes.size(), "lane %d does not exist (gs_espnet_set_lanes)", lane);
    Model &m = h->lane(lane);
    GS_HIP(hipDeviceSynchronize());
    if (!m.ws)
        return GS_OK;
    if (m.ws_bytes > ((size_t)1 << 30)) {
        set_error("gs_espnet_workspace_poison: a workspace of %zu bytes is above the 1 GiB this test tool takes", m.ws_bytes);
        return GS_ERR_UNSUPPORTED;
    }
    WorkspacePlan plan;
    const gs_status st = lane_workspace_plan(m, plan);
    if (st != GS_OK) return st;
    std::vector<uint32_t> host;
    for (int i = 0; i < WS_PIECES; ++i) {   // a span goes down, its interior and free words are overwritten, and it goes back
        const WsPiece pc = ws_piece(plan, m.ws_n, i, m.classes);
        char *dev = static_cast<char *>(m.ws) + pc.at;
        host.resize(pc.span_words);
        GS_HIP(hipMemcpy(host.data(), dev, pc.span_words * sizeof(uint32_t), hipMemcpyDeviceToHost));
        ws_poison_piece(pc, host.data(), pattern);
        GS_HIP(hipMemcpy(dev, host.data(), pc.span_words * sizeof(uint32_t), hipMemcpyHostToDevice));
    }
    GS_HIP(hipDeviceSynchronize());
    m.stages.clear();   // the workspace no longer holds a forward's stages
    return GS_OK;
}

gs_status gs_espnet_set_lanes(gs_espnet *h, int n_lanes)
{
    GS_REQUIRE(h, "null handle");
    GS_REQUIRE(n_lanes >= 1 && n_lanes <= 4, "gs_espnet_set_lanes: 1 to 4 lanes (got %d)", n_lanes);
    GS_HIP(hipDeviceSynchronize());
    while ((int)h->lanes.size() > n_lanes - 1) {
        free_lane(*h->lanes.back());
        h->lanes.pop_back();
    }
    while ((int)h->lanes.size() < n_lanes - 1) {
        std::unique_ptr<Model> l(new Model(h->m));   // same weights (shared device blob), same configuration ...
        l->ws = nullptr;                             // ... and nothing else of the original: own workspace, no profile
        l->ws_bytes = 0;
        l->ws_n = l->ws_h = l->ws_w = 0;
        l->prob = nullptr;
        l->prob_bytes = 0;
        l->stages.clear();
        l->events.clear();
        l->profile = false;
        h->lanes.push_back(std::move(l));
    }
    return GS_OK;
}

int gs_espnet_lanes(gs_espnet *h) { return h ? 1 + (int)h->lanes.size() : 0; }

gs_status gs_espnet_forward(gs_espnet *h, const void *in, int in_format, int n, int height, int width,
                            const float mean[3], const float std[3], float *logits, uint8_t *mask,
                            unsigned long long *hist, void *hip_stream)
{
    return gs_espnet_forward_lane(h, 0, in, in_format, n, height, width, mean, std, logits, mask, hist, hip_stream);
}

gs_status gs_espnet_forward_lane(gs_espnet *h, int lane, const void *in, int in_format, int n, int height, int width,
                                 const float mean[3], const float std[3], float *logits, uint8_t *mask,
                                 unsigned long long *hist, void *hip_stream)
{
    GS_REQUIRE(h && in, "gs_espnet_forward: null handle or input");
    GS_REQUIRE(lane >= 0 && lane <= (int)h->lanes.size(), "lane %d does not exist (gs_espnet_set_lanes)", lane);
    gs_status st = check_shape(n, height, width);
    if (st != GS_OK) return st;
    GS_REQUIRE(in_format == GS_IN_U8_BGR_NHWC || in_format == GS_IN_F32_NCHW, "unknown input format %d", in_format);
    GS_REQUIRE(in_format != GS_IN_U8_BGR_NHWC || (mean && std), "uint8 input needs mean and std");
    // (an ESPNet-C handle's logits are the 1/8-scale ones; its mask and counts come from the head kernel, enc_head.h)
    GS_REQUIRE(logits || mask, "nothing to compute: logits and mask are both NULL");
    GS_REQUIRE(!hist || mask, "hist requires the mask output");
    if (in_format == GS_IN_U8_BGR_NHWC)
        for (int i = 0; i < 3; ++i)
            GS_REQUIRE(std[i] != 0.0f, "std[%d] is zero", i);
    ForwardReq r;
    r.in = in, r.in_format = in_format, r.n = n, r.H = height, r.W = width;
    r.mean = mean, r.stdv = std, r.logits = logits, r.mask = mask, r.hist = hist, r.s = static_cast<hipStream_t>(hip_stream);
    return espnet_forward(h, lane, r);
}

gs_status gs_espnet_read_stage(gs_espnet *h, const char *stage, int image, float *dst, size_t cap, int dims[3])
{
    GS_REQUIRE(h && stage && dims, "gs_espnet_read_stage: null argument");
    Model &m = h->m;
    auto it = m.stages.find(stage);
    GS_REQUIRE(it != m.stages.end(), "stage '%s' was not produced by the last forward%s", stage,
               m.lean ? " (a lean forward -- mask-only, glomseg_lean.h -- materialises neither 'combine_t' nor the last 'level3.<i>', and no "
                        "mask-only forward keeps 'conv': request logits to read them)" : "");
    GS_REQUIRE(image >= 0 && image < m.last_n, "image index %d out of range", image);
    const Act &a = it->second.first;
    const int C = it->second.second;
    dims[0] = C;
    dims[1] = a.H;
    dims[2] = a.W;
    const size_t count = (size_t)C * a.H * a.W;
    if (!dst)
        return GS_OK;
    GS_REQUIRE(cap >= count, "destination too small for stage '%s'", stage);
    float *tmp = nullptr;
    GS_HIP(hipMalloc(reinterpret_cast<void **>(&tmp), count * sizeof(float)));
    hipLaunchKernelGGL(unpad_kernel, dim3(blocks_for((long long)count)), dim3(256), 0, 0, view(a), image, C, tmp);
    if (m.b2_lazy && std::string(stage) == "b2")   // planes 64..127 are kept raw in the workspace: normalise the copy
        hipLaunchKernelGGL(b2_apply_kernel, dim3(blocks_for((long long)64 * a.H * a.W)), dim3(256), 0, 0, tmp, m.dblob + m.w.b2, a.H * a.W, 64, 64);
    hipError_t e = hipMemcpy(dst, tmp, count * sizeof(float), hipMemcpyDeviceToHost);
    hipFree(tmp);
    GS_HIP(e);
    return GS_OK;
}

gs_status gs_espnet_block_forward(gs_espnet *h, int kind, int level, int index, const float *in, int height, int width,
                                  float *out)
{
    GS_REQUIRE(h && in && out, "gs_espnet_block_forward: null argument");
    GS_REQUIRE((kind == 0 || kind == 1) && (level == 2 || level == 3), "kind must be 0/1 and level 2/3");
    GS_REQUIRE(height >= 1 && width >= 1, "empty input");
    Model &m = h->m;
    GS_REQUIRE(kind == 1 || (index >= 0 && index < (level == 2 ? m.p : m.q)), "no ESP block %d at level %d", index, level);
    GS_REQUIRE(kind == 0 || (height % 2 == 0 && width % 2 == 0), "the down-sampler needs an even input size");
    // the tile size whose pyramid has this block at the given size
    const int up = kind == 0 ? (level == 2 ? 4 : 8) : (level == 2 ? 2 : 4);
    gs_status st = layout_workspace(&m, 1, height * up, width * up);
    if (st != GS_OK) return st;
    const float *wb = m.dblob;
    const Act &src = kind == 0 ? (level == 2 ? m.bb[0] : m.cc[0]) : (level == 2 ? m.a0 : m.a1);
    const Act &dst = level == 2 ? (kind == 0 ? m.bb[1] : m.bb[0]) : (kind == 0 ? m.cc[1] : m.cc[0]);
    const Act &red = level == 2 ? m.r2[0] : m.r3[0];
    const int cin = kind == 0 ? (level == 2 ? 64 : 128) : (level == 2 ? 19 : 131);
    const int cout = level == 2 ? 64 : 128;
    GS_REQUIRE(src.H == height && src.W == width, "internal: workspace level size mismatch");
    const size_t nin = (size_t)cin * height * width, nout = (size_t)cout * dst.H * dst.W;
    float *tmp = nullptr;
    GS_HIP(hipMalloc(reinterpret_cast<void **>(&tmp), (nin > nout ? nin : nout) * sizeof(float)));
    gs_status rc = GS_OK;
    hipStream_t s = nullptr;
    auto body = [&]() -> gs_status {
        GS_HIP(hipMemcpy(tmp, in, nin * sizeof(float), hipMemcpyHostToDevice));
        hipLaunchKernelGGL(pad_kernel, dim3(blocks_for((long long)nin)), dim3(256), 0, s, view(src), 0, cin, tmp);
        const PackedConv &pc = kind == 1 ? (level == 2 ? m.w.l2_0 : m.w.l3_0) : (level == 2 ? m.w.l2[index] : m.w.l3[index]);
        // the block's reduce, then its branches in the unfused whole-row form its output width allows (forward_plan.h)
        const ConvArgs rca = conv_args(src, wb + pc.c1, red, nullptr, 1);
        const ConvArgs bca = conv_args(red, wb + pc.br, dst, kind == 1 ? nullptr : &src, 1);
        gs_status r;
        if (level == 2) {
            r = kind == 1 ? launch_l2_reduce(&m, rca, s) : launch_l2_c1(&m, rca, s);
            if (r != GS_OK) return r;
            r = kind == 1 ? launch_planned(&m, unfused_l2_down(dst.W, no_vec()), bca, s)
                          : launch_planned(&m, unfused_l2_esp(dst.W, no_vec()), bca, s);
        } else {
            r = kind == 1 ? launch_l3_reduce(&m, form::l3_reduce::C1S, false, rca, s) : launch_l3_c1(&m, rca, s);
            if (r != GS_OK) return r;
            r = kind == 1 ? launch_l3_down(&m, unfused_l3_down(dst.W, no_vec()), false, bca, s)
                          : launch_l3_esp_last(&m, whole_row_l3_esp(dst.W, no_vec()), false, false, bca, s);
        }
        if (r != GS_OK) return r;
        hipLaunchKernelGGL(unpad_kernel, dim3(blocks_for((long long)nout)), dim3(256), 0, s, view(dst), 0, cout, tmp);
        GS_HIP(hipGetLastError());
        GS_HIP(hipMemcpy(out, tmp, nout * sizeof(float), hipMemcpyDeviceToHost));
        return GS_OK;
    };
    rc = body();
    hipFree(tmp);
    m.stages.clear();   // the workspace no longer holds a forward's stages
    return rc;
}

gs_status gs_espnet_plan_forward(int n, int height, int width, int p, int q, int classes, int num_cus, int *out_forms, int cap,
                                 int *n_out)
{
    GS_REQUIRE(n_out, "gs_espnet_plan_forward: null argument");
    gs_status st = check_shape(n, height, width);
    if (st != GS_OK) return st;
    GS_REQUIRE(p >= 0 && q >= 0 && num_cus > 0, "gs_espnet_plan_forward: p and q must be non-negative, num_cus positive");
    if (classes < 2 || classes > 20) {
        set_error("gs_espnet_plan_forward: classes must be 2..20 (got %d)", classes);
        return GS_ERR_UNSUPPORTED;
    }
    *n_out = kLaunchClassCount;
    if (!out_forms)
        return GS_OK;
    GS_REQUIRE(cap >= kLaunchClassCount, "gs_espnet_plan_forward: %d entries needed, room for %d", kLaunchClassCount, cap);
    plan_forward(n, height, width, p, q, padded_classes(classes), num_cus, no_vec()).codes(out_forms);
    return GS_OK;
}

gs_status gs_espnet_plan_flags(int n, int height, int width, int p, int q, int classes, int encoder_only, int num_cus, int *flags)
{
    GS_REQUIRE(flags, "gs_espnet_plan_flags: null argument");
    int count = 0;
    gs_status st = gs_espnet_plan_forward(n, height, width, p, q, classes, num_cus, nullptr, 0, &count);   // (the same refusals)
    if (st != GS_OK) return st;
    const ForwardPlan pl = plan_forward(n, height, width, p, q, padded_classes(classes), num_cus, no_vec(), encoder_only != 0);
    *flags = (pl.lazy_b2 ? GS_PLAN_LAZY_B2 : 0) | (pl.l3c_in_reduce ? GS_PLAN_L3C_IN_REDUCE : 0) | (pl.cls_in_l3 ? GS_PLAN_CLS_IN_L3 : 0);
    return GS_OK;
}

gs_status gs_espnet_plan_lean(int n, int height, int width, int p, int q, int classes, int encoder_only, int num_cus, int want_logits,
                              int *lean)
{
    GS_REQUIRE(lean, "gs_espnet_plan_lean: null argument");
    int count = 0;
    gs_status st = gs_espnet_plan_forward(n, height, width, p, q, classes, num_cus, nullptr, 0, &count);   // (the same refusals)
    if (st != GS_OK) return st;
    *lean = plan_forward(n, height, width, p, q, padded_classes(classes), num_cus, no_vec(), encoder_only != 0, want_logits != 0).lean;
    return GS_OK;
}

gs_status gs_espnet_form_info(int launch_class, int form, const char **name, int *pixels_per_lane)
{
    GS_REQUIRE(launch_class >= 0 && launch_class < kLaunchClassCount, "no launch class %d", launch_class);
    const LaunchClassInfo &c = kLaunchClasses[launch_class];
    GS_REQUIRE(form >= GS_FORM_NONE && form < c.n_forms, "launch class %s has no form %d", c.name, form);
    if (name) *name = form == GS_FORM_NONE ? c.name : c.forms[form].name;   // (no form: the class itself)
    if (pixels_per_lane) *pixels_per_lane = form == GS_FORM_NONE ? 0 : c.forms[form].pixels_per_lane;
    return GS_OK;
}

// gs_espnet_form_odd_2b (glomseg_forms.h): the Spec of every row of the table, in the table's order
#define GS_ODD_ROW(id, name, ppl) (Spec<decltype(F::id), F::id, 5>::odd_2b_legal ? GS_FORM_ODD_2B_LEGAL : 0) | ((Spec<decltype(F::id), F::id, 5>::flags & F_ODD_2B) ? GS_FORM_ODD_2B_BUILT : 0),
#define GS_ODD_CLASS(cls, FORMS)                                 \
    static const int *odd_2b_##cls()                             \
    {                                                            \
        using F = form::cls;                                     \
        static const int rows[] = {FORMS(GS_ODD_ROW) 0};         \
        return rows;                                             \
    }
GS_LAUNCH_CLASSES(GS_ODD_CLASS)
#undef GS_ODD_ROW
#undef GS_ODD_CLASS
int gs_espnet_form_odd_2b(int launch_class, int form)
{
#define GS_ODD_PTR(cls, FORMS) odd_2b_##cls(),
    const int *const rows[] = {GS_LAUNCH_CLASSES(GS_ODD_PTR)};
#undef GS_ODD_PTR
    if (launch_class < 0 || launch_class >= kLaunchClassCount || form < 0 || form >= kLaunchClasses[launch_class].n_forms)
        return -1;
    return rows[launch_class][form];
}

gs_status gs_espnet_profile_enable(gs_espnet *h, int on)
{
    GS_REQUIRE(h, "null handle");
    h->m.profile = on != 0;
    return GS_OK;
}

gs_status gs_espnet_profile_read(gs_espnet *h, gs_kernel_time *out, int cap, int *n_out)
{
    GS_REQUIRE(h && n_out, "null argument");
    Model &m = h->m;
    for (auto &ev : m.events) {
        GS_HIP(hipEventSynchronize(ev.b));
        float ms = 0.0f;
        GS_HIP(hipEventElapsedTime(&ms, ev.a, ev.b));
        m.prof_ms[ev.k] += ms;
        m.prof_launches[ev.k] += 1;
        hipEventDestroy(ev.a);
        hipEventDestroy(ev.b);
    }
    m.events.clear();
    int k = 0;
    for (int i = 0; i < K_COUNT && out && k < cap; ++i) {
        if (!m.prof_launches[i])
            continue;
        std::snprintf(out[k].name, sizeof out[k].name, "%s", kKernelNames[i]);
        out[k].total_ms = m.prof_ms[i];
        out[k].launches = m.prof_launches[i];
        out[k].flops_per_tile = m.prof_flops[i] / (double)m.prof_launches[i];   // mean over the launches timed
        ++k;
    }
    *n_out = k;
    for (int i = 0; i < K_COUNT; ++i) {
        m.prof_ms[i] = 0;
        m.prof_launches[i] = 0;
        m.prof_flops[i] = 0;
    }
    return GS_OK;
}

gs_status gs_espnet_ensemble_forward(gs_espnet *const *models, int n_models, const void *in_u8, int n, int height,
                                     int width, const float *means, const float *stds, uint8_t *mask,
                                     unsigned long long *hist, void *hip_stream)
{
    GS_REQUIRE(models && n_models > 0 && in_u8 && means && stds && mask, "gs_espnet_ensemble_forward: null argument");
    gs_status st = check_shape(n, height, width);
    if (st != GS_OK) return st;
    bool enc_only = false;
    st = ensemble_kind(models, n_models, &enc_only);
    if (st != GS_OK) return st;
    for (int k = 0; k < n_models; ++k)
        for (int i = 0; i < 3; ++i)
            GS_REQUIRE(stds[3 * k + i] != 0.0f, "ensemble member %d: std[%d] is zero", k, i);
    ForwardReq r;
    r.in = in_u8, r.in_format = GS_IN_U8_BGR_NHWC, r.n = n, r.H = height, r.W = width;
    r.mask = mask, r.hist = hist, r.s = static_cast<hipStream_t>(hip_stream);
    return run_ensemble(models, n_models, 0, r, means, stds);
}

gs_status gs_espnet_segment_host(gs_espnet *h, const uint8_t *tiles, int n_tiles, int height, int width,
                                 const float mean[3], const float std[3], int batch, uint8_t *masks,
                                 unsigned long long *hist)
{
    GS_REQUIRE(h && tiles && masks && mean && std, "gs_espnet_segment_host: null argument");
    GS_REQUIRE(n_tiles > 0 && batch > 0, "n_tiles and batch must be positive");
    gs_status st = check_shape(batch, height, width);
    if (st != GS_OK) return st;
    if (batch > n_tiles) batch = n_tiles;
    const size_t in_b = (size_t)height * width * 3, out_b = (size_t)height * width;
    const size_t ncl = (size_t)h->m.classes;   // hist is [n_tiles][classes]
    const int nl = h->lanes.empty() ? 1 : 2;   // batches alternate between (at most) two lanes, each on its own compute stream
    // caller buffers that are already page-locked are DMA'd in place;
    // pageable ones are staged through the pinned slot buffers with a host memcpy
    const bool in_pinned = host_is_pinned(tiles), out_pinned = host_is_pinned(masks) && (!hist || host_is_pinned(hist));
    auto &pipe = h->tile_pipe;
    HipLatch fail;
    if (!pipe.ensure(2, true, fail, [&](TileSlot &s) {
            s.in.grow(in_b * batch, fail);
            s.out.grow(out_b * batch, fail);
            s.hist.grow(sizeof(unsigned long long) * GS_MAX_CLASSES * batch, fail);
        }))
        return fail.rc;
#ifdef GS_DIAG
    // host-side timeline of the loop (GS_PIPE_TRACE=1): where does the enqueueing thread wait?
    const bool ptrace = std::getenv("GS_PIPE_TRACE") != nullptr;
    const auto pt0 = std::chrono::steady_clock::now();
    auto stamp = [&](int bi, const char *what) {
        if (ptrace && bi < 12)
            std::fprintf(stderr, "pipe %2d %-10s %9.1f us\n", bi, what,
                         std::chrono::duration<double, std::micro>(std::chrono::steady_clock::now() - pt0).count());
    };
    const int pskip = std::getenv("GS_PIPE_SKIP") ? std::atoi(std::getenv("GS_PIPE_SKIP")) : 0;   // 1: no uploads, 2: no downloads (timing only)
#else
    auto stamp = [](int, const char *) {};
    constexpr int pskip = 0;
#endif
    const gs_status rc = pipe.run(
        (n_tiles + batch - 1) / batch, nl == 1, fail,
        [&](int bi, TileSlot &s, hipStream_t h2d) {
            s.first = bi * batch;
            s.count = n_tiles - s.first < batch ? n_tiles - s.first : batch;
            const uint8_t *src = tiles + (size_t)s.first * in_b;
            if (!in_pinned) {
                parallel_memcpy(s.in.h, src, in_b * s.count);
                src = s.in.h;
            }
            if (!(pskip & 1) || bi < pipe.NSLOT)
                fail(hipMemcpyAsync(s.in.d, src, in_b * s.count, hipMemcpyHostToDevice, h2d), "H2D copy");
        },
        [&](int bi, TileSlot &s, hipStream_t compute) {
            return gs_espnet_forward_lane(h, bi % nl, s.in.d, GS_IN_U8_BGR_NHWC, s.count, height, width, mean, std, nullptr, s.out.d,
                                          s.hist.d, compute);
        },
        [&](int, TileSlot &s, hipStream_t compute) {
            uint8_t *hdst = out_pinned ? masks + (size_t)s.first * out_b : s.out.h;
            unsigned long long *hhdst = (out_pinned && hist) ? hist + (size_t)s.first * ncl : s.hist.h;
            const size_t hb = sizeof(unsigned long long) * ncl * s.count;
            if (!(pskip & 2))
                fail(hipMemcpy2DAsync(hdst, out_b, s.out.d, out_b, out_b, s.count, hipMemcpyDeviceToHost, compute), "D2H copy");
            if (hist || !out_pinned)
                fail(hipMemcpy2DAsync(hhdst, hb, s.hist.d, hb, hb, 1, hipMemcpyDeviceToHost, compute), "D2H copy");
        },
        [&](TileSlot &s) {
            if (out_pinned)
                return;
            parallel_memcpy(masks + (size_t)s.first * out_b, s.out.h, out_b * s.count);
            if (hist) std::memcpy(hist + (size_t)s.first * ncl, s.hist.h, sizeof(unsigned long long) * ncl * s.count);
        },
        stamp);
    return rc != GS_OK ? rc : gs_device_fault_check();   // (every batch has been drained: a few microseconds)
}

}  // extern "C"
