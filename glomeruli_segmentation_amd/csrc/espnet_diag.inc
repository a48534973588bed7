// -DGS_DIAG builds only (included by espnet.hip under #ifdef GS_DIAG): the timing / stamp variants of the forward, selected by
// the GS_VARIANT environment variable at gs_espnet_create.  Results are wrong by construction unless noted.  Every function
// returns true when it took the launch over (status in `st`).  0 = the shipped configuration: nothing here runs.
//    41  stride-2 reduces with three dword loads per pixel instead of one 12-byte load (results correct)
//   101  level-3 ESP: no epilogue   102 no epilogue, no operand loads   103 ... and no LDS reads   104 no operand loads
//   105  level-3 ESP: per-wave stamps -> $GS_STAMP_DIR/stamps.txt (tools/stamps.py; results correct)   109 stores but no residual
//   160-165  per-chunk stamps of every task of a SHIPPED kernel form -> $GS_STAMP_DIR/stamps_<tag>.txt (tools/stamps3.py; results correct):
//        160 the fused level-3 ESP launch (block 1)   161 the fused level-2 ESP launch   162 the level-2 down-sampler
//        163 the last level-2 ESP launch   164 the level-3 down-sampler   165 the level-3 stride-2 reduce   (stamp_of below)

static bool diag_reduce_s2(Model *m, int level, const ConvArgs &ca, hipStream_t s, gs_status &st)
{
    if (m->variant != 41)
        return false;
    st = level == 2 ? launch_conv_mfma<CFG_L2_C1S, 0>(ca, m->num_cus, s) : launch_conv_mfma<CFG_L3_C1S, 0>(ca, m->num_cus, s);
    return true;
}

// Every stamp file of a diagnostic variant (105, 160-165) lands in the directory the GS_STAMP_DIR environment variable names
// (unset: the working directory); the stamp tools under tools/ set it to their output directory.
static std::string stamp_path(const std::string &name)
{
    const char *dir = std::getenv("GS_STAMP_DIR");
    return std::string(dir ? dir : ".") + "/" + name;
}

// Per-chunk stamps of EVERY task of every wave of one launch of a SHIPPED kernel form (results correct) -> stamps_<tag>.txt
// (stamp_path above), one line per wave: global wave id, then STAMP2_SLOTS stamps (tools/stamps3.py).  The file is written on
// the third stamped call of the process (after warm-up) and the stream is synchronised there.  What is stamped is the form's
// own Spec (espnet.hip) with F_X_STAMP2 on top -- the instantiation the plan's `case` would have launched, whichever of the
// forms below the plan picked -- and only a launch without side sums (F_SIDE1X1 / F_CLS1X1 kernels take no F_X_* flag).
struct StampVariant {
    int variant;
    const char *tag;
    int block;   // the ESP block whose launch is stamped (-1: the class has one launch)
};
template <auto F>
constexpr StampVariant stamp_of{0, nullptr, -1};
template <> constexpr StampVariant stamp_of<form::l3_esp_fused::P2R_VEC>{160, "l3esp", 1};
template <> constexpr StampVariant stamp_of<form::l2_esp_fused::P4_VEC>{161, "l2esp", -1};
template <> constexpr StampVariant stamp_of<form::l2_down::P4S_VEC_SKIP>{162, "l2down", -1};   // the tap-row-chunk form
template <> constexpr StampVariant stamp_of<form::l2_down::P4_VEC>{162, "l2down", -1};
template <> constexpr StampVariant stamp_of<form::l2_esp_last::P4_VEC>{163, "l2last", -1};
template <> constexpr StampVariant stamp_of<form::l3_down::P2R_VEC>{164, "l3down", -1};
template <> constexpr StampVariant stamp_of<form::l3_reduce::BNL>{165, "l3c1s", -1};

template <typename S>
static gs_status launch_stamped(ConvArgs ca, int num_cus, hipStream_t s, const char *tag)
{
    static unsigned long long *stamp = nullptr;
    static int calls = 0;
    // one row per wave the launch can have: a CU holds at most 32 waves (8 per SIMD), whatever the form's occupancy (the tap-row
    // form of the level-2 down-sampler runs four workgroups per CU: 8192 waves on 256 CUs)
    const size_t nw = (size_t)num_cus * 32, nst = nw * STAMP2_SLOTS;
    if (!stamp)
        GS_HIP(hipMalloc(reinterpret_cast<void **>(&stamp), nst * 8));
    GS_HIP(hipMemsetAsync(stamp, 0, nst * 8, s));
    ca.stamp = stamp;
    gs_status st = S::template launch<F_X_STAMP2>(ca, num_cus, s);
    if (st == GS_OK && ++calls == 3) {
        std::vector<unsigned long long> h(nst);
        GS_HIP(hipStreamSynchronize(s));
        GS_HIP(hipMemcpy(h.data(), stamp, nst * 8, hipMemcpyDeviceToHost));
        if (FILE *f = std::fopen(stamp_path("stamps_" + std::string(tag) + ".txt").c_str(), "w")) {
            for (size_t w = 0; w < nw; ++w) {
                if (!h[w * STAMP2_SLOTS]) continue;
                std::fprintf(f, "%zu", w);
                for (int k = 0; k < STAMP2_SLOTS; ++k) std::fprintf(f, " %llu", h[w * STAMP2_SLOTS + k]);
                std::fprintf(f, "\n");
            }
            std::fclose(f);
        }
    }
    return st;
}
// (launch_form's hook: F the form, S its Spec)
#define GS_DIAG_STAMPED(F, S, block)                                                                      \
    if constexpr (stamp_of<F>.variant != 0)                                                               \
        if (m->variant == stamp_of<F>.variant && (stamp_of<F>.block < 0 || stamp_of<F>.block == (block))) \
            return launch_stamped<S>(ca, m->num_cus, s, stamp_of<F>.tag);

// Level-3 branch kernel:
//   101 no epilogue   102 no epilogue, no operand loads   103 ... and no LDS reads   104 no operand loads
//   105 per-wave stamps -> $GS_STAMP_DIR/stamps.txt (tools/stamps.py; results correct)   109 stores but no residual
static gs_status diag_l3_variants(Model *m, ConvArgs ca, int i, hipStream_t s)
{
    switch (m->variant) {
    case 101: return launch_conv_mfma<CFG_L3_BR, F_BNACT | F_RES | F_VEC | F_X_NOEPI>(ca, m->num_cus, s);
    case 102: return launch_conv_mfma<CFG_L3_BR, F_BNACT | F_X_NOEPI | F_X_NOLOAD>(ca, m->num_cus, s);
    case 103: return launch_conv_mfma<CFG_L3_BR, F_BNACT | F_X_NOEPI | F_X_NOLOAD | F_X_NOLDS>(ca, m->num_cus, s);
    case 104: return launch_conv_mfma<CFG_L3_BR, F_BNACT | F_RES | F_X_NOLOAD>(ca, m->num_cus, s);
    case 109: return launch_conv_mfma<CFG_L3_BR, F_BNACT | F_VEC>(ca, m->num_cus, s);
    case 105: {
        static unsigned long long *stamp = nullptr;
        if (!stamp)
            GS_HIP(hipMalloc(reinterpret_cast<void **>(&stamp), 4096 * 8 * 8));
        GS_HIP(hipMemsetAsync(stamp, 0, 4096 * 8 * 8, s));
        ca.stamp = stamp;
        gs_status st = launch_conv_mfma<CFG_L3_BR, F_BNACT | F_RES | F_VEC | POL_L3_ESP | F_X_STAMP>(ca, m->num_cus, s);
        if (i == m->q - 1) {
            std::vector<unsigned long long> h(2048 * 8);
            GS_HIP(hipMemcpy(h.data(), stamp, h.size() * 8, hipMemcpyDeviceToHost));
            if (FILE *f = std::fopen(stamp_path("stamps.txt").c_str(), "w")) {
                for (int w = 0; w < 2048; ++w) {
                    for (int k = 0; k < 7; ++k) std::fprintf(f, "%llu ", h[w * 8 + k]);
                    std::fprintf(f, "\n");
                }
                std::fclose(f);
            }
        }
        return st;
    }
    default: return launch_conv_mfma<CFG_L3_BR, F_BNACT | F_RES>(ca, m->num_cus, s);
    }
}

static bool diag_l3_esp(Model *m, const ConvArgs &ca, int i, hipStream_t s, gs_status &st)
{
    if (m->variant == 0 || (m->variant >= 160 && m->variant <= 169))
        return false;
    st = diag_l3_variants(m, ca, i, s);
    return true;
}
