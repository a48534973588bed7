// The activation workspace of one lane of an ESPNet handle: which activations a forward of n tiles of H x W needs, their halos,
// pitches and plane strides, where each lies in ONE allocation, and how many bytes that is.  plan_workspace decides,
// layout_workspace (espnet.hip) allocates, zeroes and adds the base pointer.  Host-only and free of HIP (espnet_facts.h):
// gs_espnet_workspace_plan (include/glomseg_plan.h) answers "how much memory will this shape take" without a device.
#pragma once
#include <array>

#include "espnet_facts.h"

namespace gs {

struct Workspace {
    Act a0c, a0, inp1, inp2, r2[2], bb[3], a1, r3[2], cc[3], o2c, l3c, tt, t3, ee, ff;
};
constexpr int WS_PIECES = 19, WS_ACTS = 21;
// the activations with storage of their own in allocation order (bb[0] has none under lazy b2: it is a view then), then the
// views ee and a0
inline std::array<Act *, WS_ACTS> acts_of(Workspace &m)
{
    return {&m.a0c, &m.inp1, &m.inp2, &m.r2[0], &m.r2[1], &m.bb[0], &m.bb[1], &m.bb[2], &m.a1, &m.r3[0], &m.r3[1],
            &m.cc[0], &m.cc[1], &m.cc[2], &m.o2c, &m.l3c, &m.tt, &m.t3, &m.ff, &m.ee, &m.a0};
}

struct WorkspacePlan {
    Workspace acts;            // every base is null: ...
    size_t at[WS_ACTS] = {};   // ... the byte offset of acts_of(acts)[i]'s base in the allocation
    size_t bytes = 0;          // the allocation
};
constexpr size_t WS_SLACK = 64 * 1024;   // behind every piece: strips may over-read past a buffer's last row (masked lanes only)

inline Act make_act(int C, int Cp, int H, int W, int pad_t, int pad_b, int pad_l, int pad_r)
{
    Act a;
    a.C = C;
    a.Cp = Cp;
    a.H = H;
    a.W = W;
    a.pitch = (int)round_up(pad_l + W + pad_r, 32);   // 128-byte rows: interior stores stay line-aligned
    // + 96 floats: a plane stride that is a power of two (8192 floats at 1/8 scale) lands every channel of a
    // pixel on the same HBM channel / L2 slice when a kernel walks the channels (dec1, the 1x1 reduces)
    a.sc = (pad_t + H + pad_b) * a.pitch + 96;
    a.off = pad_t * a.pitch + pad_l;
    a.sn = (long long)Cp * a.sc;
    return a;
}

// cls: the padded class planes (the planes beyond the model's classes stay zero); H and W: multiples of 8 (check_shape)
inline gs_status plan_workspace(int n, int H, int W, int cls, int p, bool encoder_only, WorkspacePlan &out)
{
    out = WorkspacePlan();
    Workspace *m = &out.acts;
    const int H1 = H / 2, W1 = W / 2, H2 = H / 4, W2 = W / 4, H3 = H / 8, W3 = W / 8;
    // comb_l2_l3 (planes 0..cls-1, written by dec3) and output0_cat (planes cls..cls+18, written by the stem) share one
    // buffer in the order of the decoder's torch.cat (Model.py:375), so conv CBR(19+classes, classes, 3) reads its input as
    // ONE 24-plane activation with zero pad on all four sides.  Plane cls+19 is never written: the level-2 strided reduce
    // reads output0_cat padded to 20 channels (a multiple of the k-step) and its padding plane must be zeros, not a
    // plane some other stage writes (a non-finite value there would survive the zero weight).
    m->a0c = make_act(cls + 19, cls + 20, H1, W1, 1, 1, 32, 1);
    m->inp1 = make_act(3, 3, H1, W1, 0, 0, 0, 0);
    m->inp2 = make_act(3, 3, H2, W2, 0, 0, 0, 0);
    for (int i = 0; i < 2; ++i)   // two reduced maps: a block reads one while its epilogue writes the next block's
        m->r2[i] = make_act(12, 12, H2, W2, 16, 16, 32, 16);  // dilation up to 16
    for (int i = 0; i < 3; ++i)
        m->bb[i] = make_act(64, 64, H2, W2, 0, 0, 0, 0);
    m->a1 = make_act(131, 132, H2, W2, 1, 0, 32, 1);
    for (int i = 0; i < 2; ++i)
        m->r3[i] = make_act(25, 26, H3, W3, 16, 16, 32, 16);
    for (int i = 0; i < 3; ++i)
        m->cc[i] = make_act(128, 128, H3, W3, 0, 0, 0, 0);
    m->o2c = make_act(cls, cls, H2, W2, 0, 0, 0, 0);
    // level3_C's raw output, written by the stride-2 reduce (F_SIDE1X1) when the plan says so; else a token buffer
    m->l3c = !encoder_only && l3c_side_sums(cls) ? make_act(cls, cls, H2, W2, 0, 0, 0, 0) : make_act(1, 1, 8, 8, 0, 0, 0, 0);
    // (twelve classes and more: combine_l2_l3.1's 3x3 runs on the matrix cores and reads its input with a zero halo; t3 is its output)
    const bool dec3_mfma = dec3_on_mfma(cls);
    m->tt = dec3_mfma ? make_act(2 * cls, 2 * cls, H2, W2, 1, 1, 32, 1) : make_act(2 * cls, 2 * cls, H2, W2, 0, 0, 0, 0);
    m->t3 = dec3_mfma ? make_act(cls, cls, H2, W2, 0, 0, 0, 0) : make_act(1, 1, 8, 8, 0, 0, 0, 0);
    m->ff = make_act(cls, cls, H1, W1, 0, 0, 0, 0);
    // Lazy b2 (p > 0): output1_0 is stored RAW, once, straight into planes 64..127 of output1_cat -- bb[0] becomes a view of
    // them -- and the consumers of output1_cat apply b2 to those planes on load (espnet_config.h, "Lazy b2").
    const bool lazy_b2 = b2_is_lazy(p);
    if (lazy_b2)
        m->bb[0] = Act();   // no storage of its own
    const std::array<Act *, WS_ACTS> all = acts_of(*m);
    for (int i = 0; i < WS_PIECES; ++i) {   // kernels address one image with 32-bit byte offsets (buffer soffset / voffset)
        if ((unsigned long long)all[i]->sn * sizeof(float) >= (1ull << 31)) {
            set_error("tile %dx%d is too large: an activation of one image exceeds 2 GiB", H, W);
            return GS_ERR_UNSUPPORTED;
        }
    }
    auto at_of = [&](const Act *a) -> size_t & {
        int i = 0;
        while (all[i] != a) ++i;
        return out.at[i];
    };
    for (int i = 0; i < WS_PIECES; ++i) {
        out.at[i] = out.bytes;
        out.bytes += round_up(all[i]->bytes(n) + WS_SLACK, 256);
    }
    if (lazy_b2) {
        m->bb[0] = m->a1;
        at_of(&m->bb[0]) = at_of(&m->a1) + (size_t)64 * m->a1.sc * sizeof(float);
        m->bb[0].C = 64;
        m->bb[0].Cp = 64;
    }
    m->ee = m->a0c;   // comb_l2_l3 = the first planes of the concat buffer
    at_of(&m->ee) = at_of(&m->a0c);
    m->ee.C = cls;
    m->a0 = m->a0c;   // output0_cat = the planes after it (+ the zero plane)
    at_of(&m->a0) = at_of(&m->a0c) + (size_t)cls * m->a0c.sc * sizeof(float);
    m->a0.C = 19;
    return GS_OK;
}

}  // namespace gs
