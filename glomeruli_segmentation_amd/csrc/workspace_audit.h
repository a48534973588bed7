// Which words of a lane's activation workspace (workspace_plan.h) a forward may write, and which must stay the zeros
// layout_workspace put there.  Every convolution takes its padding from the second kind (espnet_facts.h, struct Act): a
// store that runs past a row end, into a plane tail, a padding plane or the slack is invisible in the forward that makes it
// and wrong in the next one at the same shape.  Host-only and free of HIP, like workspace_plan.h: the audit and the poison
// entries of include/glomseg_workspace.h (test tools) and a CPU test read the same runs.
//
// A piece is one of the WS_PIECES activations with storage of their own, in allocation order; its span runs from its first
// byte to the first byte of the next piece (the allocation's end for the last).  Every float of a span is one of
//   WS_INTERIOR      planes < C, rows < H, columns < W of images < ws_n: what kernels write
//   WS_MUST_BE_ZERO  * of a PADDED piece (one that plan_workspace gives a halo or Cp > C: a0c, r2[*], a1, r3[*], and tt when
//                      dec3 runs on the matrix cores) everything else inside ws_n * sn: the four halos, the pitch tail, the
//                      + 96 plane tail, the padding planes -- and the CLASS PLANES BEYOND THE MODEL'S COUNT where a convolution
//                      on the matrix cores reads them: the decoder kernels are instantiated for the padded count cp and their
//                      stores stop at the model's `classes` (espnet_kernels.h, "CLASS COUNTS"), so with classes < cp planes
//                      classes..cp-1 of a0c (comb_l2_l3, read by the decoder's last 3x3) and, when dec3 runs on the matrix
//                      cores, planes k of tt with k % cp >= classes are written by nothing and read as zeros: a non-finite
//                      value there would survive the zero weight, exactly as in a padding plane
//                    * of every piece, the span behind bytes(ws_n): WS_SLACK and the 256-byte rounding.  Under lazy b2 the
//                      piece bb[0] is a view of a1 and its span is slack alone
//   WS_FREE          the rest: pitch tails and plane tails of the halo-less pieces.  Nothing reads them as padding, and other
//                    layouts may use them (the dense class-sum planes parked in tt)
// The views (ee, a0, lazy bb[0]) add nothing: their words are classified by the piece whose storage they are.
// The same planes of the pieces whose readers re-zero the padding lanes on load (o2c, t3, ff, tt under dec3_kernel:
// zero_padding_lanes, espnet_kernels.h) are interior: nothing takes them as padding.
// Exemptions (words of the set that a kernel legitimately writes): none.
#pragma once
#include <cstdint>
#include <cstring>

#include "workspace_plan.h"

namespace gs {

enum WsClass : unsigned char { WS_FREE = 0, WS_INTERIOR = 1, WS_MUST_BE_ZERO = 2 };

constexpr const char *kWsPieceNames[WS_PIECES] = {"a0c", "inp1", "inp2", "r2[0]", "r2[1]", "bb[0]", "bb[1]", "bb[2]", "a1", "r3[0]",
                                                  "r3[1]", "cc[0]", "cc[1]", "cc[2]", "o2c", "l3c", "tt", "t3", "ff"};

struct WsPiece {
    const char *name = nullptr;
    Act act;              // base null
    size_t at = 0;        // byte offset of the span in the allocation
    size_t own_words = 0; // ws_n * sn, or 0 for a piece without storage (lazy bb[0])
    size_t span_words = 0;
    bool padded = false;
    int cls_planes = 0, cp = 1, classes = 1;   // planes c < cls_planes with c % cp >= classes: class planes no kernel writes
    bool dead_plane(int c) const { return c < cls_planes && c % cp >= classes; }
};

// A halo on the top, the left or the bottom, or padding planes.  (Act keeps no pad_r; plan_workspace gives no piece a right
// halo alone.)
inline bool ws_is_padded(const Act &a) { return a.off != 0 || a.Cp > a.C || a.sc != a.H * a.pitch + 96; }

// piece i of a plan laid out for ws_n images (the n plan_workspace was called with) of a model of `classes` classes
inline WsPiece ws_piece(WorkspacePlan &plan, int ws_n, int i, int classes)
{
    const std::array<Act *, WS_ACTS> all = acts_of(plan.acts);
    size_t cum = 0, next = 0;
    bool own = true;
    for (int k = 0; k <= i; ++k) {   // plan_workspace's own sum: a view's `at` points into another piece, its span does not
        own = plan.at[k] == next;
        cum = next;
        next = cum + (size_t)round_up((own ? all[k]->bytes(ws_n) : 0) + WS_SLACK, 256);
    }
    WsPiece pc;
    pc.name = kWsPieceNames[i];
    pc.act = *all[i];
    pc.at = cum;
    pc.own_words = own ? (size_t)ws_n * (size_t)pc.act.sn : 0;
    pc.span_words = (next - cum) / sizeof(float);
    pc.padded = own && ws_is_padded(pc.act);
    const int cp = padded_classes(classes);
    const bool a0c = all[i] == &plan.acts.a0c, tt = all[i] == &plan.acts.tt && dec3_on_mfma(cp);
    if (a0c || tt)
        pc.cls_planes = a0c ? cp : 2 * cp, pc.cp = cp, pc.classes = classes;
    return pc;
}

// fn(class, first word, end word) for every run of the span, ascending and gap-free
template <typename F>
inline void ws_for_each_run(const WsPiece &pc, F &&fn)
{
    const Act &a = pc.act;
    const WsClass other = pc.padded ? WS_MUST_BE_ZERO : WS_FREE;
    size_t w = 0;
    if (pc.own_words) {
        const size_t images = pc.own_words / (size_t)a.sn;
        for (size_t n = 0; n < images; ++n) {
            for (int c = 0; c < a.Cp; ++c) {
                const size_t plane = n * (size_t)a.sn + (size_t)c * a.sc, end = plane + a.sc;
                if (c < a.C && !pc.dead_plane(c)) {
                    for (int y = 0; y < a.H; ++y) {
                        const size_t row = plane + a.off + (size_t)y * a.pitch;
                        if (row > w) fn(other, w, row);
                        fn(WS_INTERIOR, row, row + a.W);
                        w = row + a.W;
                    }
                }
                fn(other, w, end);
                w = end;
            }
        }
    }
    if (pc.span_words > w) fn(WS_MUST_BE_ZERO, w, pc.span_words);
}

struct WsWhere {
    int image, plane, row, col;
};
// Where word w of the span lies: row and column relative to the interior origin (a left halo has col < 0, a pitch tail
// col >= W, a top halo row < 0, the bottom halo and the + 96 tail row >= H).  A word of the slack: image = the images of the
// piece, plane = row = 0, col = its distance from the slack's first word.
inline WsWhere ws_where(const WsPiece &pc, size_t w)
{
    const Act &a = pc.act;
    if (w >= pc.own_words)
        return {pc.own_words ? (int)(pc.own_words / (size_t)a.sn) : 0, 0, 0, (int)(w - pc.own_words)};
    const size_t r = w % (size_t)a.sn % (size_t)a.sc;
    return {(int)(w / (size_t)a.sn), (int)(w % (size_t)a.sn / (size_t)a.sc), (int)(r / a.pitch) - a.off / a.pitch,
            (int)(r % a.pitch) - a.off % a.pitch};
}

struct WsReport {   // (gs_workspace_report of include/glomseg_workspace.h, field for field)
    long long must_be_zero = 0, offenders = 0;
    char piece[16] = {0};
    int image = 0, plane = 0, row = 0, col = 0;
    unsigned int bits = 0;
};

// adds the must-be-zero words of one span (`words`: its host copy) to the report; the first offender is the first in
// allocation order when the pieces are given in that order
inline void ws_audit_piece(const WsPiece &pc, const uint32_t *words, WsReport &rep)
{
    ws_for_each_run(pc, [&](WsClass cls, size_t b, size_t e) {
        if (cls != WS_MUST_BE_ZERO) return;
        rep.must_be_zero += (long long)(e - b);
        for (size_t w = b; w < e; ++w) {
            if (words[w] == 0) continue;
            if (rep.offenders++ == 0) {
                const WsWhere at = ws_where(pc, w);
                std::strncpy(rep.piece, pc.name, sizeof rep.piece - 1);
                rep.image = at.image, rep.plane = at.plane, rep.row = at.row, rep.col = at.col;
                rep.bits = words[w];
            }
        }
    });
}

// overwrites every interior and free word of a span's host copy with the pattern
inline void ws_poison_piece(const WsPiece &pc, uint32_t *words, uint32_t pattern)
{
    ws_for_each_run(pc, [&](WsClass cls, size_t b, size_t e) {
        if (cls == WS_MUST_BE_ZERO) return;
        for (size_t w = b; w < e; ++w) words[w] = pattern;
    });
}

inline void ws_class_map(const WsPiece &pc, unsigned char *map)
{
    ws_for_each_run(pc, [&](WsClass cls, size_t b, size_t e) { std::memset(map + b, cls, e - b); });
}

}  // namespace gs
