// The weight packer of an ESPNet handle: a state_dict (fp32 blob + tensor table, include/glomseg.h) -> the ONE float blob the
// kernels read, every piece in the layout its kernel wants, and the float offsets of the pieces.  Every layout decision of the
// weights is made here.  Host-only and free of HIP (espnet_facts.h): gs_espnet_create uploads exactly this blob, the device-free
// entry gs_espnet_pack_weights (include/glomseg_plan.h) returns it to CPU tests, tests/helpers/espnet_setup_driver.cpp runs it
// under sanitizers.
#pragma once
#include <cmath>
#include <cstdio>
#include <cstring>
#include <initializer_list>
#include <map>
#include <string>
#include <vector>

#include "../../include/glomseg_plan.h"
#include "espnet_facts.h"

namespace gs {

struct PackedConv {   // float offsets into the weight blob
    long long c1 = -1, br = -1;
    bool fused_next = false;   // br carries the F_FUSE1X1 table of the following block's c1
};

// float offsets into the weight blob (-1: this model has no such piece), and what of the weights travels as kernel arguments
struct EspnetOffsets {
    long long b2 = -1, b3 = -1, br = -1, wup3 = -1, w3c = -1, cbr0 = -1, wcc = -1, bncc = -1, wup2 = -1, bnu2 = -1, wclassifier = -1;
    long long wtail = -1;      // the fused decoder tail's image (five classes)
    long long wconv = -1;      // the generic decoder tail's conv_mfma image (class counts other than five)
    long long wcc_mfma = -1;   // twelve classes and more: combine_l2_l3.1 as a conv_mfma image (see decode)
    PackedConv l2_0, l3_0;
    std::vector<PackedConv> l2, l3;
    float stem_params[537] = {0};   // level1 weights + folded bn1 + folded b1
};

struct EspnetWeights : EspnetOffsets {
    std::vector<float> blob;
    std::vector<gs_weight_piece> pieces;   // every piece of the blob in order, the tail guard last
};

struct WeightTable {
    const float *blob;
    std::map<std::string, const gs_layer_desc *> by_name;
    bool ok = true;
    const float *get(const std::string &name, std::initializer_list<int> shape)
    {
        auto it = by_name.find(name);
        if (it == by_name.end()) {
            set_error("weight tensor '%s' missing from the table", name.c_str());
            ok = false;
            return nullptr;
        }
        const gs_layer_desc *d = it->second;
        int i = 0;
        bool match = d->ndim == (int)shape.size();
        for (int s : shape)
            match = match && d->shape[i++] == s;
        if (!match) {
            set_error("weight tensor '%s' has the wrong shape", name.c_str());
            ok = false;
            return nullptr;
        }
        return blob + d->offset;
    }
};

struct BlobBuilder {
    std::vector<float> &data;
    std::vector<gs_weight_piece> &pieces;
    long long reserve(const std::string &name, size_t n)
    {
        const size_t at = (data.size() + 3) / 4 * 4;   // 16-byte aligned pieces (float4 LDS staging)
        data.resize(at + (n + 3) / 4 * 4, 0.0f);
        gs_weight_piece pc{};
        std::snprintf(pc.name, sizeof pc.name, "%s", name.c_str());
        pc.offset = (long long)at;
        pc.floats = (long long)(data.size() - at);
        pieces.push_back(pc);
        return (long long)at;
    }
    long long push(const std::string &name, const std::vector<float> &v)
    {
        const long long at = reserve(name, v.size());
        std::memcpy(data.data() + at, v.data(), v.size() * sizeof(float));
        return at;
    }
};

// BatchNorm2d(eps=1e-3).eval() folded to y = x*scale + shift, plus the PReLU slope (1 when `act` is empty):
// layout [scale | shift | alpha][C]; empty when a tensor is missing.  reference: Model.py:21-22,44-45,141-142
static inline std::vector<float> fold_bn(WeightTable &t, const std::string &bn, const std::string &act, int C)
{
    const float *g = t.get(bn + ".weight", {C}), *b = t.get(bn + ".bias", {C});
    const float *m = t.get(bn + ".running_mean", {C}), *v = t.get(bn + ".running_var", {C});
    const float *al = act.empty() ? nullptr : t.get(act + ".weight", {C});
    if (!t.ok)
        return {};
    std::vector<float> dst(3 * (size_t)C);
    for (int c = 0; c < C; ++c) {
        const double inv = 1.0 / std::sqrt((double)v[c] + 1e-3);
        dst[c] = (float)((double)g[c] * inv);
        dst[C + c] = (float)((double)b[c] - (double)m[c] * (double)g[c] * inv);
        dst[2 * C + c] = al ? al[c] : 1.0f;
    }
    return dst;
}

// ... the first `rows` of its rows as [rows][cpn] through `map` (padded index -> source channel or -1): padding planes get scale 0,
// shift 0, slope 1, so they stay exact zeros
template <typename Map>
static inline std::vector<float> fold_bn_mapped(WeightTable &t, const std::string &bn, const std::string &act, int C, int rows, int cpn, Map map)
{
    const std::vector<float> src = fold_bn(t, bn, act, C);
    if (src.empty())
        return {};
    std::vector<float> o((size_t)rows * cpn, 0.0f);
    for (int k = 0; k < cpn; ++k) {
        const int sc = map(k);
        for (int r = 0; r < rows; ++r)
            o[(size_t)r * cpn + k] = sc >= 0 ? src[(size_t)r * C + sc] : (r == 2 ? 1.0f : 0.0f);
    }
    return o;
}

// conv weight [cout][cin][k][k] -> LDS image rows [tap][planes][nrow] of dilation slot `slot`; plane `pl` holds input channel
// map(pl), or stays zero where that is negative
template <typename Map>
static inline void conv_rows_mapped(const float *w, int cout, int cin, int k, float *dst, int slot, int taps, int planes, int nrow, Map map)
{
    for (int tap = 0; tap < taps; ++tap)
        for (int pl = 0; pl < planes; ++pl) {
            const int ci = map(pl);
            if (ci < 0) continue;
            for (int co = 0; co < cout; ++co)
                dst[(((size_t)slot * taps + tap) * planes + pl) * nrow + co] = w[((size_t)co * cin + ci) * k * k + tap];
        }
}
// ... the planes are the input channels, padded to cinp
static inline void pack_conv(const float *w, int cout, int cin, int k, float *dst, int slot, int taps, int cinp, int nrow)
{
    conv_rows_mapped(w, cout, cin, k, dst, slot, taps, cinp, nrow, [&](int pl) { return pl < cin ? pl : -1; });
}

// `next` names the block whose c1 (1x1 reduce of THIS block's output, Model.py:193) is computed in this block's epilogue
// (F_FUSE1X1); empty = no fusion.  `name`: the block's name in the piece table.
static inline bool pack_block(WeightTable &t, BlobBuilder &bb, const std::string &name, const std::string &pre, bool down, int level,
                              PackedConv &pc, const float *dual = nullptr, int dual_coff = 0, int dual_c = 0, const std::string &next = "",
                              const float *in2_bn = nullptr, int in2_c0 = 0, int in2_cn = 0, int in2_c = 0,
                              const float *side_w = nullptr, int side_n = 0)
{
    // level 2: cin 19 (down) / 64, n = 12, n1 = 16;  level 3: cin 131 (down) / 128, n = 25, n1 = 28
    const int n = level == 2 ? 12 : 25, n1 = level == 2 ? 16 : 28, nOut = n1 + 4 * n;
    const int cin = level == 2 ? (down ? 19 : 64) : (down ? 131 : 128);
    const int kl = level == 2 ? 4 : 2;
    const int cinp = (cin + kl - 1) / kl * kl;
    const int taps = down ? 9 : 1;
    const float *wc1 = t.get(pre + ".c1.conv.weight", {n, cin, down ? 3 : 1, down ? 3 : 1});
    if (!t.ok)
        return false;
    const int c1_floats = conv_wfloats(cinp, taps, 1, n, n, false);
    const int bnl_c = cinp + kl;   // F_BNLOAD table: one entry per (padded) input channel + an all-zero slot of one k-group
    // F_SIDE1X1: the class weights [side_n][cin] of a 1x1 over this reduce's input, as [cinp + SIDE_ZROWS][SIDE_REC] behind the table above
    const int side_at = side_table_offset(c1_floats, cinp, kl);
    pc.c1 = bb.reserve(name + ".c1", side_w ? side_at + side_table_floats(cinp) : c1_floats + (in2_bn ? 3 * bnl_c : 0));
    if (side_w)
        for (int ch = 0; ch < cin; ++ch)
            for (int k = 0; k < side_n; ++k)
                bb.data[pc.c1 + side_at + (size_t)ch * SIDE_REC + k] = side_w[(size_t)k * cin + ch];
    pack_conv(wc1, n, cin, down ? 3 : 1, bb.data.data() + pc.c1, 0, taps, cinp, n);
    if (in2_bn) {   // [scale | shift | alpha][bnl_c]: identity, except the cat's BR for the channels that are stored raw
        float *x = bb.data.data() + pc.c1 + c1_floats;
        for (int c = 0; c < bnl_c; ++c) {
            const bool raw = c >= in2_c0 && c < in2_c0 + in2_cn, zero = c >= cinp;
            x[c] = zero ? 0.0f : raw ? in2_bn[c] : 1.0f;
            x[bnl_c + c] = zero ? 0.0f : raw ? in2_bn[in2_c + c] : 0.0f;
            x[2 * bnl_c + c] = raw ? in2_bn[2 * in2_c + c] : 1.0f;
        }
    }

    const int rcinp = (n + kl - 1) / kl * kl;
    const int mt = level == 2 ? 16 : 32, nacc = level == 2 ? 4 : 16;
    pc.fused_next = !next.empty();
    const ConvImage im = conv_image(rcinp, 9, 5, n1, n, true, dual != nullptr, pc.fused_next ? nacc : 0);
    pc.br = bb.reserve(name + ".br", im.total);
    static const char *dn[5] = {".d1", ".d2", ".d4", ".d8", ".d16"};
    for (int di = 0; di < 5; ++di) {
        const int co = di == 0 ? n1 : n;
        const float *w = t.get(pre + dn[di] + ".conv.weight", {co, n, 3, 3});
        if (!t.ok)
            return false;
        pack_conv(w, co, n, 3, bb.data.data() + pc.br, di, 9, rcinp, n1);
    }
    if (pc.fused_next) {
        // table[di][r][lane]: the A operand of the k-step "accumulator register r of slot di": lane = (k-group, c1 output
        // row i); k-group kq of register r holds this block's channel cb + row(r, kq)
        const float *w2 = t.get(next + ".c1.conv.weight", {n, nOut, 1, 1});
        if (!t.ok)
            return false;
        float *tab = bb.data.data() + pc.br + im.w + im.bn;
        for (int di = 0; di < 5; ++di) {
            const int nout = di == 0 ? n1 : n, cb = di == 0 ? 0 : n1 + (di - 1) * n;
            for (int r = 0; r < nacc; ++r)
                for (int lane = 0; lane < 64; ++lane) {
                    const int i = lane % mt, kq = lane / mt;
                    const int row = mt == 32 ? (r & 3) + 8 * (r >> 2) + 4 * kq : kq * 4 + r;
                    tab[(di * nacc + r) * 64 + lane] = (row < nout && i < n) ? w2[(size_t)i * nOut + cb + row] : 0.0f;
                }
        }
    }
    float *bnp = bb.data.data() + pc.br + im.w;
    // DownSamplerB: self.bn / self.act (Model.py:141-142); ESP block: self.bn = BR(nOut) (Model.py:184)
    if (dual)   // slice of the following concat's BR parameters, same [scale | shift | alpha][nOut] layout
        for (int j = 0; j < 3; ++j)
            for (int c = 0; c < nOut; ++c)
                bnp[(3 + j) * nOut + c] = dual[j * dual_c + dual_coff + c];
    const std::vector<float> bn = down ? fold_bn(t, pre + ".bn", pre + ".act", nOut) : fold_bn(t, pre + ".bn.bn", pre + ".bn.act", nOut);
    if (bn.empty())
        return false;
    std::memcpy(bnp, bn.data(), sizeof(float) * 3 * nOut);
    return true;
}

// A state_dict of ESPNet(classes, p, q) -- `encoder_only`: of ESPNet-C, whose tensors carry no "encoder." prefix -- packed into
// out.blob.  The caller has checked classes (2..20), p and q (gs_espnet_create).  A missing or mis-shaped tensor is
// GS_ERR_INVALID, named by gs_last_error.
static inline gs_status pack_espnet_weights(const float *blob, const gs_layer_desc *table, int n_layers, int classes, int p, int q,
                                            bool encoder_only, EspnetWeights &out)
{
    out = EspnetWeights();
    WeightTable t;
    t.blob = blob;
    for (int i = 0; i < n_layers; ++i)
        t.by_name[std::string(table[i].name)] = &table[i];
    const std::string e = encoder_only ? "" : "encoder.";
    const int c = classes, cp = padded_classes(classes);
    BlobBuilder bb{out.blob, out.pieces};
    auto idx = [](const char *s, int i) { return s + std::to_string(i); };

    const float *w;
    std::vector<float> v;
    if (!(w = t.get(e + "level1.conv.weight", {16, 3, 3, 3}))) return GS_ERR_INVALID;
    const long long w1 = bb.push("w1", std::vector<float>(w, w + 432));
    if ((v = fold_bn(t, e + "level1.bn", e + "level1.act", 16)).empty()) return GS_ERR_INVALID;
    const long long bn1 = bb.push("bn1", v);
    if ((v = fold_bn(t, e + "b1.bn", e + "b1.act", 19)).empty()) return GS_ERR_INVALID;
    const long long b1 = bb.push("b1", v);
    std::memcpy(out.stem_params, bb.data.data() + w1, sizeof(float) * 432);
    std::memcpy(out.stem_params + 432, bb.data.data() + bn1, sizeof(float) * 48);
    std::memcpy(out.stem_params + 480, bb.data.data() + b1, sizeof(float) * 57);
    const std::vector<float> b2f = fold_bn(t, e + "b2.bn", e + "b2.act", 131);
    if (b2f.empty()) return GS_ERR_INVALID;
    out.b2 = bb.push("b2", b2f);
    auto next2 = [&](int i) { return l2_c1_fused(i, p) ? e + idx("level2.", i) : std::string(); };
    auto next3 = [&](int i) { return l3_c1_fused(i, q) ? e + idx("level3.", i) : std::string(); };
    // (lazy b2: the down-sampler has no second store, so its image carries no second BN section)
    if (!pack_block(t, bb, "l2_0", e + "level2_0", true, 2, out.l2_0, nullptr, 0, 0, next2(0))) return GS_ERR_INVALID;
    out.l2.resize(p);
    for (int i = 0; i < p; ++i)
        if (!pack_block(t, bb, idx("l2.", i), e + idx("level2.", i), false, 2, out.l2[i], i == p - 1 ? b2f.data() : nullptr, 0, 131, next2(i + 1)))
            return GS_ERR_INVALID;
    // (the reduce of a five-class decoder model also computes level3_C: forward_plan.h, l3c_side_sums)
    const float *w3c = nullptr;
    if (!encoder_only && !(w3c = t.get("level3_C.conv.weight", {c, 131, 1, 1}))) return GS_ERR_INVALID;
    if (!pack_block(t, bb, "l3_0", e + "level3_0", true, 3, out.l3_0, nullptr, 0, 0, next3(0), b2f.data(), 64, 64, 131,
                    l3c_side_sums(cp) ? w3c : nullptr, c))
        return GS_ERR_INVALID;
    out.l3.resize(q);
    for (int i = 0; i < q; ++i)
        if (!pack_block(t, bb, idx("l3.", i), e + idx("level3.", i), false, 3, out.l3[i], nullptr, 0, 0, next3(i + 1))) return GS_ERR_INVALID;

    // ---- decoder: every piece is packed for cp class planes, zero beyond the model's c (espnet_kernels.h, "CLASS COUNTS")
    auto ident = [&](int k) { return k < c ? k : -1; };
    // [rows][cols][2][2] deconvolution weights -> [cp][cp][2][2]
    auto push_deconv = [&](const char *name, const char *tensor, long long &at) {
        const float *src = t.get(tensor, {c, c, 2, 2});
        if (!src) return false;
        std::vector<float> o((size_t)cp * cp * 4, 0.0f);
        for (int i = 0; i < c; ++i)
            for (int o2 = 0; o2 < c; ++o2)
                for (int k = 0; k < 4; ++k)
                    o[((size_t)i * cp + o2) * 4 + k] = src[((size_t)i * c + o2) * 4 + k];
        at = bb.push(name, o);
        return true;
    };
    auto push_bn = [&](const char *name, const std::string &bn, const std::string &act, int C, int rows, int cpn, auto map, long long &at) {
        const std::vector<float> o = fold_bn_mapped(t, bn, act, C, rows, cpn, map);
        if (o.empty()) return false;
        at = bb.push(name, o);
        return true;
    };
    const std::vector<float> b3f = fold_bn(t, e + "b3.bn", e + "b3.act", 256);
    if (b3f.empty()) return GS_ERR_INVALID;
    if (!(w = t.get(e + "classifier.conv.weight", {c, 256, 1, 1}))) return GS_ERR_INVALID;
    {
        const int rec = (3 + cp + 3) / 4 * 4;   // dec1_record<cp>
        std::vector<float> pk((size_t)256 * rec, 0.0f);   // [channel][scale, shift, alpha, w0..]
        for (int ch = 0; ch < 256; ++ch) {
            for (int j = 0; j < 3; ++j) pk[(size_t)ch * rec + j] = b3f[j * 256 + ch];
            for (int k = 0; k < c; ++k) pk[(size_t)ch * rec + 3 + k] = w[k * 256 + ch];
        }
        out.b3 = bb.push("b3", pk);
    }
    if (!encoder_only) {
        if (!push_bn("br", "br", "", c, 2, cp, ident, out.br)) return GS_ERR_INVALID;
        if (!push_deconv("wup3", "up_l3.0.weight", out.wup3)) return GS_ERR_INVALID;
        {
            const int rec = (cp + 3) / 4 * 4;   // dec2_record<cp>
            std::vector<float> pk((size_t)131 * rec, 0.0f);
            for (int ch = 0; ch < 131; ++ch)
                for (int k = 0; k < c; ++k) pk[(size_t)ch * rec + k] = w3c[k * 131 + ch];
            out.w3c = bb.push("w3c", pk);
        }
        // combine_l2_l3: cat([level3_C out, up_l3 out]) (Model.py:373) lives in 2 * cp planes, each half padded on its own
        auto cat2 = [&](int k) { return k < cp ? (k < c ? k : -1) : (k - cp < c ? c + k - cp : -1); };
        if (!push_bn("cbr0", "combine_l2_l3.0.bn", "combine_l2_l3.0.act", 2 * c, 3, 2 * cp, cat2, out.cbr0)) return GS_ERR_INVALID;
        if (!(w = t.get("combine_l2_l3.1.conv.weight", {c, 2 * c, 3, 3}))) return GS_ERR_INVALID;
        {
            std::vector<float> o((size_t)cp * 2 * cp * 9, 0.0f);
            for (int k = 0; k < c; ++k)
                for (int ch = 0; ch < 2 * cp; ++ch) {
                    const int sc = cat2(ch);
                    if (sc < 0) continue;
                    for (int tap = 0; tap < 9; ++tap)   // (five classes: the reference's own order; else [plane][tap][class], see Dec3Args)
                        o[cp == 5 ? ((size_t)k * 2 * cp + ch) * 9 + tap : ((size_t)ch * 9 + tap) * cp + k] = w[((size_t)k * 2 * c + sc) * 9 + tap];
                }
            out.wcc = bb.push("wcc", o);
        }
        if (dec3_on_mfma(cp)) {   // the same convolution as a conv_mfma image: [tap][2 * cp planes][cp rows], then its folded BN + PReLU
            out.wcc_mfma = bb.reserve("wcc_mfma", conv_wfloats(2 * cp, 9, 1, cp, cp, true));
            conv_rows_mapped(w, c, 2 * c, 3, bb.data.data() + out.wcc_mfma, 0, 9, 2 * cp, cp, cat2);
        }
        if (!push_bn("bncc", "combine_l2_l3.1.bn", "combine_l2_l3.1.act", c, 3, cp, ident, out.bncc)) return GS_ERR_INVALID;
        if (out.wcc_mfma >= 0)
            std::memcpy(bb.data.data() + out.wcc_mfma + (size_t)9 * 2 * cp * cp, bb.data.data() + out.bncc, sizeof(float) * 3 * cp);
        if (!push_deconv("wup2", "up_l2.0.weight", out.wup2)) return GS_ERR_INVALID;
        if (!push_bn("bnu2", "up_l2.1.bn", "up_l2.1.act", c, 3, cp, ident, out.bnu2)) return GS_ERR_INVALID;
        const float *wc = t.get("conv.conv.weight", {c, 19 + c, 3, 3});
        if (!wc) return GS_ERR_INVALID;
        const std::vector<float> bn_conv = fold_bn_mapped(t, "conv.bn", "conv.act", c, 3, cp, ident);
        if (bn_conv.empty()) return GS_ERR_INVALID;
        if (!dec_tail_fused(cp)) {   // (five classes: dec_tail reads wtail, packed below)
            // the generic tail's conv_mfma image [tap][CINP planes][cp rows] + BN: CINP = 19 + cp rounded up to the k-step.  Plane
            // `pl` of the concat buffer [comb_l2_l3 (cp planes) | output0_cat (19) | zero planes] <-> channel of the reference's
            // torch.cat([comb_l2_l3, output0_cat]) (Model.py:375)
            auto cat_ch = [&](int pl) { return pl < cp ? (pl < c ? pl : -1) : (pl - cp < 19 ? c + pl - cp : -1); };
            const int cinp = (19 + cp + 3) / 4 * 4;
            out.wconv = bb.reserve("wconv", conv_wfloats(cinp, 9, 1, cp, cp, true));
            float *dst = bb.data.data() + out.wconv;
            conv_rows_mapped(wc, c, 19 + c, 3, dst, 0, 9, cinp, cp, cat_ch);
            std::memcpy(dst + (size_t)9 * cinp * cp, bn_conv.data(), sizeof(float) * 3 * cp);
        }
        if (!push_deconv("wclassifier", "classifier.weight", out.wclassifier)) return GS_ERR_INVALID;
        if (dec_tail_fused(cp)) {
            // dec_tail image: A operands [ty][plane group][lane] (lane = k-group * 16 + MFMA row, row = tx*c + o),
            // then BN scale / shift / alpha of conv, then classifier.weight
            out.wtail = bb.reserve("wtail", DT_PACK_FLOATS);
            float *dt = bb.data.data() + out.wtail;
            for (int ty = 0; ty < 3; ++ty)
                for (int g = 0; g < 6; ++g)
                    for (int lane = 0; lane < 64; ++lane) {
                        const int rho = lane & 15, ch = 4 * g + (lane >> 4);
                        dt[(ty * 6 + g) * 64 + lane] =
                            rho < 3 * c ? wc[(((size_t)(rho % c) * (19 + c) + ch) * 3 + ty) * 3 + rho / c] : 0.0f;
                    }
            std::memcpy(dt + DT_A_FLOATS, bn_conv.data(), sizeof(float) * 3 * c);
            std::memcpy(dt + DT_A_FLOATS + 16, bb.data.data() + out.wclassifier, sizeof(float) * c * c * 4);   // (cp == c: no padding in it)
        }
    }
    bb.reserve("guard", 512);   // tail guard: LDS-DMA staging reads whole 1-KiB pieces
    return GS_OK;
}

}  // namespace gs
