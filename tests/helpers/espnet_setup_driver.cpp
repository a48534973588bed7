// Sanitizer driver (tests/test_espnet_setup.py) for the host-only set-up of an ESPNet handle: the weight packer
// (csrc/espnet_weights.h) and the activation layout (csrc/workspace_plan.h).  Packs a random state_dict for every class count
// 2..20, p and q in 0..3 and both handle kinds -- the tensors lie in one blob with poisoned gaps between them, so that
// AddressSanitizer sees a read past the end of any tensor as well as a write past the packed blob -- and checks every
// workspace plan for the invariants the forward relies on.  Built with g++ only: no HIP in here.
#include <cmath>
#include <cstdarg>
#include <cstdio>
#include <cstring>
#include <random>
#include <string>
#include <vector>

#if defined(__SANITIZE_ADDRESS__)
#include <sanitizer/asan_interface.h>
#else
#define ASAN_POISON_MEMORY_REGION(a, n) ((void)(a), (void)(n))
#define ASAN_UNPOISON_MEMORY_REGION(a, n) ((void)(a), (void)(n))
#endif

#include "espnet_weights.h"
#include "workspace_plan.h"

namespace gs {
static char g_err[1024];
void set_error(const char *fmt, ...)
{
    va_list ap;
    va_start(ap, fmt);
    std::vsnprintf(g_err, sizeof g_err, fmt, ap);
    va_end(ap);
}
}  // namespace gs
using namespace gs;

static int fail(const char *what, int a, int b, int c)
{
    std::fprintf(stderr, "FAILED: %s (%d, %d, %d): %s\n", what, a, b, c, g_err);
    return 1;
}

// the tensors of ESPNet(classes, p, q) (Model.py:242-339), ESPNet-C's without the "encoder." prefix and without the decoder
struct StateDict {
    static constexpr size_t GAP = 16;   // floats between two tensors, poisoned
    std::vector<float> blob;
    std::vector<gs_layer_desc> table;
    std::mt19937 rng{12345};
    void add(const std::string &name, std::initializer_list<int> shape, float lo, float hi)
    {
        gs_layer_desc d{};
        std::snprintf(d.name, sizeof d.name, "%s", name.c_str());
        size_t n = 1;
        for (int s : shape) d.shape[d.ndim++] = s, n *= (size_t)s;
        d.offset = (long long)blob.size();
        std::uniform_real_distribution<float> u(lo, hi);
        for (size_t i = 0; i < n; ++i) blob.push_back(u(rng));
        blob.resize((blob.size() + GAP + 1) / 2 * 2, 0.0f);   // (8-byte granules: the next tensor starts on one)
        table.push_back(d);
    }
    void bn(const std::string &name, int c)
    {
        add(name + ".weight", {c}, 0.5f, 1.5f), add(name + ".bias", {c}, -0.1f, 0.1f);
        add(name + ".running_mean", {c}, -0.1f, 0.1f), add(name + ".running_var", {c}, 0.5f, 1.5f);
    }
    void block(const std::string &pre, int cin, int cout, bool down)
    {
        const int n = cout / 5, n1 = cout - 4 * n, k = down ? 3 : 1;
        add(pre + ".c1.conv.weight", {n, cin, k, k}, -0.3f, 0.3f);
        add(pre + ".d1.conv.weight", {n1, n, 3, 3}, -0.3f, 0.3f);
        for (int d : {2, 4, 8, 16}) add(pre + ".d" + std::to_string(d) + ".conv.weight", {n, n, 3, 3}, -0.3f, 0.3f);
        bn(pre + (down ? ".bn" : ".bn.bn"), cout), add(pre + (down ? ".act" : ".bn.act") + ".weight", {cout}, 0.05f, 0.4f);
    }
    StateDict(int c, int p, int q, bool encoder_only)
    {
        const std::string e = encoder_only ? "" : "encoder.";
        add(e + "level1.conv.weight", {16, 3, 3, 3}, -0.3f, 0.3f), bn(e + "level1.bn", 16), add(e + "level1.act.weight", {16}, 0.05f, 0.4f);
        bn(e + "b1.bn", 19), add(e + "b1.act.weight", {19}, 0.05f, 0.4f);
        block(e + "level2_0", 19, 64, true);
        for (int i = 0; i < p; ++i) block(e + "level2." + std::to_string(i), 64, 64, false);
        bn(e + "b2.bn", 131), add(e + "b2.act.weight", {131}, 0.05f, 0.4f);
        block(e + "level3_0", 131, 128, true);
        for (int i = 0; i < q; ++i) block(e + "level3." + std::to_string(i), 128, 128, false);
        bn(e + "b3.bn", 256), add(e + "b3.act.weight", {256}, 0.05f, 0.4f);
        add(e + "classifier.conv.weight", {c, 256, 1, 1}, -0.3f, 0.3f);
        if (!encoder_only) {
            add("level3_C.conv.weight", {c, 131, 1, 1}, -0.3f, 0.3f), bn("br", c);
            add("conv.conv.weight", {c, 19 + c, 3, 3}, -0.3f, 0.3f), bn("conv.bn", c), add("conv.act.weight", {c}, 0.05f, 0.4f);
            add("up_l3.0.weight", {c, c, 2, 2}, -0.4f, 0.4f);
            bn("combine_l2_l3.0.bn", 2 * c), add("combine_l2_l3.0.act.weight", {2 * c}, 0.05f, 0.4f);
            add("combine_l2_l3.1.conv.weight", {c, 2 * c, 3, 3}, -0.3f, 0.3f), bn("combine_l2_l3.1.bn", c);
            add("combine_l2_l3.1.act.weight", {c}, 0.05f, 0.4f);
            add("up_l2.0.weight", {c, c, 2, 2}, -0.4f, 0.4f), bn("up_l2.1.bn", c), add("up_l2.1.act.weight", {c}, 0.05f, 0.4f);
            add("classifier.weight", {c, c, 2, 2}, -0.4f, 0.4f);
        }
        poison(true);
    }
    ~StateDict() { poison(false); }
    void poison(bool on)
    {
        for (size_t i = 0; i < table.size(); ++i) {
            size_t n = 1;
            for (int d = 0; d < table[i].ndim; ++d) n *= (size_t)table[i].shape[d];
            const size_t end = (size_t)table[i].offset + n, next = i + 1 < table.size() ? (size_t)table[i + 1].offset : blob.size();
            if (on)
                ASAN_POISON_MEMORY_REGION(blob.data() + end, (next - end) * sizeof(float));
            else
                ASAN_UNPOISON_MEMORY_REGION(blob.data() + end, (next - end) * sizeof(float));
        }
    }
};

static int check_weights(int c, int p, int q, bool enc)
{
    StateDict sd(c, p, q, enc);
    EspnetWeights w;
    if (pack_espnet_weights(sd.blob.data(), sd.table.data(), (int)sd.table.size(), c, p, q, enc, w) != GS_OK)
        return fail("pack_espnet_weights refused a complete table", c, p, q);
    long long at = 0;
    for (const gs_weight_piece &pc : w.pieces) {   // the pieces tile the blob, each on a multiple of four floats
        if (pc.offset != at || pc.offset % 4 || pc.floats <= 0 || pc.floats % 4)
            return fail(pc.name, c, p, q);
        at += pc.floats;
    }
    if (at != (long long)w.blob.size() || w.pieces.empty() || w.pieces.back().floats != 512)
        return fail("the pieces do not end with the blob and its guard", c, p, q);
    for (size_t i = 0; i < w.blob.size(); ++i)
        if (!std::isfinite(w.blob[i]) || (i >= w.blob.size() - 512 && w.blob[i] != 0.0f))
            return fail("a value that is not finite, or a guard float that is not zero", c, p, q);
    const long long must[] = {w.b2, w.b3, w.l2_0.c1, w.l2_0.br, w.l3_0.c1, w.l3_0.br};
    for (long long o : must)
        if (o < 0) return fail("an offset every model has was left unset", c, p, q);
    if ((int)w.l2.size() != p || (int)w.l3.size() != q || (w.wtail >= 0) != (!enc && c == 5) || (w.wconv >= 0) != (!enc && c != 5) ||
        (w.wcc_mfma >= 0) != (!enc && c > 8) || (w.br >= 0) != !enc)
        return fail("the offsets do not match the model", c, p, q);
    // a table without one tensor, and one with a tensor of another shape, are refused by name
    std::vector<gs_layer_desc> cut(sd.table.begin() + 1, sd.table.end());
    if (pack_espnet_weights(sd.blob.data(), cut.data(), (int)cut.size(), c, p, q, enc, w) != GS_ERR_INVALID || !std::strstr(g_err, sd.table[0].name))
        return fail("a missing tensor was not refused by name", c, p, q);
    std::vector<gs_layer_desc> bent = sd.table;
    bent.back().shape[0] += 1;
    if (pack_espnet_weights(sd.blob.data(), bent.data(), (int)bent.size(), c, p, q, enc, w) != GS_ERR_INVALID || !std::strstr(g_err, bent.back().name))
        return fail("a mis-shaped tensor was not refused by name", c, p, q);
    return 0;
}

static int check_workspace(int n, int H, int W, int c, int p, bool enc)
{
    const int cp = padded_classes(c);
    WorkspacePlan pl;
    if (plan_workspace(n, H, W, cp, p, enc, pl) != GS_OK)
        return fail("plan_workspace refused a small shape", H, W, c);
    const auto acts = acts_of(pl.acts);
    const bool lazy = b2_is_lazy(p);
    const Workspace &m = pl.acts;
    auto at = [&](const Act *a) {
        int i = 0;
        while (acts[i] != a) ++i;
        return pl.at[i];
    };
    size_t end = 0;   // the pieces in allocation order: 256-byte aligned, one behind the other with the slack in between, inside the total
    for (int i = 0; i < WS_PIECES; ++i) {
        if (lazy && acts[i] == &m.bb[0]) continue;   // a view
        if (acts[i]->base || pl.at[i] % 256 || pl.at[i] < end)
            return fail("a piece is misaligned or overlaps the one before it", i, H, W);
        end = pl.at[i] + acts[i]->bytes(n) + WS_SLACK;
        if (end > pl.bytes)
            return fail("a piece and its slack do not lie inside the total", i, H, W);
        const Act &a = *acts[i];   // every pixel of the last image's last plane, halo included, lies inside the piece
        if (a.Cp < a.C || a.sn != (long long)a.Cp * a.sc || a.pitch % 32 || a.pitch < a.W ||
            (long long)a.off + (long long)(a.H - 1) * a.pitch + a.W > a.sc)
            return fail("an activation's geometry is inconsistent", i, H, W);
    }
    if (lazy && (at(&m.bb[0]) != at(&m.a1) + (size_t)64 * m.a1.sc * sizeof(float) || m.bb[0].C != 64 || m.bb[0].Cp != 64 ||
                 m.bb[0].sc != m.a1.sc || m.bb[0].sn != m.a1.sn || m.bb[0].pitch != m.a1.pitch || m.bb[0].off != m.a1.off))
        return fail("the lazy-b2 view is not plane 64 of a1", n, H, W);
    if (!lazy && (m.bb[0].C != 64 || m.bb[0].sn != m.bb[1].sn))
        return fail("bb[0] has no storage of its own without lazy b2", n, H, W);
    if (at(&m.ee) != at(&m.a0c) || m.ee.C != cp || m.ee.sc != m.a0c.sc || m.ee.sn != m.a0c.sn || m.ee.off != m.a0c.off)
        return fail("ee is not planes 0..cp-1 of the concat buffer", n, H, W);
    if (at(&m.a0) != at(&m.a0c) + (size_t)cp * m.a0c.sc * sizeof(float) || m.a0.C != 19 || m.a0c.Cp != cp + 20 || m.a0.sc != m.a0c.sc ||
        m.a0.sn != m.a0c.sn || m.a0.off != m.a0c.off)
        return fail("a0 is not the planes cp..cp+18 behind ee", n, H, W);
    return 0;
}

int main()
{
    int packs = 0, plans = 0;
    for (int c = 2; c <= 20; ++c)
        for (int enc = 0; enc < 2; ++enc)
            for (int p = 0; p <= 3; ++p) {
                for (int q = 0; q <= 3; ++q, ++packs)
                    if (check_weights(c, p, q, enc != 0)) return 1;
                for (int H : {8, 64, 520})
                    for (int W : {8, 64, 520})
                        for (int n : {1, 3}) {
                            if (check_workspace(n, H, W, c, p, enc != 0)) return 1;
                            ++plans;
                        }
            }
    WorkspacePlan pl;   // output1_cat of one 8192 x 8192 image is 132 planes x 2049 rows x 2112 floats: more than 2 GiB
    if (plan_workspace(1, 8192, 8192, 5, 2, false, pl) != GS_ERR_UNSUPPORTED || plan_workspace(1, 4096, 4096, 5, 2, false, pl) != GS_OK)
        return fail("the 2 GiB refusal", 0, 0, 0);
    std::printf("espnet setup ok: %d packs, %d plans\n", packs, plans);
    return 0;
}
