// Sanitizer driver (tests/test_workspace_invariants.py) for csrc/workspace_audit.h: the classes of every float of an activation
// workspace, the audit and the poison over host copies.  Every span is a heap block of exactly its size, so AddressSanitizer
// sees a run, a map byte, a poisoned word or an audited word past either end.  Built with g++ only: no HIP in here.
#include <cstdarg>
#include <cstdio>
#include <vector>

#include "workspace_audit.h"

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

static int fail(const char *what, const char *piece, int a, int b, int c)
{
    std::fprintf(stderr, "FAILED: %s (%s; %d, %d, %d)\n", what, piece, a, b, c);
    return 1;
}

static int check(int n, int H, int W, int c, int p, bool enc, long long &words)
{
    constexpr uint32_t QNAN = 0x7fc00000u;
    WorkspacePlan pl;
    if (plan_workspace(n, H, W, padded_classes(c), p, enc, pl) != GS_OK)
        return fail("plan_workspace refused a small shape", "", H, W, c);
    size_t end = 0;
    WsReport total;
    for (int i = 0; i < WS_PIECES; ++i) {
        const WsPiece pc = ws_piece(pl, n, i, c);
        if (pc.at != end || pc.own_words > pc.span_words || pc.span_words - pc.own_words < WS_SLACK / sizeof(float))
            return fail("the spans do not tile the allocation", pc.name, H, W, c);
        end = pc.at + pc.span_words * sizeof(float);
        // the runs: ascending, gap-free, the whole span
        size_t at = 0, counts[3] = {0, 0, 0};
        bool ordered = true;
        ws_for_each_run(pc, [&](WsClass cls, size_t b, size_t e) {
            ordered = ordered && b == at && e > b && cls <= WS_MUST_BE_ZERO;
            counts[cls] += e - b;
            at = e;
        });
        if (!ordered || at != pc.span_words)
            return fail("the runs leave a gap, overlap or stop short of the span", pc.name, H, W, c);
        if (!pc.padded && counts[WS_MUST_BE_ZERO] != pc.span_words - pc.own_words)
            return fail("a halo-less piece has must-be-zero words other than its slack", pc.name, H, W, c);
        if (pc.padded && counts[WS_FREE])
            return fail("a padded piece has free words", pc.name, H, W, c);
        std::vector<unsigned char> map(pc.span_words);
        ws_class_map(pc, map.data());
        std::vector<uint32_t> copy(pc.span_words, 0u);
        ws_poison_piece(pc, copy.data(), QNAN);
        for (size_t w = 0; w < pc.span_words; ++w)
            if ((copy[w] == QNAN) != (map[w] != WS_MUST_BE_ZERO))
                return fail("the poison and the class map disagree", pc.name, H, W, c);
        WsReport rep;
        ws_audit_piece(pc, copy.data(), rep);
        if (rep.offenders || rep.must_be_zero != (long long)counts[WS_MUST_BE_ZERO])
            return fail("a poisoned span does not audit clean", pc.name, H, W, c);
        // the first and the last must-be-zero word of the span, and where the audit says they are
        size_t first = pc.span_words;
        for (size_t w = 0; w < pc.span_words && first == pc.span_words; ++w)
            if (map[w] == WS_MUST_BE_ZERO) first = w;
        copy[first] = 1u, copy[pc.span_words - 1] = 2u;
        rep = WsReport();
        ws_audit_piece(pc, copy.data(), rep);
        const WsWhere wh = ws_where(pc, first);
        if (rep.offenders != 2 || rep.bits != 1u || rep.image != wh.image || rep.plane != wh.plane || rep.row != wh.row || rep.col != wh.col)
            return fail("two planted offenders are not reported as such", pc.name, H, W, c);
        if (first < pc.own_words) {   // ws_where's coordinates lead back to the word
            const Act &a = pc.act;
            const long long back = (long long)wh.image * a.sn + (long long)wh.plane * a.sc + a.off + (long long)wh.row * a.pitch + wh.col;
            if (back != (long long)first)
                return fail("ws_where does not invert the activation's addressing", pc.name, H, W, c);
        }
        ws_audit_piece(pc, copy.data(), total);
        words += (long long)pc.span_words;
    }
    if (end != pl.bytes || total.offenders != 2 * WS_PIECES)
        return fail("the spans do not end with the allocation", "", H, W, c);
    return 0;
}

int main()
{
    int plans = 0;
    long long words = 0;
    static const int shapes[][3] = {{1, 8, 8}, {3, 8, 8}, {3, 8, 24}, {1, 24, 24}, {1, 8, 264}, {1, 136, 8}, {2, 136, 24}};   // n, H, W
    for (int c : {2, 5, 7, 12, 18, 20})   // every padded count but 16; 7 and 18 leave class planes no kernel writes
        for (int enc = 0; enc < (c == 5 ? 2 : 1); ++enc)
            for (int p = 0; p <= 1; ++p)   // b2 with storage of its own, and lazy
                for (const int *s : shapes) {
                    if (check(s[0], s[1], s[2], c, p, enc != 0, words)) return 1;
                    ++plans;
                }
    std::printf("workspace audit ok: %d plans, %lld words\n", plans, words);
    return 0;
}
