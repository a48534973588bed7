/*
 * glomseg_workspace.h -- TEST TOOLS for the activation workspace of an ESPNet handle (an addition to glomseg.h; the ABI number
 * stays: no signature changes, and a caller finds out whether a library has an entry by looking the symbol up).
 *
 * Every convolution of the forward takes its padding from words of the workspace that are zeroed once, when the workspace is
 * laid out, and that no kernel may write afterwards.  csrc/workspace_audit.h sorts every float of every activation piece into
 * one of three classes -- interior (what kernels write), must-be-zero (halos, pitch tails, plane tails and padding planes of the
 * padded pieces; the slack behind every piece), free (the rest) -- and the entries here hold a lane's workspace to it.  None of
 * them launches a kernel, and no product path calls them.
 */
#ifndef GLOMSEG_WORKSPACE_H
#define GLOMSEG_WORKSPACE_H

#include "glomseg.h"

#ifdef __cplusplus
extern "C" {
#endif

#define GS_WS_FREE 0
#define GS_WS_INTERIOR 1
#define GS_WS_MUST_BE_ZERO 2

/* must_be_zero: the words of that class that were looked at; offenders: those whose bits are not 0x00000000.  With
 * offenders > 0 the first one in allocation order: the piece's name, image, plane, and row and column relative to the
 * interior's origin (a left halo has col < 0, a pitch tail col >= W, a top halo row < 0, the bottom halo and the plane tail
 * row >= H; a word of the slack behind a piece: image = the images of the piece, plane = row = 0, col = the word's distance from
 * the slack's start), and its bits. */
typedef struct gs_workspace_report {
    long long must_be_zero, offenders;
    char piece[16];
    int image, plane, row, col;
    unsigned int bits;
} gs_workspace_report;

/* one activation piece: its span starts `offset` bytes into the allocation and holds `span_words` floats, of which the first
 * `own_words` are its images and the rest the slack behind them; padded != 0: it has a halo or padding planes */
typedef struct gs_workspace_piece {
    char name[16];
    unsigned long long offset, own_words, span_words;
    int padded;
    int C, Cp, H, W, pitch, sc, off;
} gs_workspace_piece;

/* Host-only, no handle and no device.  The pieces of the workspace gs_espnet_reserve(h, ws_n, height, width) lays out for such
 * a handle (the arguments and refusals of gs_espnet_workspace_plan), in allocation order: *n_pieces (may be NULL) their number;
 * with 0 <= piece < that number, *info (may be NULL) describes the piece and map (may be NULL; room for `cap` bytes, at least
 * span_words) receives one GS_WS_* class per float of its span. */
gs_status gs_espnet_workspace_classes(int ws_n, int height, int width, int p, int q, int classes, int encoder_only, int piece,
                                      gs_workspace_piece *info, unsigned char *map, size_t cap, int *n_pieces);

/* Host-only, no handle and no device.  Audits `copy`, a host copy of a whole workspace allocation of `bytes` bytes (exactly
 * what gs_espnet_workspace_plan reports for the same arguments), as gs_espnet_workspace_audit audits a lane's. */
gs_status gs_espnet_workspace_audit_host(int ws_n, int height, int width, int p, int q, int classes, int encoder_only,
                                         const void *copy, size_t bytes, gs_workspace_report *report);

/* Waits for the device, copies every activation piece of lane `lane`'s workspace to the host and counts the must-be-zero words
 * that are not zero.  Writes nothing to the device.  A lane without a workspace reports zero words. */
gs_status gs_espnet_workspace_audit(gs_espnet *h, int lane, gs_workspace_report *report);

/* Waits for the device and overwrites every interior and every free float of lane `lane`'s activation pieces with `pattern`
 * (0x7fc00000: a quiet NaN); must-be-zero words keep what they hold.  Nothing but the pieces of the workspace is touched: not
 * the weights, not the ensemble scratch, no flag or mailbox word.  The stages of gs_espnet_read_stage are gone afterwards.
 * Refuses (GS_ERR_UNSUPPORTED) a workspace above 1 GiB. */
gs_status gs_espnet_workspace_poison(gs_espnet *h, int lane, unsigned int pattern);

#ifdef __cplusplus
}
#endif

#endif
