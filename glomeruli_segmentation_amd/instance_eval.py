"""Per-glomerulus scoring of a slide against its annotation: match the instances of the two class maps on the GPU.

wsi_eval scores per pixel (a confusion matrix, IoU rows): one large glomerulus outweighs ten small missed ones.  Here the rows
are glomeruli.  Both 1/8 class maps (WindowEvaluator.run()'s gt_map / pred_map, or the <slide>_gt_classmap.png /
<slide>_pred_classmap.png files wsi_eval writes) are labelled by gs_slide_instances (instances.label_instances);
gs_instance_overlaps lists every pair of a ground-truth and a predicted instance that share a pixel, with the shared pixels and
those of them whose class agrees; gs_instance_match marks a pair as matched when its IoU is strictly above the threshold
(include/glomseg_instance_match.h, csrc/instance_match.hip).  With a threshold of at least 1/2 a match is unique on both sides,
so there is no assignment to solve.  All of it is integer arithmetic; the ratios below are float64 on the host from those
integers.

    python -m glomeruli_segmentation_amd.instance_eval --eval_dir DIR --output_csv FILE --summary_tsv FILE
           [--classes 5] [--connectivity 8] [--iou_threshold 0.5] [--gpu_id 0] [--boundary]

--boundary adds, per matched pair, how far the two outlines lie apart (include/glomseg_boundary_dist.h, csrc/boundary_dist.hip:
exact squared distances between the boundary pixels of the pair, on the GPU): the Hausdorff distance, its 95th percentile, the
average surface distance and the root mean square, in map pixels.
"""
import glob
import os
import sys
from argparse import ArgumentParser
from fractions import Fraction

import numpy as np

from . import _call, _lib, _slides
from . import instances
from ._slides import host as _host

GT_SUFFIX, PRED_SUFFIX = "_gt_classmap.png", "_pred_classmap.png"           # what wsi_eval writes
IOU_DEN_MAX = 65535
SUMMARY_KEYS = ["gt", "pred", "tp", "fp", "fn", "precision", "recall", "f1", "mean_iou", "pq", "mean_dice"]
BOUNDARY_COLUMNS = ["hd", "hd95", "assd", "rmsd"]                            # --boundary: behind a TP row, in map pixels
BOUNDARY_SUMMARY_KEYS = ["mean_hd", "mean_hd95", "mean_assd"]                # ... and behind the summary


def check_threshold(iou):
    """(num, den) or a Fraction -> (num, den) in the ABI's range: 1 <= num <= den <= 65535, 2 * num >= den"""
    num, den = (iou.numerator, iou.denominator) if isinstance(iou, Fraction) else (int(iou[0]), int(iou[1]))
    if not (1 <= num <= den <= IOU_DEN_MAX and 2 * num >= den):
        raise ValueError("the IoU threshold must be num / den with 1 <= num <= den <= %d and at least 1/2: below 1/2 a match is "
                         "not unique (got %s / %s)" % (IOU_DEN_MAX, num, den))
    return num, den


def parse_threshold(text):
    """'0.5', '3/5', '0.59' -> (num, den), exactly (fractions.Fraction), refused where it does not fit the ABI"""
    try:
        f = Fraction(text)
    except (ValueError, ZeroDivisionError):
        raise ValueError("the IoU threshold %r is neither a decimal nor a fraction" % (text,))
    return check_threshold(f)


def workspace_bytes(height, width, pair_cap=4096):
    """gs_instance_match_plan: host-only"""
    return _call.planned_bytes(_lib.load().gs_instance_match_plan, height, width, pair_cap)


def boundary_workspace_bytes(height, width):
    """gs_boundary_dist_plan: host-only"""
    return _call.planned_bytes(_lib.load().gs_boundary_dist_plan, height, width)


def boundary_ratios(stats, samples):
    """stats: int64 [n_gt,2,3] {boundary pixels, max d2, sum of d2} per direction; samples: per direction (ids, d2), the gt id and
    the d2 of every boundary pixel that has one, sorted ascending by (id, d2) -> {"hd", "hd95", "assd", "rmsd"}: float64 [n_gt],
    nan where the instance has no sample in either direction (unmatched).  numpy on the host, from the exact integers:
    hd = sqrt(max d2 over both directions); hd95 = sqrt of the larger of the two directions' nearest-rank 95th percentiles
    (element (95 * n + 99) // 100, 1-based, of the direction's sorted d2); assd = sum of sqrt(d2) / (n0 + n1);
    rmsd = sqrt(sum of d2 / (n0 + n1))."""
    stats = np.asarray(stats, dtype=np.int64).reshape(-1, 2, 3)
    n_gt = len(stats)
    n = stats[:, :, 0]
    have = (n[:, 0] > 0) & (n[:, 1] > 0)
    p95 = np.zeros((n_gt, 2), dtype=np.int64)
    root_sum = np.zeros(n_gt, dtype=np.float64)
    for d, (ids, d2) in enumerate(samples):
        ids, d2 = np.asarray(ids, dtype=np.int64), np.asarray(d2, dtype=np.int64)
        if len(ids) != int(n[:, d].sum()) or np.any(np.bincount(ids - 1, minlength=n_gt)[:n_gt] != n[:, d]):
            raise ValueError("direction %d: the samples are not the boundary pixels stats counts" % d)
        start = np.cumsum(n[:, d]) - n[:, d]
        rank = (95 * n[:, d] + 99) // 100                                      # 1-based, 1..n where n >= 1
        some = n[:, d] > 0
        p95[some, d] = d2[(start + rank - 1)[some]]
        np.add.at(root_sum, ids - 1, np.sqrt(d2.astype(np.float64)))
    total = np.where(have, n.sum(axis=1), 1).astype(np.float64)
    nan = np.full(n_gt, np.nan)
    return {"hd": np.where(have, np.sqrt(stats[:, :, 1].max(axis=1).astype(np.float64)), nan),
            "hd95": np.where(have, np.sqrt(p95.max(axis=1).astype(np.float64)), nan),
            "assd": np.where(have, root_sum / total, nan),
            "rmsd": np.where(have, np.sqrt(stats[:, :, 2].sum(axis=1).astype(np.float64) / total), nan)}


def boundary_distances(result):
    """result: what match_instances returns (labels and match arrays on the device) -> {"stats": int64 [n_gt,2,3] {boundary
    pixels, max d2, sum of d2} by (gt id - 1, direction), "dist_gt", "dist_pred": int32 [h,w], d2 at the boundary pixels of the
    matched instances and -1 elsewhere (tensors on the labels' device), "hd", "hd95", "assd", "rmsd": float64 [n_gt] numpy arrays,
    nan where unmatched (boundary_ratios), in map pixels}.  The integers are gs_instance_boundary_dist's; the per-pair
    distributions are read off its two maps with torch on the device (mask, sort by (id, d2)) and the ratios taken on the host."""
    import torch
    lib = _lib.load()
    lg, lp = result["gt"]["labels"], result["pred"]["labels"]
    if lg is None or lp is None or not getattr(lg, "is_cuda", False) or not getattr(lp, "is_cuda", False):
        raise ValueError("boundary_distances needs match_instances' result with its label maps on the GPU")
    dev = lg.device
    h, w = lg.shape
    n_gt, n_pred = int(result["gt"]["n"]), int(result["pred"]["n"])
    lg, lp = lg.contiguous(), lp.contiguous()
    match_gt, match_pred = result["match_gt"].contiguous(), result["match_pred"].contiguous()
    with torch.cuda.device(dev):
        stream = _call.stream_ptr(dev)
        ws = torch.empty(boundary_workspace_bytes(h, w), dtype=torch.uint8, device=dev)
        dist_gt = torch.empty((h, w), dtype=torch.int32, device=dev)
        dist_pred = torch.empty((h, w), dtype=torch.int32, device=dev)
        stats = torch.empty((n_gt, 2, 3), dtype=torch.int64, device=dev)
        _lib.check(lib.gs_instance_boundary_dist(lg.data_ptr(), lp.data_ptr(), match_gt.data_ptr() if n_gt else None, n_gt,
                                                 match_pred.data_ptr() if n_pred else None, n_pred, h, w, ws.data_ptr(), ws.numel(),
                                                 dist_gt.data_ptr(), dist_pred.data_ptr(), stats.data_ptr() if n_gt else None, stream))
        samples = []
        for dist, labels, partner in ((dist_gt, lg, None), (dist_pred, lp, match_pred)):
            mask = dist >= 0
            ids, d2 = labels[mask].to(torch.int64), dist[mask].to(torch.int64)
            if partner is not None:
                ids = partner.to(torch.int64)[ids - 1]                         # a pixel with a d2 belongs to a matched prediction
            key = torch.sort(ids << 31 | d2).values                            # d2 < 2^31
            samples.append(((key >> 31).cpu().numpy(), (key & 0x7FFFFFFF).cpu().numpy()))
        out = {"stats": stats, "dist_gt": dist_gt, "dist_pred": dist_pred}
        out.update(boundary_ratios(stats.cpu().numpy(), samples))
    return out


def match_instances(gt_map, pred_map, classes=5, connectivity=8, iou=(1, 2), pair_cap=4096, boundary=False):
    """gt_map, pred_map: uint8 [h,w] of one size, CUDA tensors or numpy arrays (uploaded to the current device).
    -> {"gt", "pred": instances.label_instances' tables with labels, "pairs" int32 [n,2] (gt id, pred id; ascending),
        "inter", "agree" int64 [n], "match_gt" int32 [n_gt] (matched pred id or 0), "match_pred" int32 [n_pred], "iou": (num, den)},
    tensors on the maps' device.  On overflow of the pair table it runs again with pair_cap doubled: two maps have no more
    distinct pairs than pixels, so that ends.  boundary=True adds boundary_distances' result under "boundary"."""
    import torch
    lib = _lib.load()
    num, den = check_threshold(iou)
    gt_map, pred_map = (_call.device_map(m, "uint8", "a class map", upload=True) for m in (gt_map, pred_map))
    if gt_map.shape != pred_map.shape or gt_map.device != pred_map.device:
        raise ValueError("ground truth %s and prediction %s differ in size or device" % (tuple(gt_map.shape), tuple(pred_map.shape)))
    dev = gt_map.device
    h, w = gt_map.shape
    pair_cap = max(1, int(pair_cap))
    with torch.cuda.device(dev):
        gt = instances.label_instances(gt_map, classes=classes, connectivity=connectivity, want_labels=True)
        pred = instances.label_instances(pred_map, classes=classes, connectivity=connectivity, want_labels=True)
        stream = _call.stream_ptr(dev)
        n_pairs = torch.empty(2, dtype=torch.int32, device=dev)
        while True:
            ws = torch.empty(workspace_bytes(h, w, pair_cap), dtype=torch.uint8, device=dev)
            pairs = torch.empty((pair_cap, 2), dtype=torch.int32, device=dev)
            inter = torch.empty((pair_cap, 2), dtype=torch.int64, device=dev)
            _lib.check(lib.gs_instance_overlaps(gt["labels"].data_ptr(), pred["labels"].data_ptr(), gt_map.data_ptr(), pred_map.data_ptr(),
                                                h, w, ws.data_ptr(), ws.numel(), pair_cap, pairs.data_ptr(), inter.data_ptr(),
                                                n_pairs.data_ptr(), stream))
            n, overflow = n_pairs.tolist()
            if not overflow:
                break
            if pair_cap >= h * w:
                raise RuntimeError("gs_instance_overlaps reports more distinct pairs than pixels")      # (cannot happen)
            pair_cap = min(2 * pair_cap, h * w)
        counts_gt, counts_pred = gt["counts"].contiguous(), pred["counts"].contiguous()
        match_gt = torch.empty(gt["n"], dtype=torch.int32, device=dev)
        match_pred = torch.empty(pred["n"], dtype=torch.int32, device=dev)
        _lib.check(lib.gs_instance_match(pairs.data_ptr(), inter.data_ptr(), n_pairs.data_ptr(), pair_cap,
                                         counts_gt.data_ptr() if gt["n"] else None, gt["n"],
                                         counts_pred.data_ptr() if pred["n"] else None, pred["n"], int(classes), num, den,
                                         match_gt.data_ptr() if gt["n"] else None, match_pred.data_ptr() if pred["n"] else None, stream))
    result = {"gt": gt, "pred": pred, "pairs": pairs[:n], "inter": inter[:n, 0], "agree": inter[:n, 1], "match_gt": match_gt,
              "match_pred": match_pred, "iou": (num, den)}
    if boundary:
        result["boundary"] = boundary_distances(result)
    return result


def header(classes=5, boundary=False):
    """the columns of instance_rows: the class names are instances.header's; boundary: BOUNDARY_COLUMNS behind them"""
    names = instances.header(classes)[7:]
    return (['slide', 'kind', 'gt_id', 'gt_xmin', 'gt_ymin', 'gt_xmax', 'gt_ymax', 'gt_area', 'pred_id', 'pred_xmin', 'pred_ymin',
             'pred_xmax', 'pred_ymax', 'pred_area', 'inter', 'iou', 'dice', 'class_agreement']
            + ['gt_' + c for c in names] + ['pred_' + c for c in names] + (BOUNDARY_COLUMNS if boundary else []))


def on_host(result):
    """the result as numpy arrays, without the label maps: what instance_rows and summary need of it"""
    def side(t):
        return {"n": t["n"], "boxes": _host(t["boxes"]), "counts": _host(t["counts"]), "labels": None}
    out = {"gt": side(result["gt"]), "pred": side(result["pred"]), "pairs": _host(result["pairs"]), "inter": _host(result["inter"]),
           "agree": _host(result["agree"]), "match_gt": _host(result["match_gt"]), "match_pred": _host(result["match_pred"]),
           "iou": result["iou"]}
    if "boundary" in result:                       # without the two maps: the rows and the summary need the ratios only
        out["boundary"] = {k: _host(result["boundary"][k]) for k in ["stats"] + BOUNDARY_COLUMNS}
    return out


def _tables(result):
    """the result on the host, as Python integers: (gt boxes, gt counts, pred boxes, pred counts, {(g, p): (inter, agree)},
    match_gt, match_pred)"""
    gb, gc = _host(result["gt"]["boxes"]).astype(np.int64).tolist(), _host(result["gt"]["counts"]).astype(np.int64).tolist()
    pb, pc = _host(result["pred"]["boxes"]).astype(np.int64).tolist(), _host(result["pred"]["counts"]).astype(np.int64).tolist()
    pairs = _host(result["pairs"]).astype(np.int64).reshape(-1, 2).tolist()
    inter, agree = _host(result["inter"]).astype(np.int64).tolist(), _host(result["agree"]).astype(np.int64).tolist()
    table = {(g, p): (i, a) for (g, p), i, a in zip(pairs, inter, agree)}
    return gb, gc, pb, pc, table, _host(result["match_gt"]).astype(np.int64).tolist(), _host(result["match_pred"]).astype(np.int64).tolist()


def _matched(result):
    """[(g, p, area_g, area_p, inter, agree)] of the matched pairs, ascending by g"""
    _, gc, _, pc, table, match_gt, _ = _tables(result)
    return [(g, p, sum(gc[g - 1]), sum(pc[p - 1])) + table[(g, p)] for g, p in enumerate(match_gt, 1) if p]


def instance_rows(result, key, boundary=False):
    """header(classes) names the columns.  One row per ground-truth instance, kind TP (matched) or FN, then one per unmatched
    prediction, kind FP.  The columns of the absent side are empty; inter, IoU, Dice and class agreement (agree / inter) belong
    to a TP row.  boundary: header(classes, True)'s four columns from result["boundary"] behind a TP row, empty elsewhere."""
    if boundary:
        b = result["boundary"]
        ratios = [[float(b[k][g]) for k in BOUNDARY_COLUMNS] for g in range(len(_host(result["match_gt"])))]
        return [row + (ratios[row[2] - 1] if row[1] == 'TP' else [''] * len(BOUNDARY_COLUMNS)) for row in instance_rows(result, key)]
    gb, gc, pb, pc, table, match_gt, match_pred = _tables(result)
    width = len(gc[0]) if gc else (len(pc[0]) if pc else 1)
    none_side, none_classes = [''] * 6, [''] * (width - 1)
    rows = []
    for g, p in enumerate(match_gt, 1):
        area_g = sum(gc[g - 1])
        gt_side = [g] + gb[g - 1] + [area_g]
        if p:
            area_p = sum(pc[p - 1])
            inter, agree = table[(g, p)]
            rows.append([key, 'TP'] + gt_side + [p] + pb[p - 1] + [area_p, inter, inter / (area_g + area_p - inter),
                                                                  2 * inter / (area_g + area_p), agree / inter]
                        + gc[g - 1][1:] + pc[p - 1][1:])
        else:
            rows.append([key, 'FN'] + gt_side + none_side + ['', '', '', ''] + gc[g - 1][1:] + none_classes)
    for p, g in enumerate(match_pred, 1):
        if not g:
            rows.append([key, 'FP'] + none_side + [p] + pb[p - 1] + [sum(pc[p - 1]), '', '', '', ''] + none_classes + pc[p - 1][1:])
    return rows


def summary(results):
    """one result, or a list of results pooled -> the counts and, in float64 from the exact integers: precision, recall,
    f1 (recognition quality), mean_iou over the matched pairs (segmentation quality), pq = f1 * mean_iou (panoptic quality),
    mean_dice.  A ratio with nothing below the line is nan."""
    if isinstance(results, dict):
        results = [results]
    n_gt = n_pred = tp = 0
    ious, dices = [], []
    for r in results:
        m = _matched(r)
        n_gt += len(_host(r["match_gt"]))
        n_pred += len(_host(r["match_pred"]))
        tp += len(m)
        ious += [inter / (ag + ap - inter) for _, _, ag, ap, inter, _ in m]
        dices += [2 * inter / (ag + ap) for _, _, ag, ap, inter, _ in m]
    fp, fn = n_pred - tp, n_gt - tp
    nan = float('nan')
    precision = tp / n_pred if n_pred else nan
    recall = tp / n_gt if n_gt else nan
    f1 = 2 * tp / (n_gt + n_pred) if n_gt + n_pred else nan
    mean_iou = float(np.sum(np.array(ious, dtype=np.float64)) / tp) if tp else nan
    mean_dice = float(np.sum(np.array(dices, dtype=np.float64)) / tp) if tp else nan
    pq = float(np.sum(np.array(ious, dtype=np.float64)) / (tp + 0.5 * fp + 0.5 * fn)) if n_gt + n_pred else nan
    return {"gt": n_gt, "pred": n_pred, "tp": tp, "fp": fp, "fn": fn, "precision": precision, "recall": recall, "f1": f1,
            "mean_iou": mean_iou, "pq": pq, "mean_dice": mean_dice}


def boundary_summary(results):
    """one result with "boundary", or a list of them pooled -> mean_hd, mean_hd95, mean_assd over the matched pairs, float64;
    nan without a matched pair"""
    if isinstance(results, dict):
        results = [results]
    out = {}
    for name, k in zip(BOUNDARY_SUMMARY_KEYS, BOUNDARY_COLUMNS):
        v = np.concatenate([np.asarray(_host(r["boundary"][k]), dtype=np.float64).reshape(-1) for r in results] + [np.zeros(0)])
        v = v[~np.isnan(v)]
        out[name] = float(np.sum(v) / len(v)) if len(v) else float('nan')
    return out


def summary_row(key, s):
    return [key] + [s[k] for k in SUMMARY_KEYS] + [s[k] for k in BOUNDARY_SUMMARY_KEYS if k in s]


def build_parser():
    p = ArgumentParser(description='per-glomerulus scoring of the slide class maps wsi_eval writes: matched, missed and spurious instances')
    p.add_argument('--eval_dir', required=True, help='directory of the <slide>_gt_classmap.png / <slide>_pred_classmap.png pairs wsi_eval writes')
    p.add_argument('--output_csv', required=True, help='one row per ground-truth instance (TP / FN) and per unmatched prediction (FP)')
    p.add_argument('--summary_tsv', required=True, help='one line per slide and one over all slides')
    p.add_argument('--classes', type=int, default=5)
    p.add_argument('--connectivity', type=int, default=8, choices=[4, 8])
    p.add_argument('--iou_threshold', default='0.5', help='a decimal or a fraction, at least 1/2; a pair matches strictly above it')
    p.add_argument('--gpu_id', type=int, default=0)
    p.add_argument('--boundary', action='store_true', help='add the boundary distances of every matched pair, in map pixels: the columns '
                   'hd, hd95, assd, rmsd behind the TP rows and mean_hd, mean_hd95, mean_assd behind the summary')
    return p


def find_pairs(eval_dir):
    """[(slide, gt path, pred path)], sorted; a slide with only one of the two files is an error naming the file"""
    gts = {os.path.basename(p)[:-len(GT_SUFFIX)]: p for p in glob.glob(os.path.join(eval_dir, "*" + GT_SUFFIX))}
    preds = {os.path.basename(p)[:-len(PRED_SUFFIX)]: p for p in glob.glob(os.path.join(eval_dir, "*" + PRED_SUFFIX))}
    if not gts and not preds:
        raise FileNotFoundError("no *%s / *%s under %s" % (GT_SUFFIX, PRED_SUFFIX, eval_dir))
    for slide in sorted(set(gts) ^ set(preds)):
        have, lack = (gts[slide], PRED_SUFFIX) if slide in gts else (preds[slide], GT_SUFFIX)
        raise FileNotFoundError("%s has no partner %s%s" % (have, slide, lack))
    return [(slide, gts[slide], preds[slide]) for slide in sorted(gts)]


def main(argv=None, out=sys.stdout):
    args = build_parser().parse_args(argv)
    iou = parse_threshold(args.iou_threshold)
    import torch
    _slides.require_device("the instances are labelled and matched on the GPU")
    triples = find_pairs(args.eval_dir)
    rows, lines, results = [], [], []
    with torch.cuda.device(args.gpu_id):
        for slide, gt_path, pred_path in triples:
            gt, pred = _slides.read_map(gt_path), _slides.read_map(pred_path)
            if gt.shape != pred.shape:
                raise ValueError("%s is %d x %d but %s is %d x %d" % ((pred_path,) + pred.shape[::-1] + (gt_path,) + gt.shape[::-1]))
            res = match_instances(gt, pred, classes=args.classes, connectivity=args.connectivity, iou=iou, boundary=args.boundary)
            res = on_host(res)
            results.append(res)
            rows += instance_rows(res, slide, boundary=args.boundary)
            s = summary(res)
            if args.boundary:
                s.update(boundary_summary(res))
            lines.append(summary_row(slide, s))
            print("{}: {} annotated, {} predicted, {} matched".format(slide, s["gt"], s["pred"], s["tp"]), file=out)
    s = summary(results)
    if args.boundary:
        s.update(boundary_summary(results))
    lines.append(summary_row("all", s))
    _slides.write_table(args.output_csv, header(args.classes, args.boundary), rows)
    _slides.write_table(args.summary_tsv, ['slide'] + SUMMARY_KEYS + (BOUNDARY_SUMMARY_KEYS if args.boundary else []), lines, delimiter='\t')
    return 0


if __name__ == '__main__':
    sys.exit(main())
