"""Cost of the COCO metric next to the project's own detection metric and to the merge that produced the rows (recorded in
profiles/det_coco.txt; not a gate).

    python tools/det_coco_bench.py [--segments 8] [--frames 198] [--objects 100] [--out profiles/det_coco.txt]
    rocprofv3 --kernel-trace --stats -d DIR -o k1 --output-format csv -- python tools/det_coco_bench.py --trace-run 1      (and 64: runs of their own)
    python tools/det_coco_bench.py --append-trace 1 DIR/k1_kernel_stats.csv --append-trace 64 DIR/k64_kernel_stats.csv   (adds the split to --out)

At the size of tools/det_eval_bench.py (8 segments x 5 cameras x 198 frames from synthetic.make_tracking_json, `categories` added;
the detections and a jittered copy of them are the two ensemble inputs), all in one process on one GPU:
  (a) wt_det_coco_dev for K = 1 and K = 64 results, device events around repeated launches (inputs resident in HBM, tables only);
  (b) wt_det_eval_dev on the same rows, timed the same way in the same run;
  (c) the ensemble merge that produced the scored result, wall clock;
  (d) evaluate_coco_sets end to end for K = 1 (packing in numpy, staging, kernels, read-back), wall clock;
  (e) tests/coco_ap_ref.py on one CPU thread on the first --ref-images images of the K = 1 result (default: all), and that the device
      tables of that subset are equal to it.
The device call is one entry point that enqueues all its kernels, so device events cannot separate its stages; --trace-run K does only
3 warm-up and 5 more launches of K results for a kernel trace taken in a separate run, and --append-trace turns the trace's per-kernel
statistics into the split between the stages (select and match are one kernel).
"""
import argparse
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

CATEGORIES = [{'id': 1, 'name': 'vehicle'}, {'id': 2, 'name': 'pedestrian'}, {'id': 3, 'name': 'sign'}, {'id': 4, 'name': 'cyclist'}]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--segments', type=int, default=8)
    ap.add_argument('--frames', type=int, default=198)
    ap.add_argument('--objects', type=int, default=100)
    ap.add_argument('--repeats', type=int, default=20)
    ap.add_argument('--ref-images', type=int, default=0, help='images of the one-thread CPU restatement (plain Python); 0 = all')
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'det_coco.txt'))
    ap.add_argument('--trace-run', type=int, default=0, choices=(0, 1, 64), help='only 3 + 5 launches of this many results, nothing timed or written')
    ap.add_argument('--append-trace', nargs=2, action='append', metavar=('K', 'CSV'), help='append the stage split of a rocprofv3 kernel_stats.csv to --out')
    args = ap.parse_args()
    if args.append_trace:
        return append_trace(args)
    import numpy as np
    import torch
    assert torch.cuda.is_available(), 'needs the GPU'
    from waymo_2d_tracking_amd import _lib, synthetic as syn
    from waymo_2d_tracking_amd.detnet import ensemble as EN, evaluate as E
    lines = []

    def say(text):
        print(text, flush=True)
        lines.append(text)

    dets, gt_json = syn.make_tracking_json(1, n_segments=args.segments, n_frames=args.frames, n_objects=args.objects)
    gt_json['categories'] = CATEGORIES
    rng = np.random.default_rng(2)
    second = [dict(r, bbox=[int(v + rng.integers(-3, 4)) for v in r['bbox'][:2]] + [max(1, int(v + rng.integers(-3, 4))) for v in r['bbox'][2:]],
                   score=round(float(np.clip(r['score'] + rng.normal(0, 0.02), 0.0, 1.0)), 5)) for r in dets]
    subs = [EN.submission_columns(dets), EN.submission_columns(second)]
    gt = E.pack_coco_ground_truth(gt_json)
    gt_own = E.pack_ground_truth(gt_json)
    say('device: %s' % (_lib.device_info(),))
    say('input: %d segments x 5 cameras x %d frames = %d images, 2 ensemble inputs of %d detections each, %d ground-truth boxes'
        % (args.segments, args.frames, len(gt['image_ids']), len(dets), gt['x'].size))

    def merge(method, iou, cut, min_score):
        image_ids, category_ids, rows = EN.merge_inputs(subs, [1.0, 1.0], min_score)
        packed = EN.pack_groups(len(image_ids), category_ids, rows, 2)
        out5, counts = EN.merge_groups(packed, 2, method, iou, cut)
        o = EN.output_rows(packed, category_ids, out5, counts, min_score)
        b = o['bbox'].astype(np.float64).reshape(-1, 4)
        return dict(image_ids=image_ids, image=o['image'], category=o['category'], score=o['score'], x=b[:, 0], y=b[:, 1], w=b[:, 2], h=b[:, 3])

    reference = ('soft_nms', 0.5, 0.9, 0.01)
    merge(*reference)
    times = []
    for _ in range(5):
        t0 = time.perf_counter()
        one = merge(*reference)
        times.append(time.perf_counter() - t0)
    t_merge = float(np.median(times))
    many = [merge(method, iou, cut, min_score) for method in ('soft_nms', 'nms') for iou in (0.4, 0.45, 0.5, 0.55, 0.6, 0.65, 0.7, 0.75)
            for cut in (0.9, 1.0) for min_score in (0.0, 0.01)]

    def time_dev(dev, repeats):
        for _ in range(3):
            dev.launch()
        torch.cuda.synchronize()
        if not repeats:
            return 0.0
        start, stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        start.record()
        for _ in range(repeats):
            dev.launch()
        stop.record()
        stop.synchronize()
        return start.elapsed_time(stop) / repeats

    if args.trace_run:
        dev = E.DeviceCocoEvaluation(gt, [one] if args.trace_run == 1 else many, per_row=False)
        time_dev(dev, 0)
        for _ in range(5):
            dev.launch()
        torch.cuda.synchronize()
        return
    coco1, coco64 = E.DeviceCocoEvaluation(gt, [one], per_row=False), E.DeviceCocoEvaluation(gt, many, per_row=False)
    own1, own64 = E.DeviceDetEvaluation(gt_own, [one]), E.DeviceDetEvaluation(gt_own, many)
    say('(c) ensemble merge -m soft_nms --iou-thresh=0.5 --soft-nms-cut=0.9 --min-score=0.01 (host calls, packing and staging included): '
        'median %.2f ms of 5 (min %.2f, max %.2f), %d merged rows' % (1e3 * t_merge, 1e3 * min(times), 1e3 * max(times), len(one['score'])))
    # alternate the two evaluators, three rounds each, and keep every figure: the spread is part of the record
    rounds = {'coco1': [], 'own1': [], 'coco64': [], 'own64': []}
    for _ in range(3):
        rounds['coco1'].append(time_dev(coco1, args.repeats)); rounds['own1'].append(time_dev(own1, args.repeats))
        rounds['coco64'].append(time_dev(coco64, max(2, args.repeats // 4))); rounds['own64'].append(time_dev(own64, max(2, args.repeats // 4)))
    med = {k: float(np.median(v)) for k, v in rounds.items()}
    fmt = lambda v: ', '.join('%.3f' % x for x in v)
    say('(a) wt_det_coco_dev K = 1: %.3f ms per call (median of 3 windows of %d calls: %s), %d rows, %d problems, workspace %.1f MiB'
        % (med['coco1'], args.repeats, fmt(rounds['coco1']), coco1.n_det, len(gt['image_ids']) * 4, coco1.ws_bytes / 2.0 ** 20))
    say('(b) wt_det_eval_dev  K = 1: %.3f ms per call (%s), %d rows above min_conf 0.01 or not' % (med['own1'], fmt(rounds['own1']), own1.n_det))
    say('(a) wt_det_coco_dev K = 64: %.3f ms per call = %.3f ms per result (%s), %d rows, %d problems, workspace %.1f MiB'
        % (med['coco64'], med['coco64'] / 64, fmt(rounds['coco64']), coco64.n_det, 64 * len(gt['image_ids']) * 4, coco64.ws_bytes / 2.0 ** 20))
    say('(b) wt_det_eval_dev  K = 64: %.3f ms per call = %.3f ms per result (%s)' % (med['own64'], med['own64'] / 64, fmt(rounds['own64'])))
    r1 = coco1.results()[0]
    for line in r1.lines():
        say('    ' + line)
    res64 = coco64.results()
    best = max(range(64), key=lambda i: (res64[i].stats[0], -i))
    say('    best of the 64 settings by COCO mAP: #%d, %.4f; by the project metric: #%d' % (
        best, res64[best].stats[0], _best_own(own64)))
    # (d) end to end
    E.evaluate_coco_sets(gt, [one])
    times = []
    for _ in range(5):
        t0 = time.perf_counter()
        E.evaluate_coco_sets(gt, [one])
        times.append(time.perf_counter() - t0)
    t_e2e = float(np.median(times))
    say('(d) evaluate_coco_sets K = 1 (packing in numpy, staging, kernels, read-back): median %.2f ms of 5 (min %.2f, max %.2f)'
        % (1e3 * t_e2e, 1e3 * min(times), 1e3 * max(times)))
    # (e) the restatement on a subset, one thread, and equality on that subset
    sys.path.insert(0, os.path.join(ROOT, 'tests'))
    import coco_ap_ref as R
    torch.set_num_threads(1)
    n_ref = min(args.ref_images or len(gt['image_ids']), len(gt['image_ids']))
    keep = set(str(k) for k in gt['image_ids'][:n_ref])
    sub_gt = dict(gt_json, images=[im for im in gt_json['images'] if str(im['id']) in keep],
                  annotations=[a for a in gt_json['annotations'] if str(a['image_id']) in keep])
    ids = one['image_ids']
    rows = [{'image_id': ids[int(i)], 'category_id': int(c), 'bbox': [float(x), float(y), float(w), float(h)], 'score': float(s)}
            for i, c, x, y, w, h, s in zip(one['image'], one['category'], one['x'], one['y'], one['w'], one['h'], one['score']) if str(ids[int(i)]) in keep]
    t0 = time.perf_counter()
    rgt = R.ground_truth(sub_gt)
    ref = R.evaluate(rgt, [R.result(rgt, rows)])
    t_ref = time.perf_counter() - t0
    got = E.evaluate_coco_sets(sub_gt, [rows])[0]
    equal = bool(np.array_equal(got.precision, ref['precision'][0]) and np.array_equal(got.recall, ref['recall'][0]) and np.array_equal(got.npig, ref['npig'][0]))
    say('(e) tests/coco_ap_ref.py (plain Python, one CPU thread) on the first %d images (%d rows, %d boxes): %.2f s = %.1f ms per image; '
        'device tables of that subset equal to it: %s' % (n_ref, len(rows), rgt['x'].size, t_ref, 1e3 * t_ref / max(1, n_ref), equal))

    def verdict(name, holds, detail):
        say('claim "%s": %s (%s)' % (name, 'HOLDS' if holds else 'DOES NOT HOLD', detail))
    verdict('scoring one result costs less than merging it', med['coco1'] < 1e3 * t_merge, 'device call %.3f ms, end to end %.2f ms, merge %.2f ms'
            % (med['coco1'], 1e3 * t_e2e, 1e3 * t_merge))
    verdict('K = 64 costs less per result than K = 1', med['coco64'] / 64 < med['coco1'], '%.3f ms per result against %.3f ms' % (med['coco64'] / 64, med['coco1']))
    say('COCO metric against the project metric on the same rows: K = 1 %.2f x, K = 64 %.2f x the time of wt_det_eval_dev' % (
        med['coco1'] / med['own1'], med['coco64'] / med['own64']))
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, 'wt') as fp:
        fp.write('\n'.join(lines) + '\n')


STAGES = (('prep + npig', ('coco_prep_kernel', 'coco_npig_kernel', 'coco_npig_fill_kernel')), ('select + match', ('coco_match_kernel',)),
          ('order (rocPRIM sorts, gathers, offsets)', ('rocprim', 'det_gather_seg_kernel', 'coco_gather_rows_kernel', 'det_offsets_kernel')),
          ('curve', ('coco_curve_kernel',)))
TRACE_CALLS = 8                                     # --trace-run: 3 warm-up + 5 launches


def append_trace(args):
    import csv
    lines = []
    for k, path in args.append_trace:
        total = {name: 0.0 for name, _ in STAGES}
        with open(path) as fp:
            for row in csv.DictReader(fp):
                for name, keys in STAGES:
                    if any(key in row['Name'] for key in keys):
                        total[name] += float(row['TotalDurationNs'])
                        break
        whole = sum(total.values())
        lines.append('stage split of wt_det_coco_dev K = %s from a kernel trace of %d launches (a run of its own; kernel time only, %.3f ms per call):'
                     % (k, TRACE_CALLS, whole / TRACE_CALLS / 1e6))
        lines += ['    %-42s %9.3f ms per call  %5.1f %%' % (name, total[name] / TRACE_CALLS / 1e6, 100 * total[name] / whole) for name, _ in STAGES]
    print('\n'.join(lines))
    with open(args.out, 'at') as fp:
        fp.write('\n'.join(lines) + '\n')
    return 0


def _best_own(dev):
    res = dev.results()
    return max(range(len(res)), key=lambda i: (res[i].mean_ap(), -i))


if __name__ == '__main__':
    main()
