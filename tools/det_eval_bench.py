"""Cost of scoring detection results next to the cost of producing them (recorded in profiles/det_eval.txt; not a gate).

    python tools/det_eval_bench.py [--segments 8] [--frames 198] [--objects 100] [--out profiles/det_eval.txt]

On a validation-like size (8 segments x 5 cameras x 198 frames from synthetic.make_tracking_json, `categories` added; the
detections and a jittered copy of them are the two ensemble inputs):
  (a) wt_det_eval_dev for K = 1 and K = 64 results, device events around repeated launches (inputs resident in HBM);
  (b) evaluate_detection_sets end to end for K = 1 (packing in numpy, staging, kernels, read-back), wall clock;
  (c) the ensemble merge that produced the scored result (merge_inputs + pack_groups + merge_groups + output_rows), wall clock;
  (d) metric.evaluate_detections on one CPU thread on the same result.
The K = 64 results are 64 different ensemble settings (2 methods x 8 IoU thresholds x 2 cuts x 2 minimal scores).
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
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'det_eval.txt'))
    ap.add_argument('--no-cpu-reference', action='store_true')
    args = ap.parse_args()
    import numpy as np
    import torch
    assert torch.cuda.is_available(), 'needs the GPU'
    from waymo_2d_tracking_amd import _lib, synthetic as syn
    from waymo_2d_tracking_amd.detnet import ensemble as EN, evaluate as E
    from waymo_2d_tracking_amd.detnet.data import metric as M
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
    gt = E.pack_ground_truth(gt_json)
    say('device: %s' % (_lib.device_info(),))
    say('input: %d segments x 5 cameras x %d frames = %d images, 2 ensemble inputs of %d detections each, %d ground-truth boxes'
        % (args.segments, args.frames, len(gt['image_ids']), len(dets), gt['x1'].size))

    def merge(method, iou, cut, min_score):
        image_ids, category_ids, rows = EN.merge_inputs(subs, [1.0, 1.0], min_score)
        packed = EN.pack_groups(len(image_ids), category_ids, rows, 2)
        out5, counts = EN.merge_groups(packed, 2, method, iou, cut)
        o = EN.output_rows(packed, category_ids, out5, counts, min_score)
        b = o['bbox'].astype(np.float64).reshape(-1, 4)
        return dict(image_ids=image_ids, image=o['image'], category=o['category'], score=o['score'], x=b[:, 0], y=b[:, 1], w=b[:, 2], h=b[:, 3])

    # (c) the merge
    reference = ('soft_nms', 0.5, 0.9, 0.01)
    merge(*reference)
    times = []
    for _ in range(5):
        t0 = time.perf_counter()
        one = merge(*reference)
        times.append(time.perf_counter() - t0)
    t_merge = float(np.median(times))
    say('(c) ensemble merge -m soft_nms --iou-thresh=0.5 --soft-nms-cut=0.9 --min-score=0.01 (host calls, packing and staging included): '
        'median %.2f ms of 5 (min %.2f, max %.2f), %d merged rows' % (1e3 * t_merge, 1e3 * min(times), 1e3 * max(times), len(one['score'])))

    # (a) the evaluator, device form
    def time_dev(sets):
        dev = E.DeviceDetEvaluation(gt, sets)
        for _ in range(3):
            dev.launch()
        torch.cuda.synchronize()
        start, stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        start.record()
        for _ in range(args.repeats):
            dev.launch()
        stop.record()
        stop.synchronize()
        return start.elapsed_time(stop) / args.repeats, dev

    ms1, dev1 = time_dev([one])
    r1 = dev1.results()[0]
    say('(a) wt_det_eval_dev K = 1: %.3f ms per call (events around %d calls), %d rows, %d problems, workspace %.1f MiB'
        % (ms1, args.repeats, dev1.n_det, len(gt['image_ids']) * 4, dev1.ws_bytes / 2.0 ** 20))
    for line in r1.lines():
        say('    ' + line)
    # (b) end to end
    E.evaluate_detection_sets(gt, [one])
    times = []
    for _ in range(5):
        t0 = time.perf_counter()
        E.evaluate_detection_sets(gt, [one])
        times.append(time.perf_counter() - t0)
    t_e2e = float(np.median(times))
    say('(b) evaluate_detection_sets K = 1 (packing in numpy, staging, kernels, read-back): median %.2f ms of 5 (min %.2f, max %.2f)'
        % (1e3 * t_e2e, 1e3 * min(times), 1e3 * max(times)))
    many = []
    t0 = time.perf_counter()
    for method in ('soft_nms', 'nms'):
        for iou in (0.4, 0.45, 0.5, 0.55, 0.6, 0.65, 0.7, 0.75):
            for cut in (0.9, 1.0):
                for min_score in (0.0, 0.01):
                    many.append(merge(method, iou, cut, min_score))
    t_many = time.perf_counter() - t0
    ms64, dev64 = time_dev(many)
    say('(a) wt_det_eval_dev K = 64: %.3f ms per call = %.3f ms per result, %d rows, %d problems, workspace %.1f MiB (merging the 64 settings: %.2f s)'
        % (ms64, ms64 / 64, dev64.n_det, 64 * len(gt['image_ids']) * 4, dev64.ws_bytes / 2.0 ** 20, t_many))
    res64 = dev64.results()
    best = max(range(64), key=lambda i: (res64[i].mean_ap(), -i))
    say('    best of the 64 settings: #%d, mean AP %.4f (K = 1 setting above: %.4f)' % (best, res64[best].mean_ap(), r1.mean_ap()))

    # (d) the host loop
    t_ref = None
    if not args.no_cpu_reference:
        torch.set_num_threads(1)
        p = E.pack_detections(gt, [one])
        per_image = {}
        lo = p['image_det_offsets'][0]
        for i, k in enumerate(gt['image_ids']):
            a, b = int(lo[i]), int(lo[i + 1])
            rows = np.stack([p[c][a:b] for c in E.DET_COLUMNS], axis=1)
            per_image[k] = [rows[p['category'][a:b] == c] for c in (1, 2, 3, 4)]
        t0 = time.perf_counter()
        ev = M.evaluate_detections(per_image, gt_json)
        t_ref = time.perf_counter() - t0
        worst = max(abs(ev[n]['ap'] - r1.summary()[n]['ap']) for n, _ in r1.classes)
        tied = 0
        for c in (1, 2, 3, 4):
            conf = p['conf'][(p['category'] == c) & (p['conf'] > 0.01)]
            _, counts = np.unique(conf, return_counts=True)
            tied += int(counts[counts > 1].sum())
        say('(d) metric.evaluate_detections (numpy, one CPU thread) on the K = 1 result: %.2f s; largest |AP difference| to the device over the classes %.3g'
            % (t_ref, worst))
        say('    %d of the %d rows share their 5-decimal wire score with another row of their class: the order of equal confidences is defined on '
            'the device and an accident of the sort in metric.py, so the two agree to the bound of DESIGN section 16 only on tie-free input' % (tied, p['conf'].size))

    def verdict(name, holds, detail):
        say('claim "%s": %s (%s)' % (name, 'HOLDS' if holds else 'DOES NOT HOLD', detail))
    verdict('scoring one result costs less than merging it', ms1 < 1e3 * t_merge, 'device call %.3f ms, end to end %.2f ms, merge %.2f ms'
            % (ms1, 1e3 * t_e2e, 1e3 * t_merge))
    if t_ref is not None:
        verdict('scoring one result costs less than metric.py', 1e3 * t_e2e < 1e3 * t_ref, 'end to end %.2f ms against %.0f ms: %.0f x; device call alone %.0f x'
                % (1e3 * t_e2e, 1e3 * t_ref, t_ref / t_e2e, 1e3 * t_ref / ms1))
    verdict('K = 64 in one call costs less per result than K = 1', ms64 / 64 < ms1, '%.3f ms per result against %.3f ms' % (ms64 / 64, ms1))
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, 'wt') as fp:
        fp.write('\n'.join(lines) + '\n')


if __name__ == '__main__':
    main()
