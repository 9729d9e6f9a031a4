"""Hand-off check of the COCO metric against the pycocotools package, where that package is installed.

    python tools/check_coco_eval.py --gt GT.json --dt DETS.json [--dt-images]

The metric of detnet/evaluate.py is this project's restatement of the published algorithm, pinned by
hand-worked cases because the package is not a dependency.  Where it is installed, this runs COCOeval (iouType 'bbox') and the
device path on the same two files and prints the largest difference per statistic; where it is not, it prints one line and exits
0.  One departure is stated in the definition: an empty intersection has IoU 0 also where the union is 0.  No test calls this.
"""
import argparse
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--gt', required=True)
    ap.add_argument('--dt', required=True)
    ap.add_argument('--dt-images', action='store_true')
    args = ap.parse_args()
    try:
        from pycocotools.coco import COCO
        from pycocotools.cocoeval import COCOeval
    except ImportError:
        print('pycocotools is not installed: nothing to compare (the metric stays pinned by tests/test_coco_ap_ref.py)')
        return 0
    import numpy as np
    from waymo_2d_tracking_amd.detnet import evaluate as E
    ours = E.evaluate_coco_sets(args.gt, [args.dt], dt_images=args.dt_images)[0]
    coco_gt = COCO(args.gt)
    coco_dt = coco_gt.loadRes(args.dt)
    ev = COCOeval(coco_gt, coco_dt, 'bbox')
    if args.dt_images:
        ev.params.imgIds = sorted(coco_dt.getImgIds())
    ev.evaluate()
    ev.accumulate()
    ev.summarize()
    theirs = np.asarray(ev.stats, np.float64)
    worst = 0.0
    for name, a, b in zip(E.COCO_STATS, ours.stats, theirs):
        print('%-6s device %.17g  package %.17g  |difference| %.3g' % (name, a, b, abs(a - b)))
        worst = max(worst, abs(a - b))
    p = np.asarray(ev.eval['precision'], np.float64)                   # (T, R, K, A, M), the layout of the device table
    if p.shape == ours.precision.shape:
        print('precision table: largest |difference| %.3g over %d entries' % (float(np.abs(p - ours.precision).max()), p.size))
    print('largest |difference| over the twelve statistics: %.3g' % worst)
    return 0


if __name__ == '__main__':
    sys.exit(main())
