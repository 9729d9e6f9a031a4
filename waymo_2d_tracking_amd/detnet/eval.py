"""COCO bbox evaluation of one detection file on the GPU.

    python -m waymo_2d_tracking_amd.detnet.eval --gt GT.json --dt DETS.json [--dt-images] [--catId 1,2] [--each-category]

Prints the twelve summary numbers (AP@[.5:.95], AP50, AP75, AP by area, AR at 1 / 10 / 100 detections, AR by area) of the
selected categories; with --each-category also one table row per category that has any value, best mAP first.  The numbers
come from the HIP kernels behind ``wt_det_coco_host`` through detnet/evaluate.py (DESIGN.md section 28 has the definition);
nothing of the metric but the means over the finished tables runs on the host, and without the library or a GPU the call fails.
"""
import argparse

from . import evaluate as E


def build_parser():
    parser = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    parser.add_argument('--gt', required=True, help='ground-truth COCO json')
    parser.add_argument('--dt', default='submission.json', help='detection json: [{image_id, category_id, bbox [x, y, w, h], score}]')
    parser.add_argument('--dt-images', action='store_true', help='only the images that have at least one detection take part')
    parser.add_argument('--catId', type=lambda s: [int(v) for v in s.split(',') if v], default=[], help="category ids of the summary, e.g. '1,2' (default: all)")
    parser.add_argument('--each-category', action='store_true', help='also print one row per category')
    return parser


def main(argv=None, coco_call=None, print_fn=print):
    """coco_call replaces the HIP call (tests: the restatement).  Returns the CocoResult."""
    args = build_parser().parse_args(argv)
    gt = E.pack_coco_ground_truth(args.gt)
    unknown = [c for c in args.catId if c not in gt['cat_ids']]
    if unknown:
        raise SystemExit('--catId %s: the ground truth defines %s' % (','.join(str(c) for c in unknown), gt['cat_ids']))
    result = E.evaluate_coco_sets(gt, [args.dt], dt_images=args.dt_images, cat_ids=args.catId or None, call=coco_call)[0]
    for line in result.lines():
        print_fn(line)
    if args.each_category:
        for line in result.table():
            print_fn(line)
    return result


if __name__ == '__main__':
    main()
