"""Drop-in for /root/reference/tracking/track.py (same flags, same prints, same output JSON):

    python -m waymo_2d_tracking_amd.tracking.track --input det.json --output tracks.json \
        --max-age=2 --min-hits=0 --score-threshold=0.95,0.6,1.0,0.9

All (segment, camera) streams are tracked in one GPU call (utils.track_all) instead of the sequential loop of
track.py:43-47; `--ground-truth` is accepted but, like in the reference, its content is never used (the file
is not required to exist).

Beyond the reference: `--low-score-threshold=0.3,0.3,1.0,0.3 [--low-iou-threshold 0.5]` lets detections between the two score
thresholds continue tracks that no detection above `--score-threshold` matched (second association; one
process only), and the post-passes of split.py, stitch.py, xlink.py, dedup.py, xclass.py, refine.py and smooth.py follow when their
flags ask for them.
"""
import argparse
import importlib
import json
import time

import os

from .utils import read_data_file, track_all


def _floats(s):
    return [float(item) for item in s.split(',')]


def _ints(s):
    return [int(item) for item in s.split(',')]


def _pairs(s):
    return [tuple(int(c) for c in item.split(':')) for item in s.split(',')]


def build_parser():
    parser = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.ArgumentDefaultsHelpFormatter)
    parser.add_argument("--ground-truth", type=str, default='/data/waymo/det2d/validation/images.json',
                        help='ground-truth json')
    parser.add_argument("--input", type=str, default='submission_12545.json', help='submission.json')
    parser.add_argument("--output", type=str, default='tracker_predictions.json',
                        help='file to save the tracker predictions')
    parser.add_argument("--max-age", type=int, default=1, help='SORT max-age')
    parser.add_argument("--min-hits", type=int, default=0, help='SORT min-hits')
    parser.add_argument("--score-threshold", type=_floats, default=[0.95, 0.6, 1.0, 0.9],
                        help='score threshold to track')
    parser.add_argument("--iou-threshold", type=_floats, default=[0.01, 0.01, 1.0, 0.0],
                        help='IOU threshold for tracking')
    parser.add_argument("--interpolate-gap", type=_ints, default=[0],
                        help='fill gaps of up to this many frames inside a track by linear interpolation (one value, or one per class)')
    parser.add_argument("--min-track-len", type=_ints, default=[1],
                        help='drop tracks observed in fewer frames than this (one value, or one per class)')
    parser.add_argument("--track-score", choices=('keep', 'mean'), default='keep',
                        help='mean: every box of a track carries the mean score of its observed boxes')
    parser.add_argument("--split-iou", type=_floats, default=[0.0],
                        help='split tracks: cut a track between two consecutive boxes when the boxes extrapolated from the frames before AND after them '
                             'overlap the other side by less than this IoU (one value, or one per class; 0 = off)')
    parser.add_argument("--split-gap", type=_ints, default=[0],
                        help='split tracks: cut a track where more than this many frames lie between two consecutive boxes (one value, or one per class; 0 = off)')
    parser.add_argument("--split-motion", choices=('linear', 'hold'), default='linear',
                        help='how a box is extrapolated for --split-iou: moved on by the step next to it, or held')
    parser.add_argument("--link-gap", type=_ints, default=[0],
                        help='stitch tracks: link a track that ends to one of its class that starts up to this many frames later (one value, or one per class)')
    parser.add_argument("--link-iou", type=_floats, default=[0.3],
                        help='lowest IoU of the ended track\'s extrapolated box and the new track\'s first box (one value, or one per class); read when --link-gap is set')
    parser.add_argument("--link-motion", choices=('hold', 'linear'), default='hold',
                        help='how the ended track is extrapolated over the gap: its last box, or moved on by its last step')
    parser.add_argument("--dedup-frames", type=_ints, default=[0],
                        help='suppress duplicate tracks: a track is dropped when a stronger one of its class overlaps it in at least this many frames '
                             '(one value, or one per class; 0 = off)')
    parser.add_argument("--dedup-iou", type=_floats, default=[0.7],
                        help='lowest IoU of the two tracks\' boxes in a frame that counts (one value, or one per class); read when --dedup-frames is set')
    parser.add_argument("--dedup-frac", type=_floats, default=[0.5],
                        help='lowest share of the shorter track\'s frames that must count (one value, or one per class); read when --dedup-frames is set')
    parser.add_argument("--xclass-pairs", type=_pairs, default=None,
                        help='suppress duplicate tracks across classes: the class pairs that are compared, as 2:4,1:4 (absent = off); a track is '
                             'dropped when a stronger one of the other class overlaps it in enough frames')
    parser.add_argument("--xclass-frames", type=_ints, default=[3],
                        help='lowest number of frames in which the two tracks\' boxes overlap (one value, or one per listed pair; 0 = the pair is off)')
    parser.add_argument("--xclass-overlap", type=_floats, default=[0.7],
                        help='lowest overlap of the two tracks\' boxes in a frame that counts (one value, or one per listed pair)')
    parser.add_argument("--xclass-frac", type=_floats, default=[0.5],
                        help='lowest share of the weaker track\'s frames that must count (one value, or one per listed pair)')
    parser.add_argument("--xclass-measure", choices=('iou', 'iomin'), default='iomin',
                        help='the overlap of two boxes: intersection over union, or over the smaller area (a rider box inside a cyclist box)')
    parser.add_argument("--xclass-prio", type=_ints, default=[0],
                        help='class priority, one int per class: of two overlapping tracks the one of the higher priority stays, whatever their lengths')
    parser.add_argument("--xlink-pairs", type=_pairs, default=None,
                        help='repair class flicker: the class pairs across which a track that ends is linked to one that starts, as 2:4,1:2 '
                             '(a:a = inside a class; absent = off); the linked rows take one id and the class most of them have')
    parser.add_argument("--xlink-gap", type=_ints, default=[1],
                        help='link up to this many frames later (one value, or one per listed pair; 0 = the pair is off)')
    parser.add_argument("--xlink-iou", type=_floats, default=[0.3],
                        help='lowest IoU of the ended track\'s extrapolated box and the new track\'s first box (one value, or one per listed pair)')
    parser.add_argument("--xlink-motion", choices=('hold', 'linear'), default='hold',
                        help='how the ended track is extrapolated over the gap: its last box, or moved on by its last step')
    parser.add_argument("--xlink-prio", type=_ints, default=[0],
                        help='class priority, one int per class: decides the class of linked rows when two classes have equally many')
    parser.add_argument("--smooth-window", type=_ints, default=[0],
                        help='smooth tracks: every box becomes the weighted mean of its track\'s boxes up to this many frames to either side, '
                             'both sides or neither (one value, or one per class)')
    parser.add_argument("--smooth-sigma", type=_floats, default=[1.0],
                        help='width of the gaussian weights in frames (one value, or one per class); read when --smooth-window is set')
    parser.add_argument("--smooth-kernel", choices=('gaussian', 'box'), default='gaussian',
                        help='the weights over the window: exp(-d^2 / (2 sigma^2)), or all equal')
    parser.add_argument("--low-score-threshold", type=_floats, default=None,
                        help='second association: detections from this score on (one value per class, none above --score-threshold) may continue '
                             'a track that no detection above --score-threshold matched; they never start one (absent = off)')
    parser.add_argument("--low-iou-threshold", type=_floats, default=[0.5],
                        help='lowest IoU of a low-score detection and the track it continues (one value, or one per class); '
                             'read when --low-score-threshold is set')
    parser.add_argument("--segment-id", type=str, help='track only a single segment')
    parser.add_argument("--python-io", action='store_true',
                        help='parse / write JSON with the Python json module (default: native reader / writer of libwaymotrack)')
    return parser


def refines(args):
    """Whether the flags ask for any refinement (tracking/refine.py); with the defaults the output is the tracker's own."""
    return max(args.interpolate_gap) > 0 or max(args.min_track_len) > 1 or args.track_score != 'keep'


def splits(args):
    """Whether the flags ask for splitting (tracking/split.py)."""
    return max(args.split_iou) > 0 or max(args.split_gap) > 0


def stitches(args):
    """Whether the flags ask for stitching (tracking/stitch.py)."""
    return max(args.link_gap) > 0


def dedups(args):
    """Whether the flags ask for the suppression of duplicate tracks (tracking/dedup.py)."""
    return max(args.dedup_frames) > 0


def _per_pair(values, flag, n):
    if len(values) not in (1, n):
        raise SystemExit('%s needs one value, or one per listed pair (%d)' % (flag, n))
    return list(values) * n if len(values) == 1 else list(values)


def xclass_pairs(args):
    """The pairs of tracking/xclass.py that the flags switch on: {(a, b): {'frames', 'overlap', 'frac'}}; empty = the pass is off."""
    if not args.xclass_pairs:
        return {}
    n = len(args.xclass_pairs)
    if any(len(pair) != 2 for pair in args.xclass_pairs):
        raise SystemExit('--xclass-pairs takes pairs of classes, as 2:4,1:4')
    per_pair = lambda values, flag: _per_pair(values, flag, n)
    frames, overlap, frac = per_pair(args.xclass_frames, '--xclass-frames'), per_pair(args.xclass_overlap, '--xclass-overlap'), per_pair(args.xclass_frac, '--xclass-frac')
    return dict((pair, {'frames': f, 'overlap': o, 'frac': q}) for pair, f, o, q in zip(args.xclass_pairs, frames, overlap, frac) if f > 0)


def xclasses(args):
    """Whether the flags ask for the suppression of duplicate tracks across classes (tracking/xclass.py)."""
    return bool(xclass_pairs(args))


def xlink_pairs(args):
    """The pairs of tracking/xlink.py that the flags switch on: {(a, b): {'max_link', 'link_iou'}}; empty = the pass is off."""
    if not args.xlink_pairs:
        return {}
    n = len(args.xlink_pairs)
    if any(len(pair) != 2 for pair in args.xlink_pairs):
        raise SystemExit('--xlink-pairs takes pairs of classes, as 2:4,1:2')
    gaps, ious = _per_pair(args.xlink_gap, '--xlink-gap', n), _per_pair(args.xlink_iou, '--xlink-iou', n)
    return dict((pair, {'max_link': g, 'link_iou': v}) for pair, g, v in zip(args.xlink_pairs, gaps, ious) if g > 0)


def xlinks(args):
    """Whether the flags ask for linking across classes (tracking/xlink.py)."""
    return bool(xlink_pairs(args))


def smooths(args):
    """Whether the flags ask for smoothing (tracking/smooth.py)."""
    return max(args.smooth_window) > 0


def _stage(name):
    return importlib.import_module('.' + name, __package__)


def _split(args, packed, out, n_classes):
    from . import utils as T
    # the tracker writes the id counter + 1 for a birth; so does a new piece
    out = _stage('split').split_one(packed, out, args.split_iou, args.split_gap, args.split_motion, T._GLOBAL_IDS['next'] + 1, n_classes)
    T._GLOBAL_IDS['next'] += out['n_new']
    return out


# (whether the flags ask for the pass, what runs it - its module is imported then), in the order of the chain: splitting first, so
# that the pieces of an impure track can be linked to the tracks they belong to - a new piece takes the next id of the tracker's
# counter, as a birth does; then stitching, so that a merged track is length-filtered and gap-filled as one; then the suppression
# of duplicates, which judges a stitched track at its full length and leaves gap filling and the length filter the survivors only -
# inside a class first, then across the class pairs that are switched on; smoothing last, so that filled rows are smoothed too
PASSES = (
    (splits, _split),
    (stitches, lambda args, packed, out, n: _stage('stitch').stitch_one(packed, out, args.link_gap, args.link_iou, args.link_motion, n)),
    (dedups, lambda args, packed, out, n: _stage('dedup').dedup_one(packed, out, args.dedup_frames, args.dedup_iou, args.dedup_frac, n)),
    (xclasses, lambda args, packed, out, n: _stage('xclass').xclass_one(packed, out, xclass_pairs(args), args.xclass_prio, args.xclass_measure, n)),
    (refines, lambda args, packed, out, n: _stage('refine').refine_one(packed, out, args.interpolate_gap, args.min_track_len, args.track_score, n)),
    (smooths, lambda args, packed, out, n: _stage('smooth').smooth_one(packed, out, args.smooth_window, args.smooth_sigma, args.smooth_kernel, n)))


# The chain that runs: PASSES with the linking across classes between stitching and deduplication - after the stitching, so that
# a piece is first joined to its own class where it can be and the vote sees whole tracks, and before the suppression of
# duplicates, which then judges a repaired track at its full length and in its voted class.  Off unless --xlink-pairs is given.
CHAIN = PASSES[:2] + (
    (xlinks, lambda args, packed, out, n: _stage('xlink').xlink_one(packed, out, xlink_pairs(args), args.xlink_prio, args.xlink_motion, n)),
) + PASSES[2:]


def refined(args, packed, out):
    """The tracker's rows after the post-passes the flags ask for, in the order of CHAIN."""
    for asked, run in CHAIN:
        if asked(args):
            out = run(args, packed, out, len(args.iou_threshold))
    return out


post_passes = refined


def second_association(args):
    """Whether the flags ask for the second association with low-score detections (utils.track_packed_byte)."""
    return args.low_score_threshold is not None


def read_threshold(args):
    """The score thresholds the detections file is read with: the low ones when the second association is on."""
    return args.low_score_threshold if second_association(args) else args.score_threshold


def tracked_byte(args, packed):
    """The tracker's rows with the second association; the id counter moves on as in track_all."""
    from . import utils as T
    out, births = T.track_packed_byte(packed, args.iou_threshold, args.max_age, args.min_hits, args.score_threshold,
                                      args.low_score_threshold, args.low_iou_threshold, T._GLOBAL_IDS['next'])
    T._GLOBAL_IDS['next'] += births
    return out


def main_native(args):
    """file -> SoA in HBM -> file without per-row Python objects (wt_detfile_read / wt_tracks_write_json)."""
    from . import utils as T
    nat = T.NativeDetFile(args.input, read_threshold(args))
    packed = nat.packed()
    start_time = time.time()
    for segment_id in dict.fromkeys(s for s, _ in packed['stream_keys']):
        print(segment_id)
    if second_association(args):
        out = tracked_byte(args, packed)
    else:
        out, births = T.track_packed(packed, args.iou_threshold, args.max_age, args.min_hits, None, T._GLOBAL_IDS['next'])
        T._GLOBAL_IDS['next'] += births
    print("duration: %.2fs" % (time.time() - start_time))
    nat.write_tracks(args.output, refined(args, packed, out))
    nat.close()
    return 0


def main_sharded(args, world, rank):
    """torchrun: one process per GPU.  Every rank parses the file natively, tracks its block of streams and the result
    columns reach rank 0 through one tensor gather (distributed.track_packed_sharded); rank 0 writes the JSON natively."""
    import torch
    import torch.distributed as dist
    from . import utils as T
    from ..distributed import track_packed_sharded
    backend = os.environ.get('WT_DIST_BACKEND', 'nccl')
    if backend == 'nccl':
        torch.cuda.set_device(int(os.environ.get('LOCAL_RANK', '0')))
    dist.init_process_group(backend)
    nat = T.NativeDetFile(args.input, args.score_threshold)
    packed = nat.packed()
    if args.segment_id:
        keep = [i for i, (s, _) in enumerate(packed['stream_keys']) if s == args.segment_id]
        packed = T.slice_streams(packed, keep[0], keep[-1] + 1) if keep else T.slice_streams(packed, 0, 0)
    start_time = time.time()
    if rank == 0:
        for segment_id in dict.fromkeys(s for s, _ in packed['stream_keys']):
            print(segment_id)
    cols, births = track_packed_sharded(packed, args.iou_threshold, args.max_age, args.min_hits, None, None, T._GLOBAL_IDS['next'])
    T._GLOBAL_IDS['next'] += births
    if rank == 0:
        print("duration: %.2fs" % (time.time() - start_time))
        cols = refined(args, packed, cols)
        if args.segment_id:
            with open(args.output, 'wt') as fp:
                json.dump(T.format_tracks(packed, cols), fp)
        else:
            nat.write_tracks(args.output, cols)
    nat.close()
    dist.barrier()
    dist.destroy_process_group()
    return 0


def main(argv=None):
    args = build_parser().parse_args(argv)
    print(args)
    world = int(os.environ.get('WORLD_SIZE', '1'))
    rank = int(os.environ.get('RANK', '0'))
    if second_association(args):
        if world > 1:
            raise SystemExit('--low-score-threshold is not available under torchrun (world size %d): the second association '
                             'has no sharded form yet; run it in one process' % world)
        from .utils import per_class
        n_classes = len(args.iou_threshold)
        if len(args.score_threshold) != n_classes:
            raise SystemExit('--score-threshold and --iou-threshold need one value per class')
        args.low_score_threshold = per_class(args.low_score_threshold, n_classes, '--low-score-threshold')
        args.low_iou_threshold = per_class(args.low_iou_threshold, n_classes, '--low-iou-threshold')
    if world > 1:
        return main_sharded(args, world, rank)
    if not args.python_io and not args.segment_id:
        return main_native(args)
    predictions = read_data_file(args.input, read_threshold(args))
    if args.segment_id:
        predictions = {k: v for k, v in predictions.items() if k in [args.segment_id]}
    start_time = time.time()
    for segment_id in predictions.keys():
        print(segment_id)
    if second_association(args):
        from . import utils as T
        packed = T.pack_streams(predictions)
        tracked_predictions = T.format_tracks(packed, refined(args, packed, tracked_byte(args, packed)))
    elif any(asked(args) for asked, _ in CHAIN):
        from . import utils as T
        packed = T.pack_streams(predictions)
        out, births = T.track_packed(packed, args.iou_threshold, args.max_age, args.min_hits, None, T._GLOBAL_IDS['next'])
        T._GLOBAL_IDS['next'] += births
        tracked_predictions = T.format_tracks(packed, refined(args, packed, out))
    else:
        tracked_predictions = track_all(predictions, args.iou_threshold, args.max_age, args.min_hits)
    print("duration: %.2fs" % (time.time() - start_time))
    with open(args.output, 'wt') as fp:
        json.dump(tracked_predictions, fp)
    return 0


if __name__ == '__main__':
    raise SystemExit(main())
