"""The tracking sweep by the host route and with the rows resident in HBM (recorded in profiles/sweep_chain.txt; not a gate).

    python tools/sweep_chain_bench.py [--segments 8] [--frames 198] [--objects 100] [--repeats 3] [--out profiles/sweep_chain.txt]

On the config-1 size of tools/refine_bench.py (8 segments x 5 cameras x 198 frames) and a grid of 4 tracked points x 6 refinement
jobs, in ONE run on the same files:
  (a) wall time of evaluate.sweep() by the host route - the yardstick: the code path as it was - and with device_chain=True,
      alternating, after a warm-up of both on a small set; and of what both share, reading and packing the detections;
  (b) device-event time of the chain's stages per sweep: the trackers, wt_tracks_layout_dev, refine plan + emit,
      wt_tracks_to_eval_dev, wt_mot_eval_dev;
  (c) the bytes each route moves between host and device (sum of the arrays copied), and the peak of the chain's buffers.
No ratio is fixed in advance; the file states both numbers and says which route was faster.
"""
import argparse
import json
import os
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

GRID = {'score': [0.3, 0.6], 'iou': [0.01], 'max_age': [1, 3], 'min_hits': [0], 'gap': [0, 1, 2], 'min_len': [1, 2]}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--segments', type=int, default=8)
    ap.add_argument('--frames', type=int, default=198)
    ap.add_argument('--objects', type=int, default=100)
    ap.add_argument('--repeats', type=int, default=3)
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'sweep_chain.txt'))
    args = ap.parse_args()
    import numpy as np
    import torch
    assert torch.cuda.is_available(), 'needs the GPU'
    from waymo_2d_tracking_amd import _lib, synthetic as syn
    from waymo_2d_tracking_amd.tracking import chain as CH, evaluate as E, utils as T
    lines = []

    def say(text):
        print(text, flush=True)
        lines.append(text)

    def files(directory, name, **kw):
        dets, gt_json = syn.make_tracking_json(1, **kw)
        path = os.path.join(directory, name)
        with open(path, 'wt') as fp:
            json.dump(dets, fp)
        return path, E.load_ground_truth(gt_json)

    def same(a, b):
        return (a['settings'] == b['settings'] and json.dumps(a['ranked'], sort_keys=True) == json.dumps(b['ranked'], sort_keys=True) and
                all(x.counts.tobytes() == y.counts.tobytes() and x.iou_sum.tobytes() == y.iou_sum.tobytes() and x.ignored_rows == y.ignored_rows
                    for x, y in zip(a['results'], b['results'])))

    with tempfile.TemporaryDirectory() as tmp:
        small, small_gt = files(tmp, 'small.json', n_segments=1, n_frames=12, n_objects=12)
        assert same(E.sweep(small, small_gt, GRID), E.sweep(small, small_gt, GRID, device_chain=True))      # the warm-up, and the two routes agree
        path, gt = files(tmp, 'det.json', n_segments=args.segments, n_frames=args.frames, n_objects=args.objects)
        say('device: %s' % (_lib.device_info(),))
        times = {'host': [], 'chain': [], 'read': []}
        last = {}
        for _ in range(args.repeats):
            t0 = time.perf_counter()
            packed = T.pack_streams(E._detections(path))
            times['read'].append(time.perf_counter() - t0)
            for route, flag in (('host', False), ('chain', True)):
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                last[route] = E.sweep(path, gt, GRID, device_chain=flag)
                torch.cuda.synchronize()
                times[route].append(time.perf_counter() - t0)
        settings, plans = E.sweep_settings(GRID)
        points = [a for _, a in E._tracked_points(GRID, plans['second'])]
        say('input: %d segments x 5 cameras x %d frames, %d detections, %d ground-truth boxes, %d streams; grid: %d tracked points x %d refinement jobs = %d settings'
            % (args.segments, args.frames, packed['x'].size, gt['x'].size, len(gt['stream_keys']), len(points), len(plans['refine'].jobs), len(settings)))
        say('the two routes give the same settings, count tables, iou_sum bits, ignored rows and ranking: %s' % same(last['host'], last['chain']))
        med = dict((k, float(np.median(v))) for k, v in times.items())
        for route, what in (('host', 'sweep(), host route'), ('chain', 'sweep(device_chain=True)'), ('read', 'reading and packing the detections (inside both)')):
            say('(a) %-50s median %.2f s of %d (min %.2f, max %.2f)' % (what + ':', med[route], args.repeats, min(times[route]), max(times[route])))
        say('    without the shared reading: host route %.2f s, chain %.2f s' % (med['host'] - med['read'], med['chain'] - med['read']))
        # (b), (c): the chain once more with events around its stages
        ch = CH.DeviceChain(packed, gt, 4, E.DEFAULT_IOU_THRESHOLD)
        ch.record_events = True
        ch.run(points, plans['refine'].jobs)
        torch.cuda.synchronize()
        stages = ('track', 'layout', 'refine', 'to_eval', 'mot_eval')
        total = dict((s, sum(a.elapsed_time(b) for marks in ch.events for a, b in marks.get(s, []))) for s in stages)
        say('(b) device events per sweep, %d round(s) of at most %d tracked point(s): %s'
            % (ch.rounds, ch.points_per_round(len(plans['refine'].jobs)), ', '.join('%s %.2f ms' % (s, total[s]) for s in stages)))
        say('    (track = %d tracker launches; layout = wt_tracks_layout_dev; refine = plan + emit, the emit waits once for the planned size; '
            'to_eval = wt_tracks_to_eval_dev; mot_eval = wt_mot_eval_dev)' % len(points))
        n_dets, tracked, scored, J = int(packed['x'].size), sum(ch.tracked_rows), sum(ch.scored_rows), len(plans['refine'].jobs)
        dets_bytes = sum(int(np.asarray(packed[k]).nbytes) for k in ('x', 'y', 'w', 'h', 'score', 'category', 'frame_det_offsets', 'stream_frame_offsets', 'clip_w', 'clip_h'))
        gt_bytes = sum(int(np.asarray(gt[k]).nbytes) for k in ('x', 'y', 'w', 'h', 'category', 'level', 'gt_id', 'frame_gt_offsets', 'stream_frame_offsets'))
        # host route: per tracked point the detections up and its rows (60 B) down; the refinement takes them up as 48 B columns and
        # gives every job's rows (72 B) back; the metric takes every scored row up as 40 B and gives hyp_match (8 B) back
        host_bytes = len(points) * dets_bytes + 60 * tracked + 48 * tracked + 72 * scored + gt_bytes + 40 * scored + 8 * scored
        say('(c) bytes between host and device per sweep: host route %.1f MiB (%d tracked rows, %d scored rows; offsets and count tables left out), '
            'chain %.3f MiB (detections and ground truth once, pointer tables, job arrays, scalars, count tables)'
            % (host_bytes / 2.0 ** 20, tracked, scored, ch.copied_bytes / 2.0 ** 20))
        say('    peak of the chain\'s buffers in one round: %.1f MiB (limit %.0f MiB)' % (ch.peak_bytes / 2.0 ** 20, ch.limit / 2.0 ** 20))
        faster = med['chain'] < med['host']
        say('verdict: the chain is %s than the host route on this input: %.2f s against %.2f s (%.2fx); without the shared reading %.2f s against %.2f s'
            % ('FASTER' if faster else 'NOT FASTER', med['chain'], med['host'], med['host'] / med['chain'], med['chain'] - med['read'], med['host'] - med['read']))
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, 'wt') as fp:
        fp.write('\n'.join(lines) + '\n')


if __name__ == '__main__':
    main()
