"""Cost and effect of suppressing duplicate tracks across classes next to producing and deduplicating the result (recorded in
profiles/track_xclass.txt; not a gate).

    python tools/xclass_bench.py [--segments 8] [--frames 198] [--objects 100] [--out profiles/track_xclass.txt]

On the config-1 size input of tools/dedup_bench.py (8 segments x 5 cameras x 198 frames; SYNTHETIC detections), with a second,
lower-scored detection of ANOTHER class inside every third object-sized box - the pedestrian box on the rider of a bicycle, the
second box on a large vehicle - in ONE run on the same input:
  (a) wt_xclass_tracks_dev for J = 1 and J = 64 jobs on one tracked result, device events around repeated calls (inputs resident
      in HBM; the call never waits for the stream), with the workspace, the rows and trajectories dropped and the sweeps of the
      matching;
  (b) wt_dedup_tracks_dev J = 1 on the same result;
  (c) utils.track_packed on the same detections (wt_track_streams_host, staging included), wall clock;
  (d) fp and MOTA, ALL and per class, of the result before and after the pass.
"""
import argparse
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

OTHER = {1: 2, 2: 4, 4: 2}                    # the class of the second box: a pedestrian in a vehicle or a cyclist, a cyclist in a pedestrian


def with_other_class_boxes(dets, every=3, factor=0.9):
    """a second detection of another class on the middle half (in x) of every `every`-th box at least 24 px wide, at `factor` of its score"""
    extra, n = [], 0
    for e in dets:
        if e['bbox'][2] >= 24 and e['category_id'] in OTHER:
            n += 1
            if n % every == 0:
                x, y, w, h = e['bbox']
                extra.append(dict(e, bbox=[x + 0.25 * w, y, 0.5 * w, h], category_id=OTHER[e['category_id']], score=e.get('score', 1.0) * factor))
    return list(dets) + extra, len(extra)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--segments', type=int, default=8)
    ap.add_argument('--frames', type=int, default=198)
    ap.add_argument('--objects', type=int, default=100)
    ap.add_argument('--repeats', type=int, default=20)
    ap.add_argument('--rounds', type=int, default=5)
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'track_xclass.txt'))
    args = ap.parse_args()
    import numpy as np
    import torch
    assert torch.cuda.is_available(), 'needs the GPU'
    from waymo_2d_tracking_amd import _lib, synthetic as syn
    from waymo_2d_tracking_amd.tracking import dedup as D, evaluate as E, utils as T, xclass as X
    lines = []

    def say(text):
        print(text, flush=True)
        lines.append(text)

    dets, gt_json = syn.make_tracking_json(1, n_segments=args.segments, n_frames=args.frames, n_objects=args.objects)
    dets, n_extra = with_other_class_boxes(dets)
    predictions = {}
    for e in dets:
        seg, fr, cam = e['image_id'].split('/')
        predictions.setdefault(seg, {}).setdefault(cam, {}).setdefault(int(fr), []).append(
            {'bbox': e['bbox'], 'score': e['score'], 'category_id': e['category_id']})
    packed = T.pack_streams(predictions)
    gt = E.load_ground_truth(gt_json)
    say('device: %s' % (_lib.device_info(),))
    say('input (SYNTHETIC, waymo_2d_tracking_amd.synthetic seed 1): %d segments x 5 cameras x %d frames, %d detections (%d of them injected '
        'other-class detections inside every third box), %d ground-truth boxes, %d streams'
        % (args.segments, args.frames, packed['x'].size, n_extra, gt['x'].size, len(gt['stream_keys'])))

    def events(fn):
        """median, min, max over `rounds` windows of `repeats` calls each, in ms per call"""
        for _ in range(3):
            fn()
        torch.cuda.synchronize()
        per_call = []
        for _ in range(args.rounds):
            start, stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            start.record()
            for _ in range(args.repeats):
                fn()
            stop.record()
            stop.synchronize()
            per_call.append(start.elapsed_time(stop) / args.repeats)
        return float(np.median(per_call)), min(per_call), max(per_call)

    every = lambda v: dict(((a, b), v) for a in (1, 2, 4) for b in (1, 2, 4) if a < b)
    one = [{'pairs': every({'frames': 3, 'overlap': 0.7, 'frac': 0.5}), 'prio': 0, 'measure': 'iomin'}]
    many = [{'pairs': every({'frames': f, 'overlap': v, 'frac': 0.5}), 'prio': 0, 'measure': m}
            for f in range(1, 9) for v in (0.5, 0.7, 0.8, 0.9) for m in ('iomin', 'iou')]
    for label, flags in (('max_age 1, score >= 0.3', (1, 0, [0.3] * 4, [0.01] * 4)),
                         ('reference flags, max_age 2', (2, 0, [0.95, 0.6, 1.0, 0.9], [0.01, 0.01, 1.0, 0.0]))):
        T.track_packed(packed, flags[3], flags[0], flags[1], flags[2])
        times = []
        for _ in range(7):
            t0 = time.perf_counter()
            out, _ = T.track_packed(packed, flags[3], flags[0], flags[1], flags[2])
            times.append(time.perf_counter() - t0)
        say('%s:' % label)
        say('(c) track_packed (host call, staging included): median %.2f ms of 7 (min %.2f, max %.2f), %d rows'
            % (1e3 * float(np.median(times)), 1e3 * min(times), 1e3 * max(times), len(out['frame'])))
        dd = D.DeviceDedup(packed, [out], [{'min_frames': 3, 'dup_iou': 0.7, 'dup_frac': 0.5}])
        say('(b) wt_dedup_tracks_dev J = 1 (min_frames 3, dup_iou 0.7, dup_frac 0.5): median %.3f ms per call (min %.3f, max %.3f), %d trajectories dropped'
            % (events(dd.launch) + (int(dd.results()[0]['n_dropped'].sum()),)))
        for jobs, what in ((one, 'pairs 1:2, 1:4, 2:4, frames 3, overlap 0.7, frac 0.5, iomin'),
                           (many, 'the three pairs, frames 1..8 x overlap 0.5, 0.7, 0.8, 0.9 x iomin, iou')):
            dev = X.DeviceXClass(packed, [out], jobs)
            ms, lo, hi = events(dev.launch)
            res = dev.results()
            sweeps = dev.rounds()
            J = len(jobs)
            gone = [int(r['n_dropped'].sum()) for r in res]
            rows_gone = [len(out['frame']) - len(r['frame']) for r in res]
            say('(a) wt_xclass_tracks_dev J = %d (%s): median %.3f ms per call = %.3f ms per job (min %.3f, max %.3f; %d windows of %d calls), '
                '%d rows, %d trajectories, most in one stream %d, workspace %.1f MiB, trajectories dropped per job %d .. %d, rows dropped per job %d .. %d, '
                'sweeps of the matching per (job, stream) %d .. %d'
                % (J, what, ms, ms / J, lo, hi, args.rounds, args.repeats, dev.p['n_rows'], dev.p['n_traj_total'], dev.max_traj,
                   dev.ws_bytes / 2.0 ** 20, min(gone), max(gone), min(rows_gone), max(rows_gone), int(sweeps.min()), int(sweeps.max())))
            if J == 1:
                tracks = [E.tracks_from_packed(packed, out), E.tracks_from_packed(packed, res[0])]
                mot = E.evaluate_tracks(gt, tracks)
                say('(d) %d of %d trajectories dropped, %d of %d rows; LEVEL_2 before -> after the pass:'
                    % (gone[0], dev.p['n_traj_total'], rows_gone[0], len(out['frame'])))
                for c in ('ALL',) + tuple(E.ALL_CLASSES):
                    a, b = mot[0].table[c][2], mot[1].table[c][2]
                    say('    class %-3s fp %d -> %d, tp %d -> %d, idsw %d -> %d, MOTA %.5f -> %.5f' % (c, a['fp'], b['fp'], a['tp'], b['tp'], a['idsw'], b['idsw'], a['MOTA'], b['MOTA']))
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, 'wt') as fp:
        fp.write('\n'.join(lines) + '\n')


if __name__ == '__main__':
    main()
