"""Cost of the trajectory coverage table (MT / PT / ML, fragmentations) next to the CLEAR-MOT scoring it reads and next to
producing the result (recorded in profiles/mot_coverage.txt; not a gate).

    python tools/mot_coverage_bench.py [--segments 8] [--frames 198] [--objects 100] [--out profiles/mot_coverage.txt]

On the config-1 size of tools/mot_eval_bench.py (8 segments x 5 cameras x 198 frames), in ONE run on the same input:
  (a) wt_mot_coverage_dev alone (the matches of an evaluation already in HBM) for K = 1, K = 64 and the dense result: device
      events around windows of repeated launches, median / min / max of the windows, the workspace, and the split between the
      clears + mark pass, the link pass and the walk pass from events the call records around them;
  (b) wt_mot_eval_dev for the same results, the same way;
  (c) utils.track_packed on the same detections (wt_track_streams_host, staging included), wall clock;
  (d) the ALL LEVEL_2 table before and after stitching at the setting of tools/stitch_bench.py, and after filling the gaps the
      links leave.
"""
import argparse
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--segments', type=int, default=8)
    ap.add_argument('--frames', type=int, default=198)
    ap.add_argument('--objects', type=int, default=100)
    ap.add_argument('--repeats', type=int, default=20)
    ap.add_argument('--rounds', type=int, default=7)
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'mot_coverage.txt'))
    args = ap.parse_args()
    import numpy as np
    import torch
    assert torch.cuda.is_available(), 'needs the GPU'
    from waymo_2d_tracking_amd import _lib, synthetic as syn
    from waymo_2d_tracking_amd.tracking import evaluate as E, utils as T
    lines = []

    def say(text):
        print(text, flush=True)
        lines.append(text)

    dets, gt_json = syn.make_tracking_json(1, n_segments=args.segments, n_frames=args.frames, n_objects=args.objects)
    predictions = {}
    for e in dets:
        seg, fr, cam = e['image_id'].split('/')
        predictions.setdefault(seg, {}).setdefault(cam, {}).setdefault(int(fr), []).append(
            {'bbox': e['bbox'], 'score': e['score'], 'category_id': e['category_id']})
    packed = T.pack_streams(predictions)
    gt = E.load_ground_truth(gt_json)
    say('device: %s' % (_lib.device_info(),))
    say('input: %d segments x 5 cameras x %d frames, %d detections, %d ground-truth boxes, %d streams'
        % (args.segments, args.frames, packed['x'].size, gt['x'].size, len(gt['stream_keys'])))

    def track(flags):
        T.track_packed(packed, flags[3], flags[0], flags[1], flags[2])
        times = []
        for _ in range(5):
            t0 = time.perf_counter()
            out, _ = T.track_packed(packed, flags[3], flags[0], flags[1], flags[2])
            times.append(time.perf_counter() - t0)
        return out, 1e3 * float(np.median(times)), 1e3 * min(times), 1e3 * max(times)

    def events(fn):
        """Median, min and max over the windows of the time of one call."""
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

    def passes(cov):
        """Median over single launches of the three intervals between the events the call records."""
        marks = [torch.cuda.Event(enable_timing=True) for _ in range(4)]
        for e in marks:
            e.record()
        torch.cuda.synchronize()
        split = []
        for _ in range(args.repeats):
            cov.launch(pass_events=marks)
            torch.cuda.synchronize()
            split.append([marks[i].elapsed_time(marks[i + 1]) for i in range(3)])
        return np.median(np.asarray(split), axis=0)

    verdicts = []

    def both(tracks, label, t_track=None):
        K = len(tracks)
        ev = E.DeviceEvaluation(gt, tracks)
        ms_ev = events(ev.launch)
        cov = E.DeviceCoverage(gt, tracks, evaluation=ev)          # the evaluation's matches lie in HBM: only the coverage kernels run
        ms_cov = events(cov.launch)
        mark, link, walk = passes(cov)
        r = cov.results()[0].table['ALL'][2]
        say('(a) wt_mot_coverage_dev K = %d%s: median %.3f ms per launch = %.4f ms per result (min %.3f, max %.3f; %d windows of %d launches), '
            '%d trajectories, %d result rows, workspace %.2f MiB'
            % (K, label, ms_cov[0], ms_cov[0] / K, ms_cov[1], ms_cov[2], args.rounds, args.repeats, cov.total_traj, cov.n_hyp, cov.ws_bytes / 2.0 ** 20))
        say('    passes (single launches, each waited for; median of %d): clears + mark %.3f ms, link %.3f ms, walk %.3f ms'
            % (args.repeats, mark, link, walk))
        say('    first result, ALL LEVEL_2: %s' % dict((k, r[k]) for k in ('traj', 'mt', 'pt', 'ml', 'frag', 'MT', 'ML')))
        say('(b) wt_mot_eval_dev     K = %d%s: median %.3f ms per launch = %.4f ms per result (min %.3f, max %.3f)'
            % (K, label, ms_ev[0], ms_ev[0] / K, ms_ev[1], ms_ev[2]))
        verdicts.append('expectation "coverage costs less than the CLEAR-MOT evaluation it reads", K = %d%s, (a) < (b): %s (%.3f ms vs %.3f ms%s)'
                        % (K, label.split(' (')[0], 'HOLDS' if ms_cov[0] < ms_ev[0] else 'DOES NOT HOLD', ms_cov[0], ms_ev[0],
                           '' if t_track is None else '; track_packed %.2f ms' % t_track))

    reference = (2, 0, [0.95, 0.6, 1.0, 0.9], [0.01, 0.01, 1.0, 0.0])           # the reference README's flags
    out, t_track, lo, hi = track(reference)
    say('(c) track_packed, reference flags (host call, staging included): median %.2f ms of 5 (min %.2f, max %.2f), %d rows' % (t_track, lo, hi, len(out['frame'])))
    both([E.tracks_from_packed(packed, out)], '', t_track)
    many = []
    for max_age in (1, 2):
        for min_hits in (0, 1):
            for score in (0.3, 0.5, 0.7, 0.9):
                for iou in (0.0, 0.01, 0.1, 0.3):
                    o, _ = T.track_packed(packed, [iou] * 4, max_age, min_hits, [score] * 4)
                    many.append(E.tracks_from_packed(packed, o))
    both(many, ' (4 score x 4 IoU thresholds x 2 max_age x 2 min_hits)')
    dense, t_dense, lo, hi = track((2, 0, [0.3] * 4, [0.01] * 4))
    say('(c) track_packed, dense result (score >= 0.3): median %.2f ms of 5 (min %.2f, max %.2f), %d rows' % (t_dense, lo, hi, len(dense['frame'])))
    both([E.tracks_from_packed(packed, dense)], ' dense', t_dense)
    for v in verdicts:
        say(v)

    # (d) what the table says about stitching (tools/stitch_bench.py: max_age 1, score >= 0.3; max_link 5, link_iou 0.3, linear)
    from waymo_2d_tracking_amd.tracking.refine import refine_tracks
    from waymo_2d_tracking_amd.tracking.stitch import stitch_tracks
    tracked, _ = T.track_packed(packed, [0.01] * 4, 1, 0, [0.3] * 4)
    stitched = stitch_tracks(packed, [tracked], [{'max_link': 5, 'link_iou': 0.3, 'motion': 'linear'}], 4)[0]
    filled = refine_tracks(packed, [stitched], [{'max_gap': 5, 'min_len': 1, 'result': 0}], 4)[0]
    tracks = [E.tracks_from_packed(packed, o) for o in (tracked, stitched, filled)]
    p = E.pack_results(gt, tracks, 4)
    cov = E.evaluate_coverage(gt, tracks, packed=p)
    mot = E.evaluate_tracks(gt, tracks, packed=p)
    say('(d) ALL LEVEL_2, max_age 1, score >= 0.3: tracked -> stitched (max_link 5, link_iou 0.3, linear) -> gaps of up to 5 frames filled:')
    for name, c, m in zip(('tracked ', 'stitched', 'filled  '), cov, mot):
        r = c.table['ALL'][2]
        say('    %s traj %d, mt %d, pt %d, ml %d, MT %.5f, ML %.5f, FM %d, idsw %d, MOTA %.5f'
            % (name, r['traj'], r['mt'], r['pt'], r['ml'], r['MT'], r['ML'], r['FM'], m.table['ALL'][2]['idsw'], m.table['ALL'][2]['MOTA']))
    fm = [c.table['ALL'][2]['FM'] for c in cov]
    say('    FM after stitching alone: %s (stitching renames rows, it adds none); after filling the linked gaps: %s'
        % ('falls' if fm[1] < fm[0] else 'does not fall', 'falls' if fm[2] < fm[0] else 'does not fall'))
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, 'wt') as fp:
        fp.write('\n'.join(lines) + '\n')


if __name__ == '__main__':
    main()
