"""Cost of refining a tracking result next to producing it and next to scoring it (recorded in profiles/track_refine.txt; not a gate).

    python tools/refine_bench.py [--segments 8] [--frames 198] [--objects 100] [--out profiles/track_refine.txt]

On the config-1 size of tools/mot_eval_bench.py (8 segments x 5 cameras x 198 frames), in ONE run on the same input:
  (a) wt_refine_tracks_plan_dev + wt_refine_tracks_emit_dev for J = 1 and J = 64 jobs on one tracked result, device events
      around repeated plan + emit pairs (inputs resident in HBM; emit waits for the stream once, to read the planned size);
  (b) wt_mot_eval_dev on the same result;
  (c) utils.track_packed on the same detections (wt_track_streams_host, staging included), wall clock.
The expectation to report against: refining a result costs less than tracking it, (a, J = 1) < (c).
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
    ap.add_argument('--rounds', type=int, default=5)
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'track_refine.txt'))
    args = ap.parse_args()
    import numpy as np
    import torch
    assert torch.cuda.is_available(), 'needs the GPU'
    from waymo_2d_tracking_amd import _lib, synthetic as syn
    from waymo_2d_tracking_amd.tracking import evaluate as E, refine as R, utils as T
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

    verdicts = []
    for label, flags in (('max_age 3, score >= 0.3', (3, 0, [0.3] * 4, [0.01] * 4)),
                         ('reference flags, max_age 2', (2, 0, [0.95, 0.6, 1.0, 0.9], [0.01, 0.01, 1.0, 0.0]))):
        T.track_packed(packed, flags[3], flags[0], flags[1], flags[2])
        times = []
        for _ in range(7):
            t0 = time.perf_counter()
            out, _ = T.track_packed(packed, flags[3], flags[0], flags[1], flags[2])
            times.append(time.perf_counter() - t0)
        t_track = 1e3 * float(np.median(times))
        say('%s:' % label)
        say('(c) track_packed (host call, staging included): median %.2f ms of 7 (min %.2f, max %.2f), %d rows'
            % (t_track, 1e3 * min(times), 1e3 * max(times), len(out['frame'])))
        ms_one = None
        for jobs, what in (([{'max_gap': 2, 'min_len': 3}], 'max_gap 2, min_len 3'),
                           ([{'max_gap': g, 'min_len': n} for g in range(8) for n in range(1, 9)], 'max_gap 0..7 x min_len 1..8')):
            dev = R.DeviceRefine(packed, [out], jobs)

            def both():
                dev.launch()
                dev.emit()
            ms, lo, hi = events(both)
            ms_plan = events(dev.launch)[0]
            rows = dev.job_row_offsets.cpu().numpy()
            res = dev.results()
            fills = sum(int((r['source'] < 0).sum()) for r in res)
            J = len(jobs)
            say('(a) wt_refine_tracks plan + emit J = %d (%s): median %.3f ms per pair = %.3f ms per job (min %.3f, max %.3f; %d windows of %d pairs; '
                'plan alone %.3f ms), %d problems, %d trajectories, most in one stream %d, workspace %.1f MiB, %d rows out, %d of them filled'
                % (J, what, ms, ms / J, lo, hi, args.rounds, args.repeats, ms_plan, J * dev.p['n_streams'], dev.n_traj_total, dev.max_traj,
                   dev.ws_bytes / 2.0 ** 20, int(rows[-1]), fills))
            if J == 1:
                ms_one = ms
                mot = E.DeviceEvaluation(gt, [E.tracks_from_packed(packed, out), E.tracks_from_packed(packed, res[0])])
                ms_mot = events(mot.launch)[0]
                before, after = mot.results()
                say('(b) wt_mot_eval_dev K = 2 (the result and its refinement): %.3f ms per launch = %.3f ms per result' % (ms_mot, ms_mot / 2))
                for name, r in (('tracked', before), ('refined', after)):
                    say('    %s, ALL LEVEL_2: %s' % (name, dict((k, r.table['ALL'][2][k]) for k in ('gt', 'tp', 'fn', 'fp', 'idsw', 'MOTA'))))
        verdicts.append('expectation "refining a result costs less than tracking it", %s, (a, J = 1) < (c): %s (%.3f ms vs %.2f ms)'
                        % (label, 'HOLDS' if ms_one < t_track else 'DOES NOT HOLD', ms_one, t_track))
    for v in verdicts:
        say(v)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, 'wt') as fp:
        fp.write('\n'.join(lines) + '\n')


if __name__ == '__main__':
    main()
