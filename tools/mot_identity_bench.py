"""Cost of scoring identity preservation (IDF1) next to CLEAR-MOT scoring and next to producing the result
(recorded in profiles/mot_identity.txt; not a gate).

    python tools/mot_identity_bench.py [--segments 8] [--frames 198] [--objects 100] [--out profiles/mot_identity.txt]

On the config-1 size of tools/mot_eval_bench.py (8 segments x 5 cameras x 198 frames), in ONE run on the same input:
  (a) wt_mot_identity_dev for K = 1 and K = 64 results, device events around repeated launches (inputs resident in HBM),
      with the largest and mean n x m (trajectories a side) per problem;
  (b) wt_mot_eval_dev for the same K = 1 and K = 64;
  (c) utils.track_packed on the same detections (wt_track_streams_host, staging included), wall clock;
  (d) tests/mot_id_ref.py, the plain-Python restatement, on ONE segment of one result on one CPU thread (scaled to all).
Zero-row / zero-column compaction before the assignment is not built, so there is one identity time per K.
"""
import argparse
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tests'))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--segments', type=int, default=8)
    ap.add_argument('--frames', type=int, default=198)
    ap.add_argument('--objects', type=int, default=100)
    ap.add_argument('--repeats', type=int, default=20)
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'mot_identity.txt'))
    ap.add_argument('--no-cpu-reference', action='store_true')
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

    # (c) the tracker
    reference = (2, 0, [0.95, 0.6, 1.0, 0.9], [0.01, 0.01, 1.0, 0.0])           # the reference README's flags
    T.track_packed(packed, reference[3], reference[0], reference[1], reference[2])
    times = []
    for _ in range(5):
        t0 = time.perf_counter()
        out, _ = T.track_packed(packed, reference[3], reference[0], reference[1], reference[2])
        times.append(time.perf_counter() - t0)
    t_track = float(np.median(times))
    say('(c) track_packed (host call, staging included): median %.2f ms of 5 (min %.2f, max %.2f), %d rows'
        % (1e3 * t_track, 1e3 * min(times), 1e3 * max(times), len(out['frame'])))
    one = E.tracks_from_packed(packed, out)

    def time_dev(dev):
        for _ in range(3):
            dev.launch()
        torch.cuda.synchronize()
        start, stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        start.record()
        for _ in range(args.repeats):
            dev.launch()
        stop.record()
        stop.synchronize()
        return start.elapsed_time(stop) / args.repeats

    def sizes(dev):
        g = np.broadcast_to(dev.g_ntraj.astype(np.int64), dev.h_ntraj.shape)
        h = dev.h_ntraj.astype(np.int64)
        prod = (np.minimum(g, h) * np.maximum(g, h)).reshape(-1)
        i = int(np.argmax(prod))
        return int(np.minimum(g, h).reshape(-1)[i]), int(np.maximum(g, h).reshape(-1)[i]), float(prod.mean())

    def both(tracks, label):
        ident, mot = E.DeviceIdentity(gt, tracks), E.DeviceEvaluation(gt, tracks)
        ms_id, ms_mot = time_dev(ident), time_dev(mot)
        r = ident.results()[0].table['ALL'][2]
        n, m, mean = sizes(ident)
        K = len(tracks)
        say('(a) wt_mot_identity_dev K = %d%s: %.3f ms per launch = %.3f ms per result (events around %d launches), %d problems, '
            'workspace %.1f MiB; largest problem %d x %d trajectories, mean n x m %.0f'
            % (K, label, ms_id, ms_id / K, args.repeats, K * len(gt['stream_keys']) * 4, ident.ws_bytes / 2.0 ** 20, n, m, mean))
        say('    first result, ALL LEVEL_2: %s' % dict((k, r[k]) for k in ('idtp', 'idfn', 'idfp', 'idf1', 'idp', 'idr')))
        say('(b) wt_mot_eval_dev     K = %d%s: %.3f ms per launch = %.3f ms per result' % (K, label, ms_mot, ms_mot / K))
        return ms_id, ms_mot

    ms1, mot1 = both([one], '')
    many = []
    for max_age in (1, 2):
        for min_hits in (0, 1):
            for score in (0.3, 0.5, 0.7, 0.9):
                for iou in (0.0, 0.01, 0.1, 0.3):
                    o, _ = T.track_packed(packed, [iou] * 4, max_age, min_hits, [score] * 4)
                    many.append(E.tracks_from_packed(packed, o))
    ms64, mot64 = both(many, ' (4 score x 4 IoU thresholds x 2 max_age x 2 min_hits)')
    # the reference's flags keep few of the synthetic detections; the same numbers for a setting that keeps most of them
    dense = (2, 0, [0.3] * 4, [0.01] * 4)
    times = []
    for _ in range(5):
        t0 = time.perf_counter()
        o, _ = T.track_packed(packed, dense[3], dense[0], dense[1], dense[2])
        times.append(time.perf_counter() - t0)
    t_dense = float(np.median(times))
    say('    dense result (score >= 0.3, %d rows): track_packed median %.2f ms' % (len(o['frame']), 1e3 * t_dense))
    msd, motd = both([E.tracks_from_packed(packed, o)], ' dense')
    for name, ms, t in (('reference flags', ms1, t_track), ('dense', msd, t_dense)):
        say('expectation "scoring a result costs no more than producing it", %s, (a, K = 1) <= (c): %s (%.3f ms vs %.2f ms)'
            % (name, 'HOLDS' if ms <= 1e3 * t else 'DOES NOT HOLD', ms, 1e3 * t))
    say('identity / CLEAR-MOT kernel time: K = 1 %.2f x, K = 64 %.2f x, dense %.2f x' % (ms1 / mot1, ms64 / mot64, msd / motd))

    # (d) the CPU restatement, one segment
    if not args.no_cpu_reference:
        import mot_id_ref
        torch.set_num_threads(1)
        seg0 = gt['stream_keys'][0][0]
        rows = [r for r in T.format_tracks(packed, out) if r['image_id'].startswith(seg0 + '/')]
        gt0 = {'images': [im for im in gt_json['images'] if im['id'].startswith(seg0 + '/')],
               'annotations': [a for a in gt_json['annotations'] if a['image_id'].startswith(seg0 + '/')]}
        t0 = time.perf_counter()
        ref = mot_id_ref.evaluate(gt0, rows)
        t_ref = time.perf_counter() - t0
        say('(d) mot_id_ref (plain Python / numpy, one CPU thread) on ONE segment of that result: %.2f s -> about %.1f s for %d segments; '
            'ALL LEVEL_2 idtp of the segment %d' % (t_ref, t_ref * args.segments, args.segments, ref['table']['ALL'][2]['idtp']))
        say('    one result on the GPU is %.0f x faster than that; 64 in one launch %.0f x per result'
            % (t_ref * args.segments / (1e-3 * ms1), t_ref * args.segments / (1e-3 * ms64 / 64)))
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, 'wt') as fp:
        fp.write('\n'.join(lines) + '\n')


if __name__ == '__main__':
    main()
