"""Cost of scoring HOTA next to CLEAR-MOT and identity scoring and next to producing the result
(recorded in profiles/mot_hota.txt; not a gate).

    python tools/mot_hota_bench.py [--segments 8] [--frames 198] [--objects 100] [--out profiles/mot_hota.txt]

Input and method of tools/mot_identity_bench.py (8 segments x 5 cameras x 198 frames), in ONE run on the same input:
  (a) wt_mot_hota_dev for K = 1, K = 64 and the dense result, device events around repeated launches after 3 warm-ups (inputs
      resident in HBM), with the workspace bytes and, at K = 64, the calls the default workspace limit splits evaluate_hota into;
  (b) wt_mot_eval_dev and wt_mot_identity_dev for the same results;
  (c) utils.track_packed on the same detections (wt_track_streams_host, staging included), wall clock;
  (d) tests/hota_ref.py, the plain-Python restatement, on ONE stream of one result on one CPU thread (scaled to all).
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
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'mot_hota.txt'))
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

    def time_track(setting):
        T.track_packed(packed, setting[3], setting[0], setting[1], setting[2])
        times = []
        for _ in range(5):
            t0 = time.perf_counter()
            out, _ = T.track_packed(packed, setting[3], setting[0], setting[1], setting[2])
            times.append(time.perf_counter() - t0)
        return out, float(np.median(times)), times

    # (c) the tracker
    reference = (2, 0, [0.95, 0.6, 1.0, 0.9], [0.01, 0.01, 1.0, 0.0])           # the reference README's flags
    out, t_track, times = time_track(reference)
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

    def all_three(tracks, label):
        K = len(tracks)
        hota = E.DeviceHota(gt, tracks)
        ms_h = time_dev(hota)
        r = hota.results()[0].table['ALL'][2]
        cells = E._matrix_cells(hota.g_ntraj, hota.h_ntraj)
        say('(a) wt_mot_hota_dev     K = %d%s: %.3f ms per launch = %.3f ms per result (events around %d launches), %d wavefronts, '
            'workspace %.1f MiB (%d cells of 46 bytes), at most %d boxes of a class in a frame, largest problem %d cells a level'
            % (K, label, ms_h, ms_h / K, args.repeats, 2 * K * len(gt['stream_keys']) * 4, hota.ws_bytes / 2.0 ** 20, hota.matrix_cells,
               hota.max_boxes, int(cells.max()) // 2))
        say('    first result, ALL LEVEL_2: %s' % dict((k, round(r[k], 6)) for k in ('HOTA', 'DetA', 'AssA', 'LocA', 'HOTA(0)')))
        calls = E._hota_calls(_lib.lib(), hota.g_ntraj, hota.h_ntraj, hota.max_boxes, E.DEFAULT_WORKSPACE_LIMIT)
        say('    evaluate_hota under the default workspace limit of %d MiB: %d call(s)' % (E.DEFAULT_WORKSPACE_LIMIT >> 20, len(calls)))
        del hota
        ident, mot = E.DeviceIdentity(gt, tracks), E.DeviceEvaluation(gt, tracks)
        ms_id, ms_mot = time_dev(ident), time_dev(mot)
        say('(b) wt_mot_identity_dev K = %d%s: %.3f ms per launch = %.3f ms per result, workspace %.1f MiB'
            % (K, label, ms_id, ms_id / K, ident.ws_bytes / 2.0 ** 20))
        say('(b) wt_mot_eval_dev     K = %d%s: %.3f ms per launch = %.3f ms per result' % (K, label, ms_mot, ms_mot / K))
        return ms_h, ms_id, ms_mot

    h1, i1, m1 = all_three([one], '')
    many = []
    for max_age in (1, 2):
        for min_hits in (0, 1):
            for score in (0.3, 0.5, 0.7, 0.9):
                for iou in (0.0, 0.01, 0.1, 0.3):
                    o, _ = T.track_packed(packed, [iou] * 4, max_age, min_hits, [score] * 4)
                    many.append(E.tracks_from_packed(packed, o))
    h64, i64, m64 = all_three(many, ' (4 score x 4 IoU thresholds x 2 max_age x 2 min_hits)')
    del many
    # the reference's flags keep few of the synthetic detections; the same numbers for a setting that keeps most of them
    o, t_dense, _ = time_track((2, 0, [0.3] * 4, [0.01] * 4))
    say('    dense result (score >= 0.3, %d rows): track_packed median %.2f ms' % (len(o['frame']), 1e3 * t_dense))
    hd, idd, md = all_three([E.tracks_from_packed(packed, o)], ' dense')
    for name, ms, t in (('reference flags', h1, t_track), ('dense', hd, t_dense)):
        say('expectation "scoring a result costs no more than producing it", %s, (a, K = 1) <= (c): %s (%.3f ms vs %.2f ms)'
            % (name, 'HOLDS' if ms <= 1e3 * t else 'DOES NOT HOLD', ms, 1e3 * t))
    say('HOTA / CLEAR-MOT kernel time: K = 1 %.2f x, K = 64 %.2f x, dense %.2f x' % (h1 / m1, h64 / m64, hd / md))
    say('HOTA / identity kernel time:  K = 1 %.2f x, K = 64 %.2f x, dense %.2f x' % (h1 / i1, h64 / i64, hd / idd))

    # (d) the CPU restatement, one stream
    if not args.no_cpu_reference:
        import hota_ref
        torch.set_num_threads(1)
        seg0, cam0 = gt['stream_keys'][0]
        mine = lambda image_id: image_id.startswith(seg0 + '/') and image_id.endswith('/' + cam0)
        rows = [r for r in T.format_tracks(packed, out) if mine(r['image_id'])]
        gt0 = {'images': [im for im in gt_json['images'] if mine(im['id'])],
               'annotations': [a for a in gt_json['annotations'] if mine(a['image_id'])]}
        t0 = time.perf_counter()
        ref = hota_ref.evaluate(gt0, rows)
        t_ref = time.perf_counter() - t0
        n_streams = len(gt['stream_keys'])
        say('(d) hota_ref (plain Python / numpy, one CPU thread) on ONE stream of that result: %.2f s -> about %.1f s for %d streams; '
            'ALL LEVEL_2 HOTA of the stream %.6f' % (t_ref, t_ref * n_streams, n_streams, ref['table']['ALL'][2]['HOTA']))
        say('    one result on the GPU is %.0f x faster than that; 64 in one launch %.0f x per result'
            % (t_ref * n_streams / (1e-3 * h1), t_ref * n_streams / (1e-3 * h64 / 64)))
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, 'wt') as fp:
        fp.write('\n'.join(lines) + '\n')


if __name__ == '__main__':
    main()
