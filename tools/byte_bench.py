"""Cost and effect of the tracker's second association with low-score detections (recorded in profiles/track_byte.txt; not a gate).

    python tools/byte_bench.py [--segments 8] [--frames 198] [--objects 100] [--low 0.3] [--out profiles/track_byte.txt]

On the config-1 size input of the other track_* benches (8 segments x 5 cameras x 198 frames, synthetic.make_tracking_json), in ONE
process on the same input:
  (a) plain tracking at the reference thresholds (--score-threshold 0.95,0.6,1.0,0.9),
  (b) plain tracking with every class at the low threshold,
  (c) the second association with high = (a) and low = (b), low_iou 0.5.
Each is timed twice: the device-resident entry point (wt_track_streams_dev / wt_track_streams_byte_dev, inputs in HBM, device events
around windows of repeated calls after a warm-up) and the host call (utils.track_packed / track_packed_byte, staging included, wall
clock).  Rows out and ALL-level LEVEL_2 MOTA, IDF1 and HOTA follow for the three results.  No ratio is fixed in advance: the last
lines state whether (c) costs more than (b) and whether it scores above both (a) and (b).
--append FILE... adds the text of further files (register counts, bench.py lines of this tree and its parent) under the table.
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
    ap.add_argument('--low', type=float, default=0.3)
    ap.add_argument('--low-iou', type=float, default=0.5)
    ap.add_argument('--max-age', type=int, default=1)
    ap.add_argument('--repeats', type=int, default=5)
    ap.add_argument('--rounds', type=int, default=5)
    ap.add_argument('--append', nargs='*', default=[])
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'track_byte.txt'))
    args = ap.parse_args()
    import numpy as np
    import torch
    assert torch.cuda.is_available(), 'needs the GPU'
    from waymo_2d_tracking_amd import _lib, synthetic as syn
    from waymo_2d_tracking_amd.devpath import DeviceTracker, DeviceTrackerByte
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
    high, iou = [0.95, 0.6, 1.0, 0.9], [0.01, 0.01, 1.0, 0.0]
    low = [min(args.low, h) for h in high]
    low_iou = [args.low_iou] * 4
    between = sum(int(np.sum((packed['category'] == c + 1) & (packed['score'] >= low[c]) & (packed['score'] < high[c]))) for c in range(4))
    say('device: %s' % (_lib.device_info(),))
    say('input: %d segments x 5 cameras x %d frames, %d detections (%d of them between the low and the high threshold of their class), '
        '%d ground-truth boxes, %d streams; max_age %d, min_hits 0, iou %s'
        % (args.segments, args.frames, packed['x'].size, between, gt['x'].size, len(gt['stream_keys']), args.max_age, iou))

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

    def wall(fn):
        fn()
        times = []
        for _ in range(7):
            t0 = time.perf_counter()
            fn()
            times.append(time.perf_counter() - t0)
        return 1e3 * float(np.median(times)), 1e3 * min(times), 1e3 * max(times)

    runs = (('(a) track_packed, reference thresholds %s' % high,
             lambda: DeviceTracker(packed, iou, args.max_age, 0, high), lambda: T.track_packed(packed, iou, args.max_age, 0, high)),
            ('(b) track_packed, every class at the low threshold %s' % low,
             lambda: DeviceTracker(packed, iou, args.max_age, 0, low), lambda: T.track_packed(packed, iou, args.max_age, 0, low)),
            ('(c) track_packed_byte, high %s, low %s, low_iou %s' % (high, low, args.low_iou),
             lambda: DeviceTrackerByte(packed, iou, args.max_age, 0, high, low, low_iou),
             lambda: T.track_packed_byte(packed, iou, args.max_age, 0, high, low, low_iou)))
    outs, dev_ms = [], []
    for label, make, host in runs:
        dev = make()
        ms = events(dev.run)
        out, births = dev.results()
        hout, hbirths = host()
        assert hbirths == births and all(np.array_equal(out[k], hout[k]) for k in out), 'device and host form differ'
        w = wall(host)
        say(label + ':')
        say('    device form: median %.3f ms per call (min %.3f, max %.3f; %d windows of %d calls), workspace %.1f MiB; '
            'host call, staging included: median %.2f ms of 7 (min %.2f, max %.2f); %d rows out, %d ids'
            % (ms + (args.rounds, args.repeats, dev.ws_bytes / 2.0 ** 20) + w + (len(out['frame']), births)))
        outs.append(out)
        dev_ms.append(ms[0])
        del dev
    tracks = [E.tracks_from_packed(packed, o) for o in outs]
    p = E.pack_results(gt, tracks, 4)
    mot = E.evaluate_tracks(gt, tracks, packed=p)
    ident = E.evaluate_identity(gt, tracks, packed=p)
    hota = E.evaluate_hota(gt, tracks, packed=p)
    say('ALL LEVEL_2:')
    scores = []
    for k, name in enumerate(('(a)', '(b)', '(c)')):
        r = mot[k].table['ALL'][2]
        scores.append((r['MOTA'], ident[k].table['ALL'][2]['idf1'], hota[k].table['ALL'][2]['HOTA']))
        say('    %s rows %d, tp %d, fn %d, fp %d, idsw %d, MOTA %.5f, IDF1 %.5f, HOTA %.5f'
            % ((name, len(outs[k]['frame']), r['tp'], r['fn'], r['fp'], r['idsw']) + scores[-1]))
    say('(c) costs %s than (b): %.3f ms vs %.3f ms per device call.'
        % ('more' if dev_ms[2] > dev_ms[1] else 'no more', dev_ms[2], dev_ms[1]))
    above = [n for i, n in enumerate(('MOTA', 'IDF1', 'HOTA')) if scores[2][i] > scores[0][i] and scores[2][i] > scores[1][i]]
    say('(c) scores above both (a) and (b) in: %s.' % (', '.join(above) if above else 'none of MOTA, IDF1, HOTA'))
    for path in args.append:
        with open(path) as fp:
            lines.append(fp.read().rstrip('\n'))
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, 'wt') as fp:
        fp.write('\n'.join(lines) + '\n')


if __name__ == '__main__':
    main()
