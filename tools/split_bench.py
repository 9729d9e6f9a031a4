"""Cost and effect of splitting a tracking result next to producing, stitching and refining it (recorded in profiles/track_split.txt;
not a gate).

    python tools/split_bench.py [--segments 8] [--frames 198] [--objects 100] [--swaps 300] [--out profiles/track_split.txt]

On the config-1 size input of tools/stitch_bench.py (8 segments x 5 cameras x 198 frames), in ONE run on the same input:
  (a) wt_split_tracks_dev for J = 1 and J = 64 jobs on one tracked result, device events around repeated calls (inputs resident
      in HBM; the call never waits for the stream), with the breaks found and the workspace size;
  (b) wt_stitch_tracks_dev J = 1 and wt_refine_tracks plan + emit J = 1 on the same result;
  (c) utils.track_packed on the same detections (wt_track_streams_host, staging included), wall clock;
  (d) injected swaps: at `--swaps` places the ids of two trajectories of a stream that are both observed around a slot are
      exchanged from that slot on; ALL-level identity switches, IDF1, HOTA AssA and MOTA before the pass, after split, and after
      split + stitch.
The expectation to report against: splitting a result costs less than tracking it, (a, J = 1) < (c).
"""
import argparse
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def inject_swaps(np, packed, out, n_swaps, seed=5):
    """`out` with the ids of two trajectories of one stream exchanged from a slot on, at up to n_swaps places; a trajectory takes
    part in one swap at most, and both have at least three rows on either side of the slot.  Returns (rows, swaps made)."""
    rng = np.random.default_rng(seed)
    sfo = np.asarray(packed['stream_frame_offsets'], np.int64)
    frame, oid = np.asarray(out['frame'], np.int64), np.asarray(out['object_id']).copy()
    stream = np.searchsorted(sfo, frame, side='right') - 1
    made = 0
    per_stream = max(1, n_swaps // max(1, sfo.size - 1))
    for s in range(sfo.size - 1):
        rows = np.nonzero(stream == s)[0]
        ids = np.unique(oid[rows])
        rng.shuffle(ids)
        here = 0
        for a, b in zip(ids[0::2], ids[1::2]):
            if made >= n_swaps or here >= per_stream:
                break
            ra, rb = rows[oid[rows] == a], rows[oid[rows] == b]
            if min(ra.size, rb.size) < 6:
                continue
            lo = max(frame[ra][2], frame[rb][2]) + 1                     # at least three rows of each before the slot,
            hi = min(frame[ra][-3], frame[rb][-3])                       # and three from it on
            if lo > hi:
                continue
            cut = int(rng.integers(lo, hi + 1))
            oid[ra[frame[ra] >= cut]], oid[rb[frame[rb] >= cut]] = b, a
            made += 1
            here += 1
    return dict(out, object_id=oid), made


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--segments', type=int, default=8)
    ap.add_argument('--frames', type=int, default=198)
    ap.add_argument('--objects', type=int, default=100)
    ap.add_argument('--repeats', type=int, default=20)
    ap.add_argument('--rounds', type=int, default=5)
    ap.add_argument('--swaps', type=int, default=300)
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'track_split.txt'))
    args = ap.parse_args()
    import numpy as np
    import torch
    assert torch.cuda.is_available(), 'needs the GPU'
    from waymo_2d_tracking_amd import _lib, synthetic as syn
    from waymo_2d_tracking_amd.tracking import evaluate as E, refine as R, split as SP, stitch as S, utils as T
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
    for label, flags in (('max_age 1, score >= 0.3', (1, 0, [0.3] * 4, [0.01] * 4)),
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
        ref = R.DeviceRefine(packed, [out], [{'max_gap': 2, 'min_len': 3}])

        def both():
            ref.launch()
            ref.emit()
        say('(b) wt_refine_tracks plan + emit J = 1 (max_gap 2, min_len 3): median %.3f ms per pair (min %.3f, max %.3f)' % events(both))
        link = {'max_link': 5, 'link_iou': 0.3, 'motion': 'linear'}
        say('(b) wt_stitch_tracks_dev J = 1 (max_link 5, link_iou 0.3, linear): median %.3f ms per call (min %.3f, max %.3f)'
            % events(S.DeviceStitch(packed, [out], [link]).launch))
        ms_one = None
        for jobs, what in (([{'split_iou': 0.3}], 'split_iou 0.3, linear'),
                           ([{'split_iou': v, 'split_gap': g, 'motion': m} for v in (0.05, 0.1, 0.2, 0.3, 0.4, 0.5, 0.6, 0.7) for g in (0, 1, 2, 3)
                             for m in ('hold', 'linear')], 'split_iou 0.05 .. 0.7 x split_gap 0..3 x hold, linear')):
            dev = SP.DeviceSplit(packed, [out], jobs)
            ms, lo, hi = events(dev.launch)
            res = dev.results()
            J = len(jobs)
            made = [r['n_new'] for r in res]
            say('(a) wt_split_tracks_dev J = %d (%s): median %.3f ms per call = %.3f ms per job (min %.3f, max %.3f; %d windows of %d calls), '
                '%d rows, %d trajectories, most in one stream %d, workspace %.1f MiB, breaks per job %d .. %d'
                % (J, what, ms, ms / J, lo, hi, args.rounds, args.repeats, dev.p['n_rows'], dev.p['n_traj_total'], dev.max_traj,
                   dev.ws_bytes / 2.0 ** 20, min(made), max(made)))
            if J == 1:
                ms_one = ms
        verdicts.append('expectation "splitting a result costs less than tracking it", %s, (a, J = 1) < (c): %s (%.3f ms vs %.2f ms)'
                        % (label, 'HOLDS' if ms_one < t_track else 'DOES NOT HOLD', ms_one, t_track))
        swapped, n_made = inject_swaps(np, packed, out, args.swaps)
        cut = SP.split_tracks(packed, [swapped], [{'split_iou': 0.3}])[0]
        plain = S.stitch_tracks(packed, [swapped], [link])[0]
        linked = S.stitch_tracks(packed, [cut], [link])[0]
        results = (('tracked               ', out), ('swaps injected        ', swapped), ('swaps, stitch only    ', plain), ('swaps, split          ', cut),
                   ('swaps, split + stitch ', linked))
        tracks = [E.tracks_from_packed(packed, r) for _, r in results]
        p = E.pack_results(gt, tracks, 4)
        mot = E.evaluate_tracks(gt, tracks, packed=p)
        ident = E.evaluate_identity(gt, tracks, packed=p)
        hota = E.evaluate_hota(gt, tracks, packed=p)
        say('(d) %d swaps injected, %d breaks found at split_iou 0.3 linear; ALL LEVEL_2:' % (n_made, cut['n_new']))
        for k, (name, r) in enumerate(results):
            say('    %s idsw %d, IDF1 %.5f, HOTA AssA %.5f, MOTA %.5f, ids %d'
                % (name, mot[k].table['ALL'][2]['idsw'], ident[k].table['ALL'][2]['idf1'], hota[k].table['ALL'][2]['AssA'],
                   mot[k].table['ALL'][2]['MOTA'], np.unique(r['object_id']).size))
    for v in verdicts:
        say(v)
    say('what the pass is worth on real detections is not measured here: the input is synthetic and the swaps are injected')
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, 'wt') as fp:
        fp.write('\n'.join(lines) + '\n')


if __name__ == '__main__':
    main()
