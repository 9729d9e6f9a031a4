"""Cost and effect of linking a tracking result across classes next to producing and stitching it (recorded in
profiles/track_xlink.txt; not a gate).

    python tools/xlink_bench.py [--segments 8] [--frames 198] [--objects 100] [--out profiles/track_xlink.txt]

On the config-1 size input of tools/stitch_bench.py (8 segments x 5 cameras x 198 frames; SYNTHETIC detections), tracked, with
class flicker injected into the tracked rows - in every third trajectory of at least six rows the middle third of the rows moves to
a fresh id and the other class of {2, 4} (class 2 otherwise) and the last third to a second fresh id, the injection of
tests/xlink_cases.py - in ONE run on the same rows:
  (a) wt_xlink_tracks_dev for J = 1 and J = 64 jobs, device events around repeated calls (inputs resident in HBM; the call never
      waits for the stream), with the workspace, the links made, the rows relabelled and the rounds of the matching;
  (b) wt_stitch_tracks_dev J = 1 on the same rows;
  (c) utils.track_packed on the same detections (wt_track_streams_host, staging included), wall clock;
  (d) identity switches, fp, fn, MOTA, IDF1 and HOTA AssA at LEVEL_2, for ALL and for classes 2 and 4, before and after the pass.
The expectation to report against: linking a result across classes costs less than tracking it, (a, J = 1) < (c).
"""
import argparse
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def inject_flicker(np, out):
    """the injection of tests/xlink_cases.py (inject_flicker), one pass over the rows sorted by (id, frame); returns (rows, pieces moved)"""
    frame, cat, oid = np.asarray(out['frame']), np.asarray(out['category']).copy(), np.asarray(out['object_id']).copy()
    order = np.lexsort((frame, oid))
    ids, start, count = np.unique(oid[order], return_index=True, return_counts=True)
    first_row = np.asarray([order[s:s + c].min() for s, c in zip(start, count)])      # trajectories in order of first appearance in the rows
    by_appearance = np.argsort(first_row, kind='stable')
    long_ones = [k for k in by_appearance if count[k] >= 6][::3]
    fresh = int(oid.max()) + 1
    for k in long_ones:
        rows = order[start[k]:start[k] + count[k]]
        n = rows.size
        cls = int(cat[rows[0]])
        cat[rows[n // 3:2 * n // 3]] = {2: 4, 4: 2}.get(cls, 2)
        oid[rows[n // 3:2 * n // 3]] = fresh
        oid[rows[2 * n // 3:]] = fresh + 1
        fresh += 2
    return dict(out, category=cat, object_id=oid), len(long_ones)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--segments', type=int, default=8)
    ap.add_argument('--frames', type=int, default=198)
    ap.add_argument('--objects', type=int, default=100)
    ap.add_argument('--repeats', type=int, default=20)
    ap.add_argument('--rounds', type=int, default=5)
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'track_xlink.txt'))
    args = ap.parse_args()
    import numpy as np
    import torch
    assert torch.cuda.is_available(), 'needs the GPU'
    from waymo_2d_tracking_amd import _lib, synthetic as syn
    from waymo_2d_tracking_amd.tracking import evaluate as E, stitch as S, utils as T, xlink as X
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
    say('input (SYNTHETIC, waymo_2d_tracking_amd.synthetic seed 1; class flicker injected into the tracked rows): %d segments x 5 cameras x %d frames, '
        '%d detections, %d ground-truth boxes, %d streams' % (args.segments, args.frames, packed['x'].size, gt['x'].size, len(gt['stream_keys'])))

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

    both = lambda g, v: {(2, 4): {'max_link': g, 'link_iou': v}, (1, 2): {'max_link': g, 'link_iou': v}}
    one = [{'pairs': both(2, 0.3), 'prio': 0, 'motion': 'linear'}]
    many = [{'pairs': both(g, v), 'prio': 0, 'motion': m} for g in range(1, 9) for v in (0.1, 0.3, 0.5, 0.7) for m in ('hold', 'linear')]
    verdicts = []
    for label, flags in (('max_age 1, score >= 0.3', (1, 0, [0.3] * 4, [0.01] * 4)),
                         ('reference flags, max_age 1', (1, 0, [0.95, 0.6, 1.0, 0.9], [0.01, 0.01, 1.0, 0.0]))):
        T.track_packed(packed, flags[3], flags[0], flags[1], flags[2])
        times = []
        for _ in range(7):
            t0 = time.perf_counter()
            tracked, _ = T.track_packed(packed, flags[3], flags[0], flags[1], flags[2])
            times.append(time.perf_counter() - t0)
        t_track = 1e3 * float(np.median(times))
        out, moved = inject_flicker(np, tracked)
        say('%s:' % label)
        say('(c) track_packed (host call, staging included): median %.2f ms of 7 (min %.2f, max %.2f), %d rows; flicker injected into %d trajectories'
            % (t_track, 1e3 * min(times), 1e3 * max(times), len(out['frame']), moved))
        st = S.DeviceStitch(packed, [out], [{'max_link': 2, 'link_iou': 0.3, 'motion': 'linear'}])
        say('(b) wt_stitch_tracks_dev J = 1 (max_link 2, link_iou 0.3, linear): median %.3f ms per call (min %.3f, max %.3f), %d links'
            % (events(st.launch) + (int(st.results()[0]['n_links'].sum()),)))
        ms_one = None
        for jobs, what in ((one, 'pairs 2:4 and 1:2, max_link 2, link_iou 0.3, linear'),
                           (many, 'the two pairs, max_link 1..8 x link_iou 0.1, 0.3, 0.5, 0.7 x hold, linear')):
            dev = X.DeviceXLink(packed, [out], jobs)
            ms, lo, hi = events(dev.launch)
            res = dev.results()
            rounds = dev.rounds()
            J = len(jobs)
            made = [int(r['n_links'].sum()) for r in res]
            moved_back = [int(r['n_relabelled'].sum()) for r in res]
            say('(a) wt_xlink_tracks_dev J = %d (%s): median %.3f ms per call = %.3f ms per job (min %.3f, max %.3f; %d windows of %d calls), '
                '%d problems, %d rows, %d trajectories, most in one stream %d, workspace %.1f MiB, links per job %d .. %d, rows relabelled per job %d .. %d, '
                'rounds of the matching per (job, stream) %d .. %d'
                % (J, what, ms, ms / J, lo, hi, args.rounds, args.repeats, J * dev.p['n_streams'], dev.p['n_rows'], dev.p['n_traj_total'], dev.max_traj,
                   dev.ws_bytes / 2.0 ** 20, min(made), max(made), min(moved_back), max(moved_back), int(rounds.min()), int(rounds.max())))
            if J == 1:
                ms_one = ms
                tracks = [E.tracks_from_packed(packed, out), E.tracks_from_packed(packed, res[0])]
                p = E.pack_results(gt, tracks, 4)
                mot = E.evaluate_tracks(gt, tracks, packed=p)
                ident = E.evaluate_identity(gt, tracks, packed=p)
                hota = E.evaluate_hota(gt, tracks, packed=p)
                say('(d) %d links, %d rows relabelled; LEVEL_2 before -> after the pass:' % (made[0], moved_back[0]))
                for c in ('ALL', 2, 4):
                    a, b = mot[0].table[c][2], mot[1].table[c][2]
                    say('    class %-3s idsw %d -> %d, fp %d -> %d, fn %d -> %d, MOTA %.5f -> %.5f, IDF1 %.5f -> %.5f, HOTA AssA %.5f -> %.5f'
                        % (c, a['idsw'], b['idsw'], a['fp'], b['fp'], a['fn'], b['fn'], a['MOTA'], b['MOTA'], ident[0].table[c][2]['idf1'],
                           ident[1].table[c][2]['idf1'], hota[0].table[c][2]['AssA'], hota[1].table[c][2]['AssA']))
        verdicts.append('expectation "linking across classes costs less than tracking the result", %s, (a, J = 1) < (c): %s (%.3f ms vs %.2f ms)'
                        % (label, 'HOLDS' if ms_one < t_track else 'DOES NOT HOLD', ms_one, t_track))
    for v in verdicts:
        say(v)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, 'wt') as fp:
        fp.write('\n'.join(lines) + '\n')


if __name__ == '__main__':
    main()
