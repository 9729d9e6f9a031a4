"""Multi-view detect -> ensemble -> SORT pipeline against its single views, in one invocation; prints one JSON line.

    python tools/views_bench.py [--steps 12] [--warmup 3] [--height 1280 --width 1920] [--method soft_nms] [--views-only]

Each configuration is DetectTrackPipeline at the bench's settings (5 cameras x 2 frames per step, 2 frames in flight, deferred
tracking, captured graphs): views=('orig', 'x1.5,hflip') merged by --method (default soft-NMS; cut 0.9, min_score 0.01;
weighted_fusion_b / nmw are the rules of detnet.ensemble_b), then each view alone (tta='' and tta='x1.5,hflip'; --views-only skips
them, to time several merge rules in one session).  Reported per configuration: frames/s over the timed steps and the peak device memory
(torch.cuda.max_memory_reserved: graph pools included).  For the two-view run also the merge (wt_ensemble_slots_dev, both
launches) per chunk from HIP events around it on the track stream, and the ratio of its rate to the serial-composition
estimate 1 / (1 / r_orig + 1 / r_x1.5hflip)."""
import argparse
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import torch  # noqa: E402

from waymo_2d_tracking_amd.bench_e2e import DetectTrackPipeline  # noqa: E402

VIEWS = ('orig', 'x1.5,hflip')
VIEW_ENS = dict(method='soft_nms', iou_thresh=0.5, soft_nms_cut=0.9, min_score=0.01, weights=None)


def measure(args, **kw):
    torch.cuda.empty_cache()
    torch.cuda.reset_peak_memory_stats()
    pipe = DetectTrackPipeline(5, 2, height=args.height, width=args.width, seed=0, n_inflight=2, defer_tracking=True, **kw)
    pipe._capture()
    for _ in range(args.warmup):
        pipe.step()
    pipe.flush()
    torch.cuda.synchronize()
    if pipe.ensemble is not None:
        pipe.merge_events = []
    t0 = time.perf_counter()
    for _ in range(args.steps):
        pipe.step()
    pipe.flush()
    torch.cuda.synchronize()
    dt = time.perf_counter() - t0
    out = dict(frames_per_s=pipe.n_frames * args.steps / dt, ms_per_frame=1e3 * dt / (pipe.n_frames * args.steps),
               peak_reserved_gb=torch.cuda.max_memory_reserved() / 2 ** 30, peak_allocated_gb=torch.cuda.max_memory_allocated() / 2 ** 30)
    if pipe.merge_events:
        ms = [a.elapsed_time(b) for a, b in pipe.merge_events]
        out.update(merge_us_per_chunk=1e3 * sum(ms) / len(ms), merge_us_max=1e3 * max(ms), merge_chunks=len(ms),
                   merged_rows_last_chunk=int(pipe.merge_counts[(pipe.chunk - 1) % pipe.max_chunks].sum()))
    del pipe
    torch.cuda.synchronize()
    return out


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument('--steps', type=int, default=12)
    ap.add_argument('--warmup', type=int, default=3)
    ap.add_argument('--height', type=int, default=1280)
    ap.add_argument('--width', type=int, default=1920)
    ap.add_argument('--method', default=VIEW_ENS['method'], choices=('weighted_fusion', 'nms', 'soft_nms', 'weighted_fusion_b', 'nmw'),
                    help='merge rule of the two-view run (the other settings stay: iou 0.5, cut 0.9, min_score 0.01)')
    ap.add_argument('--views-only', action='store_true', help='skip the two single-view runs and the figures derived from them')
    args = ap.parse_args(argv)
    res = dict(workload='DetectTrackPipeline %dx%d, 5 cameras x 2 frames per step, 2 lanes, deferred tracking' % (args.width, args.height),
               steps=args.steps, warmup=args.warmup, method=args.method)
    res['views'] = measure(args, views=VIEWS, view_ensemble=dict(VIEW_ENS, method=args.method))
    if args.views_only:
        v = res['views']
        res['merge_share_of_chunk_time'] = v['merge_us_per_chunk'] * 1e-3 / (v['ms_per_frame'] * 10)
        print(json.dumps(res))
        return
    res['orig'] = measure(args, tta='')
    res['x1.5,hflip'] = measure(args, tta='x1.5,hflip')
    r0, r1 = res['orig']['frames_per_s'], res['x1.5,hflip']['frames_per_s']
    serial = 1.0 / (1.0 / r0 + 1.0 / r1)
    v = res['views']
    res['serial_estimate_frames_per_s'] = serial
    res['views_vs_serial_estimate'] = v['frames_per_s'] / serial
    # the merge runs once per chunk of 10 frames on the track stream, under the next chunk's detector work
    res['merge_share_of_chunk_time'] = v['merge_us_per_chunk'] * 1e-3 / (v['ms_per_frame'] * 10)
    print(json.dumps(res))


if __name__ == '__main__':
    main()
