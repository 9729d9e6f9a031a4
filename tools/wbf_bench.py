"""Cost of the weighted-boxes-fusion / NMW merge next to soft-NMS on the same input (recorded in profiles/wbf.txt; not a gate).

    python tools/wbf_bench.py [--segments 8] [--frames 198] [--objects 100] [--out profiles/wbf.txt]

The size is that of tools/det_eval_bench.py (8 segments x 5 cameras x 198 frames = 7920 images from synthetic.make_tracking_json;
the detections and a jittered copy of them are the two ensemble inputs).  Reported:
  (a) one wt_fuse_groups_dev call for weighted_fusion and for nmw, device events around batches of repeated calls (inputs
      resident in HBM, caller-owned workspace);
  (b) one wt_ensemble_groups_dev call with soft-NMS (--iou-thresh=0.5 --soft-nms-cut=0.9) on the same packed rows;
  (c) tests/wbf_ref.py on one CPU thread over the groups of the first --ref-images images, which are also compared with (a).
"""
import argparse
import ctypes as C
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
    ap.add_argument('--repeats', type=int, default=20, help='calls per timed batch')
    ap.add_argument('--batches', type=int, default=7)
    ap.add_argument('--ref-images', type=int, default=200)
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'wbf.txt'))
    args = ap.parse_args()
    import numpy as np
    import torch
    assert torch.cuda.is_available(), 'needs the GPU'
    import wbf_ref as R
    from waymo_2d_tracking_amd import _lib, synthetic as syn
    from waymo_2d_tracking_amd.detnet import ensemble as EN, ensemble_b as EB
    lib = _lib.lib()
    lib.wt_fuse_groups_workspace.restype = C.c_size_t
    lib.wt_fuse_groups_lds_rows.restype = C.c_int64
    lines = []

    def say(text):
        print(text, flush=True)
        lines.append(text)

    dets, _ = syn.make_tracking_json(1, n_segments=args.segments, n_frames=args.frames, n_objects=args.objects)
    rng = np.random.default_rng(2)
    second = [dict(r, bbox=[int(v + rng.integers(-3, 4)) for v in r['bbox'][:2]] + [max(1, int(v + rng.integers(-3, 4))) for v in r['bbox'][2:]],
                   score=round(float(np.clip(r['score'] + rng.normal(0, 0.02), 0.0, 1.0)), 5)) for r in dets]
    subs = [EN.submission_columns(dets), EN.submission_columns(second)]
    image_ids, category_ids, rows, wsum = EB.merge_inputs(subs)
    packed = EB.pack_groups(len(image_ids), category_ids, rows, 2, wsum)
    d5, off, gw, sizes = packed['dets5'], packed['group_offsets'], packed['group_wsum'], packed['input_sizes']
    G, n = packed['n_groups'], len(d5)
    per_group = np.diff(off)
    max_rows = int(per_group.max())
    say('device: %s' % (_lib.device_info(),))
    say('input: %d segments x 5 cameras x %d frames = %d images, 2 ensemble inputs of %d detections each -> %d rows in %d (image, category) '
        'groups (%d not empty; rows per group: mean %.1f, max %d; LDS holds %d)'
        % (args.segments, args.frames, len(image_ids), len(dets), n, G, int((per_group > 0).sum()), per_group[per_group > 0].mean(), max_rows,
           int(lib.wt_fuse_groups_lds_rows())))

    dev = torch.device('cuda', 0)
    t = dict(d5=torch.from_numpy(d5).to(dev), off=torch.from_numpy(off).to(dev), gw=torch.from_numpy(gw).to(dev),
             sizes=torch.from_numpy(np.ascontiguousarray(sizes)).to(dev), out5=torch.zeros((n, 5), dtype=torch.float64, device=dev),
             members=torch.zeros(n, dtype=torch.int32, device=dev), row_cluster=torch.zeros(n, dtype=torch.int32, device=dev),
             counts=torch.zeros(G, dtype=torch.int64, device=dev))
    p = lambda x: C.c_void_p(x.data_ptr())
    ws_fuse = int(lib.wt_fuse_groups_workspace(C.c_int64(n), C.c_int64(G), C.c_int64(max_rows)))
    ws_soft = int(lib.wt_ensemble_groups_workspace(C.c_int64(n), C.c_int64(G), C.c_int64(max_rows)))
    ws = torch.zeros(max(ws_fuse, ws_soft, 16), dtype=torch.uint8, device=dev)
    stream = lambda: C.c_void_p(torch.cuda.current_stream().cuda_stream)

    def fuse(method):
        _lib.check(lib.wt_fuse_groups_dev(p(t['d5']), p(t['off']), p(t['gw']), C.c_int64(n), C.c_int64(G), C.c_int64(max_rows), C.c_int(method),
                                          C.c_double(0.5), p(t['out5']), p(t['members']), p(t['row_cluster']), p(t['counts']), p(ws),
                                          C.c_size_t(ws_fuse), stream()), 'wt_fuse_groups_dev')

    def soft():
        _lib.check(lib.wt_ensemble_groups_dev(p(t['d5']), p(t['off']), p(t['sizes']), C.c_int64(n), C.c_int64(G), C.c_int64(max_rows), C.c_int(2),
                                              C.c_int(2), C.c_double(0.5), C.c_double(0.9), p(t['out5']), p(t['counts']), p(ws),
                                              C.c_size_t(ws_soft), stream()), 'wt_ensemble_groups_dev')

    def timed(fn):
        for _ in range(3):
            fn()
        torch.cuda.synchronize()
        ms = []
        for _ in range(args.batches):
            start, stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            start.record()
            for _ in range(args.repeats):
                fn()
            stop.record()
            stop.synchronize()
            ms.append(start.elapsed_time(stop) / args.repeats)
        return float(np.median(ms)), min(ms), max(ms)

    results = {}
    for code, name in ((0, 'weighted_fusion'), (1, 'nmw')):
        med, lo, hi = timed(lambda: fuse(code))
        got = (t['out5'].cpu().numpy(), t['counts'].cpu().numpy(), t['members'].cpu().numpy(), t['row_cluster'].cpu().numpy())
        results[name] = (med, got)
        say('(a) wt_fuse_groups_dev -m %s --iou-thresh=0.5: median %.3f ms per call over %d batches of %d calls (min %.3f, max %.3f), %d merged rows, '
            '%d of them with more than one member, workspace %d B'
            % (name, med, args.batches, args.repeats, lo, hi, int(got[1].sum()), int(sum((got[2][o:o + c] > 1).sum() for o, c in zip(off[:-1].tolist(), got[1].tolist()))), ws_fuse))
    med_soft, lo, hi = timed(soft)
    say('(b) wt_ensemble_groups_dev -m soft_nms --iou-thresh=0.5 --soft-nms-cut=0.9 on the same rows: median %.3f ms per call (min %.3f, max %.3f), %d rows out'
        % (med_soft, lo, hi, int(t['counts'].sum().item())))

    torch.set_num_threads(1)
    g_hi = min(G, args.ref_images * packed['ncat'])
    r_hi = int(off[g_hi])
    for name in ('weighted_fusion', 'nmw'):
        t0 = time.perf_counter()
        ref = R.fuse_groups(d5[:r_hi], off[:g_hi + 1], gw[:g_hi], name, 0.5)
        sec = time.perf_counter() - t0
        got = results[name][1]
        same = np.array_equal(got[1][:g_hi], ref[1]) and np.array_equal(got[3][:r_hi], ref[3]) and all(
            np.array_equal(got[0][o:o + c], ref[0][o:o + c]) and np.array_equal(got[2][o:o + c], ref[2][o:o + c]) for o, c in zip(off[:g_hi].tolist(), ref[1].tolist()))
        say('(c) tests/wbf_ref.py -m %s, one CPU thread, the %d groups (%d rows) of the first %d images: %.3f s = %.1f ms scaled to all rows; '
            'device output on these groups %s' % (name, g_hi, r_hi, g_hi // packed['ncat'], sec, 1e3 * sec * n / max(r_hi, 1), 'EQUAL' if same else 'DIFFERS'))
    for name in ('weighted_fusion', 'nmw'):
        say('%s / soft_nms device time: %.2f' % (name, results[name][0] / med_soft))
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, 'wt') as fp:
        fp.write('\n'.join(lines) + '\n')


if __name__ == '__main__':
    main()
